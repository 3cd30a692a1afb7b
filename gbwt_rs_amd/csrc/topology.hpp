// topology.hpp -- launch wrappers of topology.hip: the graph API (node ids, edge rows, link rows) and the H-/S-/L-lines of a GFA file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_index.hpp"
#include "kernels.hpp"

namespace gbwt_hip {

// A row of at most this many edges is decoded and written by the lane that owns the query; a longer one is handed to a workgroup
// (k_edge_fill_big).  One wave's width: a lane that writes its row holds the other 63 lanes of its wave for as many iterations as the
// row has edges, and from 64 edges on a wave can store whole 512-byte stretches of the row at once.
constexpr uint32_t EDGE_LANE_MAX = 64;
constexpr uint32_t EDGE_BIG_BLOCKS = 256;     // workgroups of k_edge_fill_big (they loop over the list of long rows)
constexpr uint32_t TEXT_STRETCH = 4096;       // output bytes of one workgroup of k_segment_lines: 256 lanes x 16 bytes

// node slots of a handle (kernels.hpp: ComponentGeometry): GBZ::min_node .. GBZ::max_node
inline ComponentGeometry graph_geometry(const DeviceIndex &d) {
    ComponentGeometry g{0, 0};
    if (d.n_records > 1) {
        g.min_node = d.first_node >> 1;
        g.slots = ((static_cast<uint64_t>(d.alphabet_offset) + d.n_records - 1) >> 1) - g.min_node + 1;
    }
    return g;
}

// The node-to-segment translation in HBM (gbwt_hip_index::seg_*; null pointers and segments = 0 without one) and the labels
struct GraphTables {
    const uint32_t *seg_of;        // [mapping_len]
    const uint32_t *seg_start;     // [segments + 1]
    const uint64_t *name_off;      // [segments + 1]
    const uint8_t *names;
    const uint64_t *seq_len;       // [segments]
    const uint8_t *node_real;      // [mapping_len]
    uint64_t mapping_len, segments;
    const uint8_t *label_bytes;    // labels of the potential nodes (sequences.hip: ensure_labels), or null
    const uint64_t *label_off;
    uint64_t labels;
    uint32_t first_node;
};

// flags[s] = 1 where the node of slot s exists (GBZ::has_node), else 0
void launch_node_flags(const DeviceIndex &ix, const ComponentGeometry &g, uint64_t *d_flags, hipStream_t s);
// flags[s] = 1 where the first node of segment s exists (GBZ::segment_iter, src/gbz.rs:927-929)
void launch_segment_flags(const GraphTables &t, uint64_t *d_flags, hipStream_t s);
// out[rank[s]] = base + s for every s < n with rank[s + 1] > rank[s] (rank = the exclusive scan of the flags, n + 1 entries)
void launch_scatter_ids(const uint64_t *d_rank, uint64_t n, uint64_t base, uint64_t *d_out, hipStream_t s);
// queries 2 s + o over all slots: ids[2 s + o] = min_node + s, orient[2 s + o] = o
void launch_all_node_queries(const ComponentGeometry &g, uint64_t *d_ids, uint8_t *d_orient, hipStream_t s);
// boundary nodes of segments (GBZ::segment_successors / _predecessors, src/gbz.rs:402-440): query k = (seg_ids[k], orient[k]), or, with
// seg_ids == null, query 2 s + o = (segment s, o) over all segments and only where the first node of the segment exists (segment_iter);
// out_ids[k] = 0 (no node) for a segment that is out of range, empty or left out
void launch_link_queries(const GraphTables &t, const uint64_t *d_seg_ids, const uint8_t *d_orient, uint64_t n, bool predecessors, uint64_t *d_out_ids, uint8_t *d_out_orient,
                         hipStream_t s);
// edge rows: counts (and valid) per query, then -- at the offsets of their scan -- the rows; d_rows (or null) receives the query of every
// edge; d_big: n u32 + one counter in front (zeroed by launch_edge_fill)
void launch_edge_count(const DeviceIndex &ix, const uint64_t *d_ids, const uint8_t *d_orient, uint64_t n, bool flip, uint64_t *d_counts, uint8_t *d_valid, hipStream_t s);
void launch_edge_fill(const DeviceIndex &ix, const uint64_t *d_ids, const uint8_t *d_orient, uint64_t n, bool flip, const uint64_t *d_offsets, uint64_t *d_edges, uint32_t *d_rows,
                      uint32_t *d_big, hipStream_t s);
// link rows from edge rows: cut[r] = edges of row r in front of the first node without a segment; then the rows at the scan of the cuts
void launch_link_cut(const GraphTables &t, const uint64_t *d_offsets, const uint64_t *d_edges, const uint32_t *d_rows, uint64_t n, uint64_t total, uint64_t *d_cut, hipStream_t s);
void launch_link_write(const GraphTables &t, const uint64_t *d_offsets, const uint64_t *d_edges, const uint32_t *d_rows, uint64_t total, const uint64_t *d_cut,
                       const uint64_t *d_link_offsets, uint64_t *d_links, hipStream_t s);
// S-lines: sizes of the lines of the items (node ids, or segment ids with a translation), then the text at the scan of the sizes, from byte
// `base` of d_text (a hipMalloc'ed buffer: the kernel stores aligned 16-byte units of it)
void launch_segment_line_sizes(const GraphTables &t, const uint64_t *d_items, uint64_t items, bool translated, uint64_t *d_sizes, hipStream_t s);
void launch_segment_lines(const GraphTables &t, const uint64_t *d_items, uint64_t items, bool translated, const uint64_t *d_line_off, uint64_t base, uint64_t bytes, char *d_text,
                          hipStream_t s);
// L-lines over the edge rows of all (node | segment, orientation) queries: the size of the line of every edge (0: not canonical, or behind
// the cut; d_cut == null: no cut) and their number (*d_lines, zeroed by the caller), then the lines at the scan of the sizes from byte `base`
void launch_link_line_sizes(const GraphTables &t, const ComponentGeometry &g, bool translated, const uint64_t *d_offsets, const uint64_t *d_edges, const uint32_t *d_rows,
                            uint64_t total, const uint64_t *d_cut, uint64_t *d_sizes, uint64_t *d_lines, hipStream_t s);
void launch_link_lines(const GraphTables &t, const ComponentGeometry &g, bool translated, const uint64_t *d_edges, const uint32_t *d_rows, uint64_t total,
                       const uint64_t *d_line_off, uint64_t base, char *d_text, hipStream_t s);

}  // namespace gbwt_hip
