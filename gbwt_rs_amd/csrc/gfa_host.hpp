// gfa_host.hpp -- what gfa_host.cpp does on the host image of an index (plain C++, no HIP): reading nodes, edges and segments from it, the
// replay of the reference's segment path iterator, and the graph lines of a GFA file.
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

#include "host_index.hpp"
#include "positional_file.hpp"

namespace gbwt_hip {

// GBZ::has_node (src/gbz.rs:286-289) on the host image (makes the host's records on first use: HostIndex::ensure_records)
bool node_exists(const HostIndex &h, uint64_t node_id);
// Edge list of a record, decoded on the host (Record::decompress_edges, src/bwt.rs:378-395) for the L-lines: (node, offset) pairs; false
// for a record that is out of range, empty or malformed
bool host_edges(const HostIndex &h, uint64_t rec, std::vector<std::pair<uint64_t, uint64_t>> &edges);

// Graph::segment / node_to_segment (src/graph.rs:172-198): node range [start, end) of a segment, the segment of a node (which must lie in
// [segment_starts[0], mapping_len)), and the length of its sequence
struct HostSegment { uint64_t id, start, end; };
HostSegment host_segment(const HostIndex &h, uint64_t id);
HostSegment host_node_to_segment(const HostIndex &h, uint64_t node_id);
uint64_t host_segment_seq_len(const HostIndex &h, const HostSegment &s);

// SegmentPathIter (src/gbz.rs:1098-1169) over the node ids of one path (GBWT nodes: id << 1 | orientation): the (segment, orientation)
// tokens up to the point where the reference's iterator stops, and the summed segment lengths
void host_segment_path(const HostIndex &h, const uint32_t *nodes, uint64_t len, std::vector<std::pair<uint64_t, bool>> &tokens, uint64_t &seq_len);

// H-, S- and L-lines of the whole graph (write_gfa_header / write_segments / write_links, src/bin/gbunzip.rs:193-317) into `file` from its
// first byte on; returns the bytes written.  Serial host work in the reference; here the node (or segment) ids are cut into ranges that up
// to eight threads turn into text side by side (config 4's 462 MB of S- and L-lines: 1 090 ms on one thread); a graph of fewer than 2^18
// potential nodes takes one thread.  A failed write is left in file.failed.
uint64_t host_graph_lines(const HostIndex &h, bool translated, PositionalFile &file);

}  // namespace gbwt_hip
