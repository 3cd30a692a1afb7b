// topology.hip -- the graph of a handle as batched device calls: node ids (GBZ::node_iter, src/gbz.rs:312-317), edge rows (GBZ::successors /
// predecessors, src/gbz.rs:327-353, EdgeIter 819-870), link rows (GBZ::segment_successors / _predecessors, src/gbz.rs:402-440, LinkIter
// 988-1005) and the S- and L-lines of a GFA file (write_segments / write_links, src/bin/gbunzip.rs:230-317), all from what a handle keeps
// in HBM: the record byte stream and the dense record starts, the node-to-segment tables of a GBZ, the node labels.
//
// EDGE ROWS: count, scan, fill.  The count of a row is its outdegree, less one for a leading ENDMARKER edge (EdgeIter::new): two varints
// of the record header, whatever the outdegree.  The fill decodes the header -- a serial chain of varints -- and writes the nodes: the lane
// of the query for rows of at most EDGE_LANE_MAX edges; a longer row goes onto a list, and a workgroup per list entry stages stretches of
// the decoded nodes in LDS (one lane decodes) and writes them with all its lanes.
//
// LINK ROWS are edge rows of boundary nodes with a mapping step, one lane per EDGE: the first node without a segment cuts its row
// (atomicMin per row), the scan of the cuts gives the link offsets, every edge in front of the cut writes its segment.
//
// TEXT.  S-lines: the output is split by BYTES -- a workgroup per TEXT_STRETCH bytes, a lane per aligned 16 of them; the lane finds the line
// of its first byte by a search over the line offsets and produces its bytes; sixteen bytes inside one label are two unaligned loads and one
// 16-byte store, so a label of 70 000 bases is copied by 4 400 lanes and a line of six bytes costs its lane six.  L-lines: one lane per
// edge of the kept rows writes its line (two names and ten bytes).
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "lf_device.hpp"
#include "topology.hpp"

namespace gbwt_hip {

namespace {


constexpr uint32_t BIG_STAGE = 1024;          // nodes staged in LDS per round of k_edge_fill_big (8 KiB)
constexpr uint32_t NO_SEGMENT = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t digits_of(uint64_t v) {
    uint32_t d = 1;
    while (v >= 10) { v /= 10; d++; }
    return d;
}

// digit `k` from the left of the `digits`-digit number v
__device__ __forceinline__ uint8_t digit_at(uint64_t v, uint32_t digits, uint32_t k) {
    for (uint32_t j = k + 1; j < digits; j++) v /= 10;
    return static_cast<uint8_t>('0' + v % 10);
}

__global__ void __launch_bounds__(256) k_node_flags(DeviceIndex ix, ComponentGeometry g, uint64_t *flags) {
    const uint64_t s = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (s >= g.slots) return;
    const uint64_t forward = 2 * (g.min_node + s);
    flags[s] = forward >= ix.first_node && record_is_real(ix, forward - ix.alphabet_offset) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_segment_flags(GraphTables t, uint64_t *flags) {
    const uint64_t s = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (s >= t.segments) return;
    const uint64_t first = t.seg_start[s];
    flags[s] = first < t.mapping_len && first < t.seg_start[s + 1] && t.node_real[first] ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_scatter_ids(const uint64_t *rank, uint64_t n, uint64_t base, uint64_t *out) {
    const uint64_t s = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (s < n && rank[s + 1] > rank[s]) out[rank[s]] = base + s;
}

__global__ void __launch_bounds__(256) k_all_node_queries(ComponentGeometry g, uint64_t *ids, uint8_t *orient) {
    const uint64_t q = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (q >= 2 * g.slots) return;
    ids[q] = g.min_node + (q >> 1);
    orient[q] = static_cast<uint8_t>(q & 1);
}

__global__ void __launch_bounds__(256) k_link_queries(GraphTables t, const uint64_t *seg_ids, const uint8_t *orient, uint64_t n, uint32_t predecessors, uint64_t *out_ids,
                                                       uint8_t *out_orient) {
    const uint64_t q = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (q >= n) return;
    const uint64_t seg = seg_ids ? seg_ids[q] : q >> 1;
    const uint32_t o = seg_ids ? (orient[q] & 1u) : static_cast<uint32_t>(q & 1);
    uint64_t node = 0;
    if (seg < t.segments) {
        const uint64_t start = t.seg_start[seg], end = t.seg_start[seg + 1];
        if (start < end && end <= t.mapping_len && (seg_ids || t.node_real[start])) node = (o == 0) != (predecessors != 0) ? end - 1 : start;
    }
    out_ids[q] = node;
    out_orient[q] = static_cast<uint8_t>(o);
}

// Opens the row of (id, o): the record of GBWT node 2 id + o, for a node that exists.  false where GBZ::successors returns None:
// !has_node(id), or no record / an empty record / outdegree 0 (BWT::record, Record::new, src/bwt.rs:124-131, 341-351).  A header that
// cannot hold its outdegree -- every edge takes two bytes at least -- is refused as well: nothing is sized from a number the bytes
// cannot back.  On success the cursor stands behind the outdegree.
__device__ __forceinline__ bool open_edge_row(const DeviceIndex &ix, uint64_t id, uint32_t o, ByteCursor &c, uint64_t &sigma) {
    if (id == 0 || id >= (uint64_t(1) << 62)) return false;
    const uint64_t forward = 2 * id;
    if (forward < ix.first_node || !record_is_real(ix, forward - ix.alphabet_offset)) return false;
    const uint64_t rec = forward + o - ix.alphabet_offset;
    if (rec >= ix.n_records) return false;
    uint64_t start, limit;
    record_bounds(ix, rec, start, limit);
    if (start >= limit || limit > ix.data_len) return false;
    c = ByteCursor(ix.data, start, limit);
    if (!c.varint(sigma) || sigma == 0) return false;
    return sigma <= (limit - c.pos) / 2;
}

__global__ void __launch_bounds__(256) k_edge_count(DeviceIndex ix, const uint64_t *ids, const uint8_t *orient, uint64_t n, uint32_t flip, uint64_t *counts, uint8_t *valid) {
    const uint64_t q = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (q >= n) return;
    ByteCursor c(ix.data, 0, 0);
    uint64_t sigma = 0, count = 0;
    const bool ok = open_edge_row(ix, ids[q], (orient[q] & 1u) ^ flip, c, sigma);
    if (ok) {
        uint64_t first = 1;
        count = sigma;
        if (c.varint(first) && first == 0) count--;            // the ENDMARKER edge (EdgeIter::new)
    }
    counts[q] = count;
    valid[q] = ok ? 1 : 0;
}

// Decodes up to `room` nodes of a header from `e` on (the cursor stands in front of edge e; node = the node of edge e - 1); the ENDMARKER
// edge -- edge 0 with node 0 -- is left out.  Returns the nodes written; e == sigma afterwards unless `room` ran out.  A header that ends
// inside the record's bytes sets e = sigma: the caller zero-fills what is left of the row.
template <class Put>
__device__ __forceinline__ uint32_t decode_edges(ByteCursor &c, uint64_t sigma, uint64_t &e, uint64_t &node, uint32_t room, Put put) {
    uint32_t written = 0;
    while (e < sigma && written < room) {
        uint64_t delta, offset;
        if (!c.varint(delta) || !c.varint(offset)) { e = sigma; break; }
        node += delta;
        if (!(e == 0 && node == 0)) put(written++, node);
        e++;
    }
    return written;
}

__global__ void __launch_bounds__(256) k_edge_fill(DeviceIndex ix, const uint64_t *ids, const uint8_t *orient, uint64_t n, uint32_t flip, const uint64_t *offsets, uint64_t *edges,
                                                    uint32_t *rows, uint32_t *big) {
    const uint64_t q = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (q >= n) return;
    const uint64_t begin = offsets[q], end = offsets[q + 1];
    if (end <= begin) return;
    if (end - begin > EDGE_LANE_MAX) { big[1 + atomicAdd(&big[0], 1u)] = static_cast<uint32_t>(q); return; }
    ByteCursor c(ix.data, 0, 0);
    uint64_t sigma = 0, e = 0, node = 0;
    uint64_t out = begin;
    if (open_edge_row(ix, ids[q], (orient[q] & 1u) ^ flip, c, sigma))
        out += decode_edges(c, sigma, e, node, static_cast<uint32_t>(end - begin), [&](uint32_t k, uint64_t v) {
            edges[begin + k] = v ^ flip;
            if (rows) rows[begin + k] = static_cast<uint32_t>(q);
        });
    for (; out < end; out++) { edges[out] = 0; if (rows) rows[out] = static_cast<uint32_t>(q); }
}

// A workgroup per long row: lane 0 decodes BIG_STAGE nodes into LDS, all lanes write them, until the row is full.
__global__ void __launch_bounds__(256) k_edge_fill_big(DeviceIndex ix, const uint64_t *ids, const uint8_t *orient, uint32_t flip, const uint64_t *offsets, uint64_t *edges,
                                                        uint32_t *rows, const uint32_t *big) {
    __shared__ uint64_t stage[BIG_STAGE];
    __shared__ uint32_t staged;
    const uint32_t listed = big[0];
    for (uint32_t b = blockIdx.x; b < listed; b += gridDim.x) {
        const uint64_t q = big[1 + b];
        const uint64_t end = offsets[q + 1];
        uint64_t out = offsets[q];
        ByteCursor c(ix.data, 0, 0);
        uint64_t sigma = 0, e = 0, node = 0;
        if (threadIdx.x == 0 && !open_edge_row(ix, ids[q], (orient[q] & 1u) ^ flip, c, sigma)) sigma = 0;
        while (out < end) {
            if (threadIdx.x == 0) {
                const uint64_t room = end - out;
                staged = decode_edges(c, sigma, e, node, static_cast<uint32_t>(room < BIG_STAGE ? room : BIG_STAGE), [&](uint32_t k, uint64_t v) { stage[k] = v; });
            }
            __syncthreads();
            const uint32_t have = staged;
            for (uint32_t k = threadIdx.x; k < have; k += blockDim.x) {
                edges[out + k] = stage[k] ^ flip;
                if (rows) rows[out + k] = static_cast<uint32_t>(q);
            }
            __syncthreads();
            if (have == 0) break;                              // (the header ended early: the rest of the row is zero-filled)
            out += have;
        }
        for (uint64_t k = out + threadIdx.x; k < end; k += blockDim.x) { edges[k] = 0; if (rows) rows[k] = static_cast<uint32_t>(q); }
        __syncthreads();
    }
}

// the segment of GBZ::node_to_segment(id) (src/gbz.rs:370-376), NO_SEGMENT for None
__device__ __forceinline__ uint32_t segment_of(const GraphTables &t, uint64_t id) {
    if (id >= t.mapping_len || !t.node_real[id]) return NO_SEGMENT;
    return t.seg_of[id];
}

__global__ void __launch_bounds__(256) k_row_lengths(const uint64_t *offsets, uint64_t n, uint64_t *cut) {
    const uint64_t r = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (r < n) cut[r] = offsets[r + 1] - offsets[r];
}

__global__ void __launch_bounds__(256) k_link_cut(GraphTables t, const uint64_t *offsets, const uint64_t *edges, const uint32_t *rows, uint64_t total, unsigned long long *cut) {
    const uint64_t e = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (e >= total) return;
    if (segment_of(t, edges[e] >> 1) == NO_SEGMENT) atomicMin(&cut[rows[e]], static_cast<unsigned long long>(e - offsets[rows[e]]));
}

__global__ void __launch_bounds__(256) k_link_write(GraphTables t, const uint64_t *offsets, const uint64_t *edges, const uint32_t *rows, uint64_t total, const uint64_t *cut,
                                                     const uint64_t *link_offsets, uint64_t *links) {
    const uint64_t e = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (e >= total) return;
    const uint32_t r = rows[e];
    const uint64_t k = e - offsets[r];
    if (k >= cut[r]) return;
    links[link_offsets[r] + k] = 2 * static_cast<uint64_t>(segment_of(t, edges[e] >> 1)) + (edges[e] & 1);
}

// ---- S-lines ----------------------------------------------------------------------------------------------------------------------------------

// What the S-line of an item is made of: "S\t" name "\t" label "\n"
struct SegmentLine {
    uint64_t id, label_len;
    const uint8_t *name;           // null: the decimal digits of id
    const uint8_t *label;
    uint32_t name_len;
};

__device__ __forceinline__ SegmentLine segment_line(const GraphTables &t, uint64_t id, bool translated) {
    SegmentLine l{id, 0, nullptr, nullptr, 0};
    if (translated) {
        const uint64_t a = t.name_off[id];
        l.name = t.names + a;
        l.name_len = static_cast<uint32_t>(t.name_off[id + 1] - a);
        const uint64_t slot = static_cast<uint64_t>(t.seg_start[id]) - 1;      // Segment::sequence: the labels of its nodes, back to back (src/graph.rs:172-184)
        if (slot < t.labels) { l.label = t.label_bytes + t.label_off[slot]; l.label_len = t.seq_len[id]; }
    } else {
        l.name_len = digits_of(id);
        const uint64_t forward = 2 * id;
        const uint64_t slot = forward >= t.first_node ? (forward - t.first_node) / 2 : t.labels;
        if (slot < t.labels) { l.label = t.label_bytes + t.label_off[slot]; l.label_len = t.label_off[slot + 1] - t.label_off[slot]; }
    }
    return l;
}

__global__ void __launch_bounds__(256) k_segment_line_sizes(GraphTables t, const uint64_t *items, uint64_t n, uint32_t translated, uint64_t *sizes) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= n) return;
    const SegmentLine l = segment_line(t, items[i], translated != 0);
    sizes[i] = 4 + static_cast<uint64_t>(l.name_len) + l.label_len;
}

// the last i in [lo, hi) with off[i] <= p (off[lo] <= p)
__device__ __forceinline__ uint64_t line_at(const uint64_t *off, uint64_t lo, uint64_t hi, uint64_t p) {
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// `base` = where the S-lines start in the text; lane units are the aligned 16 bytes of the text buffer
__global__ void __launch_bounds__(256) k_segment_lines(GraphTables t, const uint64_t *items, uint64_t n, uint32_t translated, const uint64_t *line_off, uint64_t base, uint64_t bytes,
                                                        char *text) {
    __shared__ uint64_t first_line;
    const uint64_t group = (base & ~uint64_t(15)) + static_cast<uint64_t>(blockIdx.x) * TEXT_STRETCH;      // absolute, 16-byte aligned
    if (threadIdx.x == 0) first_line = line_at(line_off, 0, n, group > base ? group - base : 0);
    __syncthreads();
    const uint64_t unit = group + 16 * threadIdx.x;
    const uint64_t lo = unit > base ? unit : base, hi = unit + 16 < base + bytes ? unit + 16 : base + bytes;
    if (lo >= hi) return;
    // every line has four bytes at least: the lines of a stretch are among the TEXT_STRETCH / 4 + 1 behind its first
    const uint64_t last = first_line + TEXT_STRETCH / 4 + 2 < n ? first_line + TEXT_STRETCH / 4 + 2 : n;
    uint64_t i = line_at(line_off, first_line, last, lo - base);
    uint64_t begin = line_off[i], end = line_off[i + 1];
    SegmentLine l = segment_line(t, items[i], translated != 0);
    uint64_t p = lo - base;                                   // position in the S-lines
    if (hi - lo == 16) {
        const uint64_t label_at = begin + 3 + l.name_len;
        if (p >= label_at && p + 16 < end) {                  // sixteen bytes of one label
            const uint8_t *src = l.label + (p - label_at);
            ulonglong2 v;
            v.x = load_u64_unaligned(src); v.y = load_u64_unaligned(src + 8);
            *reinterpret_cast<ulonglong2 *>(text + unit) = v;
            return;
        }
    }
    uint64_t word[2] = {0, 0};
    for (uint64_t at = lo; at < hi; at++, p++) {
        while (p >= end) {
            i++;
            begin = end; end = line_off[i + 1];
            l = segment_line(t, items[i], translated != 0);
        }
        const uint64_t rel = p - begin;
        uint8_t byte;
        if (rel == 0) byte = 'S';
        else if (rel == 1 || rel == 2 + l.name_len) byte = '\t';
        else if (rel < 2 + l.name_len) byte = l.name ? l.name[rel - 2] : digit_at(l.id, l.name_len, static_cast<uint32_t>(rel - 2));
        else if (p + 1 == end) byte = '\n';
        else byte = l.label[rel - 3 - l.name_len];
        if (hi - lo == 16) word[(at - lo) >> 3] |= static_cast<uint64_t>(byte) << (8 * ((at - lo) & 7));
        else text[at] = static_cast<char>(byte);
    }
    if (hi - lo == 16) {
        ulonglong2 v;
        v.x = word[0]; v.y = word[1];
        *reinterpret_cast<ulonglong2 *>(text + unit) = v;
    }
}

// ---- L-lines ----------------------------------------------------------------------------------------------------------------------------------

// from / to of edge e of the rows of all (node | segment, orientation) queries; false: no line (behind the cut, or not canonical)
struct LinkLine { uint64_t from, to; uint32_t from_rev, to_rev; };

__device__ __forceinline__ bool link_line(const GraphTables &t, const ComponentGeometry &g, bool translated, uint32_t row, uint64_t edge, LinkLine &l) {
    l.from_rev = row & 1u;
    l.to_rev = static_cast<uint32_t>(edge & 1);
    if (translated) {
        l.from = row >> 1;
        const uint32_t to = segment_of(t, edge >> 1);
        if (to == NO_SEGMENT) return false;
        l.to = to;
    } else {
        l.from = g.min_node + (row >> 1);
        l.to = edge >> 1;
    }
    // write_links (src/bin/gbunzip.rs:271-317): from a forward node to >= its id; from a reverse node to > its id, or to the same id forward
    return l.from_rev ? (l.to > l.from || (l.to == l.from && !l.to_rev)) : l.to >= l.from;
}

__device__ __forceinline__ uint32_t name_length(const GraphTables &t, bool translated, uint64_t id) {
    return translated ? static_cast<uint32_t>(t.name_off[id + 1] - t.name_off[id]) : digits_of(id);
}

__device__ __forceinline__ char *put_name(const GraphTables &t, bool translated, uint64_t id, char *out) {
    if (translated) {
        const uint64_t a = t.name_off[id], b = t.name_off[id + 1];
        for (uint64_t k = a; k < b; k++) *out++ = static_cast<char>(t.names[k]);
        return out;
    }
    const uint32_t digits = digits_of(id);
    for (uint32_t k = digits; k > 0; k--) { out[k - 1] = static_cast<char>('0' + id % 10); id /= 10; }
    return out + digits;
}

__global__ void __launch_bounds__(256) k_link_line_sizes(GraphTables t, ComponentGeometry g, uint32_t translated, const uint64_t *offsets, const uint64_t *edges, const uint32_t *rows,
                                                          uint64_t total, const uint64_t *cut, uint64_t *sizes, unsigned long long *lines) {
    const uint64_t e = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (e >= total) return;
    const uint32_t r = rows[e];
    uint64_t size = 0;
    LinkLine l;
    if ((!cut || e - offsets[r] < cut[r]) && link_line(t, g, translated != 0, r, edges[e], l))
        size = 10 + static_cast<uint64_t>(name_length(t, translated != 0, l.from)) + name_length(t, translated != 0, l.to);
    sizes[e] = size;
    if (size != 0) atomicAdd(lines, 1ull);                      // (the compiler makes one add per wave of these)
}

__global__ void __launch_bounds__(256) k_link_lines(GraphTables t, ComponentGeometry g, uint32_t translated, const uint64_t *edges, const uint32_t *rows, uint64_t total,
                                                     const uint64_t *line_off, uint64_t base, char *text) {
    const uint64_t e = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (e >= total || line_off[e + 1] == line_off[e]) return;
    LinkLine l;
    (void)link_line(t, g, translated != 0, rows[e], edges[e], l);
    char *out = text + base + line_off[e];
    *out++ = 'L'; *out++ = '\t';
    out = put_name(t, translated != 0, l.from, out);
    *out++ = '\t'; *out++ = l.from_rev ? '-' : '+'; *out++ = '\t';
    out = put_name(t, translated != 0, l.to, out);
    *out++ = '\t'; *out++ = l.to_rev ? '-' : '+'; *out++ = '\t'; *out++ = '*'; *out++ = '\n';
}

}  // namespace

void launch_node_flags(const DeviceIndex &ix, const ComponentGeometry &g, uint64_t *d_flags, hipStream_t s) {
    if (g.slots) hipLaunchKernelGGL(k_node_flags, dim3(blocks_for(g.slots)), dim3(256), 0, s, ix, g, d_flags);
}

void launch_segment_flags(const GraphTables &t, uint64_t *d_flags, hipStream_t s) {
    if (t.segments) hipLaunchKernelGGL(k_segment_flags, dim3(blocks_for(t.segments)), dim3(256), 0, s, t, d_flags);
}

void launch_scatter_ids(const uint64_t *d_rank, uint64_t n, uint64_t base, uint64_t *d_out, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_scatter_ids, dim3(blocks_for(n)), dim3(256), 0, s, d_rank, n, base, d_out);
}

void launch_all_node_queries(const ComponentGeometry &g, uint64_t *d_ids, uint8_t *d_orient, hipStream_t s) {
    if (g.slots) hipLaunchKernelGGL(k_all_node_queries, dim3(blocks_for(2 * g.slots)), dim3(256), 0, s, g, d_ids, d_orient);
}

void launch_link_queries(const GraphTables &t, const uint64_t *d_seg_ids, const uint8_t *d_orient, uint64_t n, bool predecessors, uint64_t *d_out_ids, uint8_t *d_out_orient,
                         hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_link_queries, dim3(blocks_for(n)), dim3(256), 0, s, t, d_seg_ids, d_orient, n, predecessors ? 1u : 0u, d_out_ids, d_out_orient);
}

void launch_edge_count(const DeviceIndex &ix, const uint64_t *d_ids, const uint8_t *d_orient, uint64_t n, bool flip, uint64_t *d_counts, uint8_t *d_valid, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_edge_count, dim3(blocks_for(n)), dim3(256), 0, s, ix, d_ids, d_orient, n, flip ? 1u : 0u, d_counts, d_valid);
}

void launch_edge_fill(const DeviceIndex &ix, const uint64_t *d_ids, const uint8_t *d_orient, uint64_t n, bool flip, const uint64_t *d_offsets, uint64_t *d_edges, uint32_t *d_rows,
                      uint32_t *d_big, hipStream_t s) {
    if (n == 0) return;
    (void)hipMemsetAsync(d_big, 0, sizeof(uint32_t), s);
    hipLaunchKernelGGL(k_edge_fill, dim3(blocks_for(n)), dim3(256), 0, s, ix, d_ids, d_orient, n, flip ? 1u : 0u, d_offsets, d_edges, d_rows, d_big);
    hipLaunchKernelGGL(k_edge_fill_big, dim3(EDGE_BIG_BLOCKS), dim3(256), 0, s, ix, d_ids, d_orient, flip ? 1u : 0u, d_offsets, d_edges, d_rows, d_big);
}

void launch_link_cut(const GraphTables &t, const uint64_t *d_offsets, const uint64_t *d_edges, const uint32_t *d_rows, uint64_t n, uint64_t total, uint64_t *d_cut, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_row_lengths, dim3(blocks_for(n)), dim3(256), 0, s, d_offsets, n, d_cut);
    if (total) hipLaunchKernelGGL(k_link_cut, dim3(blocks_for(total)), dim3(256), 0, s, t, d_offsets, d_edges, d_rows, total, reinterpret_cast<unsigned long long *>(d_cut));
}

void launch_link_write(const GraphTables &t, const uint64_t *d_offsets, const uint64_t *d_edges, const uint32_t *d_rows, uint64_t total, const uint64_t *d_cut,
                       const uint64_t *d_link_offsets, uint64_t *d_links, hipStream_t s) {
    if (total) hipLaunchKernelGGL(k_link_write, dim3(blocks_for(total)), dim3(256), 0, s, t, d_offsets, d_edges, d_rows, total, d_cut, d_link_offsets, d_links);
}

void launch_segment_line_sizes(const GraphTables &t, const uint64_t *d_items, uint64_t items, bool translated, uint64_t *d_sizes, hipStream_t s) {
    if (items) hipLaunchKernelGGL(k_segment_line_sizes, dim3(blocks_for(items)), dim3(256), 0, s, t, d_items, items, translated ? 1u : 0u, d_sizes);
}

void launch_segment_lines(const GraphTables &t, const uint64_t *d_items, uint64_t items, bool translated, const uint64_t *d_line_off, uint64_t base, uint64_t bytes, char *d_text,
                          hipStream_t s) {
    if (items == 0 || bytes == 0) return;
    const uint64_t first = base & ~uint64_t(15), groups = (base + bytes - first + TEXT_STRETCH - 1) / TEXT_STRETCH;
    hipLaunchKernelGGL(k_segment_lines, dim3(static_cast<unsigned>(groups)), dim3(256), 0, s, t, d_items, items, translated ? 1u : 0u, d_line_off, base, bytes, d_text);
}

void launch_link_line_sizes(const GraphTables &t, const ComponentGeometry &g, bool translated, const uint64_t *d_offsets, const uint64_t *d_edges, const uint32_t *d_rows,
                            uint64_t total, const uint64_t *d_cut, uint64_t *d_sizes, uint64_t *d_lines, hipStream_t s) {
    if (total) hipLaunchKernelGGL(k_link_line_sizes, dim3(blocks_for(total)), dim3(256), 0, s, t, g, translated ? 1u : 0u, d_offsets, d_edges, d_rows, total, d_cut, d_sizes,
                                  reinterpret_cast<unsigned long long *>(d_lines));
}

void launch_link_lines(const GraphTables &t, const ComponentGeometry &g, bool translated, const uint64_t *d_edges, const uint32_t *d_rows, uint64_t total,
                       const uint64_t *d_line_off, uint64_t base, char *d_text, hipStream_t s) {
    if (total) hipLaunchKernelGGL(k_link_lines, dim3(blocks_for(total)), dim3(256), 0, s, t, g, translated ? 1u : 0u, d_edges, d_rows, total, d_line_off, base, d_text);
}

}  // namespace gbwt_hip
