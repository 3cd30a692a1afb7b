// tags.hip -- gbz-extract's `tag-array` mode (src/bin/gbz-extract.rs:296-482): the graph position of every entry of a suffix array that an
// external tool built over the text `sequences` mode wrote.
//
// The text of paths p_0 .. p_{n-1} is the forward bases of p_0, one endmarker, the bases of p_1, one endmarker, ...  The tag of text position t
// (extract_path / encode_start, :346-371) is 0 for an endmarker and otherwise ((v << 11) | (o << 10)) + w for the base w bases (in reading
// direction, also on a reverse node) behind the first base of the visit of node v in orientation o that t falls into.  With the GBWT-encoded
// node 2 v + o of the walk that is (node << 10) + w.  It is a plain 64-bit ADDITION, as in the reference, which does not guard labels longer
// than 1 024 bases (its FIXME): there w carries into the orientation bit and the node id, and so it does here.  Nodes are nodes, never
// segments.  TAG[i] = tag(SA[i]): the reference gets there with two sorts of (index, value) pairs, which compute exactly this gather when
// the values read are a permutation of 0 .. expected_len - 1; for other input the reference's result is unspecified and ours is the gather.
// A value >= expected_len is reported (GBWT_HIP_INVALID_DATA) and never read through.
//
// PLAN (kept on the workspace while the list of path ids stays the same): the rows are the extraction of sequences 2 p (k_walk_direct); one
// pass gives every POSITION of the text's walk -- the nodes of a row and one pseudo-position of node 0 and length 1 behind it for its endmarker
// -- its node and its label length, a scan turns the lengths into text offsets, and a sampled top level holds for every 32nd text
// offset (1 << TAG_SHIFT) the position it falls into.  12 bytes per position + 4 (8 from 2^32 positions) per 32 text offsets.
//
// GATHER (k_tags): one suffix-array value in, one tag out.  The two hints around a value bound a search over at most 33 text
// offsets (every position with bases has at least one, so a window of 32 text offsets starts at most 32 of them) -- three cache lines for
// labels of one base, one for labels of tens of bases -- then the position's offset (a line the search has just touched) and its node.
// Every thread runs four lookups in lock step, so that four dependent chains are in flight per lane; the values are loaded coalesced, the
// tags leave with non-temporal stores.  A workgroup owns a contiguous range of tiles: the tag in front of a tile is the last tag of the tile
// before it, kept in LDS, so that the runs (TAG[i] != TAG[i - 1]) are counted in the same pass, with one extra lookup and one atomic per workgroup.
//
// The kernels and their launch wrappers (tags.hpp) stand here; the plan of a request, the batches and the C ABI are capi_tags.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "capi_status.hpp"
#include "device_common.hpp"
#include "tags.hpp"

using namespace gbwt_hip;

namespace {

constexpr uint32_t TAG_THREADS = 256, TAG_PER = 4, TAG_TILE = TAG_THREADS * TAG_PER;

// The position map of a plan as the kernels see it
template <class H> struct TagMap { const H *top; const uint64_t *off; const uint32_t *node; uint64_t text_len; };

// Node and label length of every position: position q of row k (the k with offsets[k] + k <= q <= offsets[k + 1] + k) is the walk's node
// offsets[k] + (q - offsets[k] - k), the last one of the row its endmarker.
__global__ void __launch_bounds__(256) k_tag_positions(const uint64_t *offsets, const uint32_t *nodes, uint64_t n, uint64_t positions, Labels L, uint32_t *pos_node,
                                                        uint64_t *pos_len) {
    const uint64_t q = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (q >= positions) return;
    uint64_t lo = 0, hi = n - 1;                     // the last row that starts at or before q
    while (lo < hi) { const uint64_t mid = lo + (hi - lo + 1) / 2; if (offsets[mid] + mid <= q) lo = mid; else hi = mid - 1; }
    const uint64_t j = q - lo;                       // index into the walk's nodes, or the end of the row
    if (j == offsets[lo + 1]) { pos_node[q] = 0; pos_len[q] = 1; return; }
    const uint32_t node = nodes[j];
    uint64_t a, b;
    label_of(L, node, a, b);
    pos_node[q] = node;
    pos_len[q] = b - a;
}

// Text offset of every row, and the text length behind the last
__global__ void __launch_bounds__(256) k_tag_rows(const uint64_t *offsets, uint64_t n, const uint64_t *pos_off, uint64_t positions, uint64_t *rows) {
    const uint64_t k = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (k > n) return;
    rows[k] = k < n ? pos_off[offsets[k] + k] : pos_off[positions];
}

// top[h] = the last position that starts at or before text offset h << TAG_SHIFT (the one that holds it: a position without bases never is the
// last one); top[hints - 1] = the last position, the bound of the searches in the last window.
template <class H>
__global__ void __launch_bounds__(256) k_tag_top(const uint64_t *pos_off, uint64_t positions, uint64_t hints, H *top) {
    const uint64_t h = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (h >= hints) return;
    if (h + 1 == hints) { top[h] = static_cast<H>(positions - 1); return; }
    top[h] = static_cast<H>(last_at_or_before(pos_off, positions, h << TAG_SHIFT));
}

// The tag of one text offset t < text_len (the lookup of the gather kernel, alone: the tag in front of a workgroup's first tile)
template <class H>
__device__ __forceinline__ uint64_t tag_of(const TagMap<H> &m, uint64_t t) {
    const uint64_t lo = last_at_or_before(m.off, m.top[t >> TAG_SHIFT], m.top[(t >> TAG_SHIFT) + 1], t);
    return (static_cast<uint64_t>(m.node[lo]) << 10) + (t - m.off[lo]);
}

// See the top of the file.  Entry base + 256 i + t of a tile is lookup i of thread t.  has_prev: a batch in front of this one has left its last
// tag in state->last[parity ^ 1]; without, entry 0 counts as the start of a run.
template <class H>
__global__ void __launch_bounds__(TAG_THREADS) k_tags(const uint64_t *__restrict__ sa, uint64_t count, TagMap<H> m, uint64_t *__restrict__ tags, TagState *state,
                                                       uint32_t has_prev, uint32_t parity) {
    __shared__ uint64_t tile[TAG_TILE + 1];          // tile[0]: the tag in front of the tile
    const uint32_t t = threadIdx.x;
    const uint64_t tiles = (count + TAG_TILE - 1) / TAG_TILE, share = (tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t first = blockIdx.x * share, end = first + share < tiles ? first + share : tiles;
    if (first >= end) return;
    uint32_t runs = 0, bad = 0;
    const bool opens = first == 0 && !has_prev;      // entry 0 has nothing in front of it
    if (t == 0) {
        uint64_t front = 0;
        if (first != 0) {
            const uint64_t v = sa[first * TAG_TILE - 1];
            if (v < m.text_len) front = tag_of(m, v);
        } else if (has_prev) front = state->last[parity ^ 1u];
        tile[0] = front;
    }
    for (uint64_t tl = first; tl < end; tl++) {
        const uint64_t base = tl * TAG_TILE;
        uint64_t v[TAG_PER], lo[TAG_PER], hi[TAG_PER];
        bool live[TAG_PER], ok[TAG_PER];
#pragma unroll
        for (uint32_t i = 0; i < TAG_PER; i++) {
            const uint64_t at = base + i * TAG_THREADS + t;
            live[i] = at < count;
            v[i] = live[i] ? __builtin_nontemporal_load(sa + at) : 0;
            ok[i] = v[i] < m.text_len;               // (text_len != 0: the host launches nothing for an empty text)
            if (!ok[i]) { bad = 1; v[i] = 0; }       // never read through: the lookup of such a lane is that of offset 0
        }
#pragma unroll
        for (uint32_t i = 0; i < TAG_PER; i++) { const uint64_t h = v[i] >> TAG_SHIFT; lo[i] = m.top[h]; hi[i] = m.top[h + 1]; }
        for (;;) {                                   // the four searches in lock step: every round loads for all of them
            bool more = false;
            uint64_t mid[TAG_PER], o[TAG_PER];
#pragma unroll
            for (uint32_t i = 0; i < TAG_PER; i++) { mid[i] = lo[i] + (hi[i] - lo[i] + 1) / 2; o[i] = m.off[mid[i]]; }
#pragma unroll
            for (uint32_t i = 0; i < TAG_PER; i++) {
                if (lo[i] < hi[i]) { if (o[i] <= v[i]) lo[i] = mid[i]; else hi[i] = mid[i] - 1; }
                more |= lo[i] < hi[i];
            }
            if (!more) break;
        }
        uint64_t o[TAG_PER], tag[TAG_PER];
        uint32_t node[TAG_PER];
#pragma unroll
        for (uint32_t i = 0; i < TAG_PER; i++) { o[i] = m.off[lo[i]]; node[i] = m.node[lo[i]]; }
#pragma unroll
        for (uint32_t i = 0; i < TAG_PER; i++) {
            tag[i] = ok[i] ? (static_cast<uint64_t>(node[i]) << 10) + (v[i] - o[i]) : 0;
            tile[1 + i * TAG_THREADS + t] = tag[i];
            if (live[i] && ok[i]) __builtin_nontemporal_store(tag[i], tags + base + i * TAG_THREADS + t);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < TAG_PER; i++) {
            const uint32_t at = i * TAG_THREADS + t;
            if (live[i]) runs += (opens && base + at == 0) || tag[i] != tile[at] ? 1u : 0u;
        }
        const uint64_t carry = tile[TAG_TILE];
        if (tl + 1 == tiles) {                       // the last entry of the batch leaves its tag for the next one
            const uint64_t last = count - 1 - base;
            if (t == last % TAG_THREADS) state->last[parity] = tile[1 + last];
        }
        __syncthreads();
        if (t == 0) tile[0] = carry;
    }
    for (int d = 32; d > 0; d >>= 1) { runs += __shfl_down(runs, d, 64); bad |= __shfl_down(bad, d, 64); }
    __shared__ uint32_t wave_runs[TAG_THREADS / 64], wave_bad[TAG_THREADS / 64];
    if (t % 64 == 0) { wave_runs[t / 64] = runs; wave_bad[t / 64] = bad; }
    __syncthreads();
    if (t == 0) {
        uint32_t r = 0, b = 0;
        for (uint32_t w = 0; w < TAG_THREADS / 64; w++) { r += wave_runs[w]; b |= wave_bad[w]; }
        if (r) atomicAdd(&state->runs, static_cast<unsigned long long>(r));
        if (b) atomicOr(&state->bad, 1u);
    }
}


}  // namespace

namespace gbwt_hip {

void launch_tag_positions(const uint64_t *d_offsets, const uint32_t *d_nodes, uint64_t n, uint64_t positions, const Labels &L, uint32_t *d_pos_node, uint64_t *d_pos_len,
                          hipStream_t s) {
    hipLaunchKernelGGL(k_tag_positions, blocks_for(positions), dim3(256), 0, s, d_offsets, d_nodes, n, positions, L, d_pos_node, d_pos_len);
}

void launch_tag_rows(const uint64_t *d_offsets, uint64_t n, const uint64_t *d_pos_off, uint64_t positions, uint64_t *d_rows, hipStream_t s) {
    hipLaunchKernelGGL(k_tag_rows, blocks_for(n + 1), dim3(256), 0, s, d_offsets, n, d_pos_off, positions, d_rows);
}

void launch_tag_top(const uint64_t *d_pos_off, uint64_t positions, uint64_t hints, void *d_top, bool wide, hipStream_t s) {
    if (wide) hipLaunchKernelGGL(k_tag_top<uint64_t>, blocks_for(hints), dim3(256), 0, s, d_pos_off, positions, hints, static_cast<uint64_t *>(d_top));
    else hipLaunchKernelGGL(k_tag_top<uint32_t>, blocks_for(hints), dim3(256), 0, s, d_pos_off, positions, hints, static_cast<uint32_t *>(d_top));
}

void launch_tags(int device, const TagTables &t, const uint64_t *d_sa, uint64_t count, uint64_t *d_tags, TagState *d_state, bool has_prev, uint32_t parity, hipStream_t s) {
    int cus = 0;
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    const uint64_t tiles = (count + TAG_TILE - 1) / TAG_TILE;
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(tiles, 8ull * static_cast<unsigned>(std::max(cus, 1))));   // eight workgroups per CU: what its registers hold
    if (t.wide) {
        const TagMap<uint64_t> m{static_cast<const uint64_t *>(t.top), t.off, t.node, t.text_len};
        hipLaunchKernelGGL(k_tags<uint64_t>, dim3(grid), dim3(TAG_THREADS), 0, s, d_sa, count, m, d_tags, d_state, has_prev ? 1u : 0u, parity);
    } else {
        const TagMap<uint32_t> m{static_cast<const uint32_t *>(t.top), t.off, t.node, t.text_len};
        hipLaunchKernelGGL(k_tags<uint32_t>, dim3(grid), dim3(TAG_THREADS), 0, s, d_sa, count, m, d_tags, d_state, has_prev ? 1u : 0u, parity);
    }
    HIP_CHECK(hipGetLastError());
}

}  // namespace gbwt_hip
