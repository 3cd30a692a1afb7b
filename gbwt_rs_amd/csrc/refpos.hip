// refpos.hip -- GBZ::reference_positions (src/gbz.rs:600-657) for any list of forward paths: about every `interval` bases of a path the
// pair (base offset of a node start, GBWT position Pos{node, offset} of that visit), and the length of the path in bases.
//
// The reference walks a path with start + forward, adds sequence_len per step and keeps a visit when its base offset has reached `next`
// (= the offset of the visit kept before + interval): a chain that is serial in the path.  Here, for the rows of sequences 2 p that
// k_walk_direct has extracted (POSITION i = node i of the rows laid end to end; P of them, P <= 2^32 - 1):
//   k_refpos_lengths  label length of every position; a scan gives off (u64, bases in front of a position, over all rows)
//   k_refpos_succ     succ(i) = the first k > i of the row with off_k >= off_i + interval (saturating), by binary search: off is strictly
//                     increasing inside a row (a node has at least one base).  No such k: the sentinel P, which maps to itself.
//   k_refpos_round    POINTER DOUBLING.  mark[first position of every row] = 1; in round t every marked i marks J_t[i], and J_{t+1} = J_t o J_t
//                     (J_0 = succ; one jump array in ping-pong).  After round t at least the chain elements of rank < 2^(t+1) are marked, and nothing
//                     but chain elements: a mark is only ever set on one (J_t[i] = succ^(2^t)(i)), so a lane that sees a mark set in its own round
//                     only runs ahead.
//                     A round that sets no new mark leaves the marked set closed under succ^(2^t), and it holds the ranks < 2^t: it is the whole
//                     chain.  Such a round leaves its flag word 0 and every later round returns at once: ceil(log2 P) launches are queued, no
//                     host wait in between.
//   a scan of the marks gives every kept position its SLOT and every row its first slot and count; the host waits once for the total.
//   k_refpos_walk     the LF walk that carries the in-record offset: one lane per sample segment of every row (device_index.hpp:
//                     row_segments), from the segment's {record, offset}; segment 0 from the endmarker entry.  A lane writes
//                     {off, node, offset} of every marked position of its segment to its slot, stops behind the last one, and takes no step
//                     when its segment holds no mark.  The node of every step is compared with the row's: a mismatch (a wrong segment
//                     start) raises a flag.
// Scratch per position: off 8 + lengths, then marks 8 + the two jump arrays, then slots 8 = 24 bytes.
#include <hip/hip_runtime.h>

#include "refpos.hpp"

#include "device_common.hpp"
#include "lf_device.hpp"
#include "pos_step.hpp"

namespace gbwt_hip {

namespace {

__global__ void __launch_bounds__(256) k_refpos_lengths(const uint32_t *__restrict__ nodes, uint64_t positions, Labels L, uint64_t *__restrict__ len) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i >= positions) return;
    uint64_t a, b;
    label_of(L, nodes[i], a, b);
    len[i] = b - a;
}

__global__ void __launch_bounds__(256) k_refpos_succ(RefposRows rows, const uint64_t *__restrict__ off, uint64_t interval, uint32_t *__restrict__ jump) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x, P = rows.positions;
    if (i > P) return;
    if (i == P) { jump[P] = static_cast<uint32_t>(P); return; }
    // the row of position i: the last one that starts at or before i (rows without nodes in front of it start where it does)
    const uint64_t r = last_at_or_before(rows.offsets, rows.n, i), end = rows.offsets[r + 1], base = off[rows.offsets[r]];
    const uint64_t here = off[i] - base;
    const uint64_t target = here + interval < here ? ~uint64_t(0) : here + interval;
    uint64_t lo = i + 1, hi = end;                   // the first k in [i + 1, end) with off_k >= target, or end
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (off[mid] - base >= target) hi = mid; else lo = mid + 1; }
    jump[i] = static_cast<uint32_t>(lo < end ? lo : P);
}

__global__ void __launch_bounds__(256) k_refpos_first_marks(RefposRows rows, uint64_t *mark) {
    const uint64_t r = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (r < rows.n && rows.offsets[r + 1] > rows.offsets[r]) mark[rows.offsets[r]] = 1;
}

__global__ void __launch_bounds__(256) k_refpos_round(uint64_t *mark, const uint32_t *__restrict__ jump, uint32_t *__restrict__ next, uint64_t positions, uint32_t *flags,
                                                       uint32_t t) {
    if (t != 0 && flags[t - 1] == 0) return;         // (the whole grid: the round in front is complete)
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    bool fresh = false;
    if (i <= positions) {
        const uint32_t j = jump[i];
        next[i] = jump[j];
        if (i < positions && j != positions && mark[i] != 0 && mark[j] == 0) { mark[j] = 1; fresh = true; }
    }
    if (__ballot(fresh) != 0 && (threadIdx.x & (WAVE - 1)) == 0) atomicOr(flags + t, 1u);
}

__global__ void __launch_bounds__(256) k_refpos_paths(RefposRows rows, const uint64_t *ids, const uint64_t *off, const uint64_t *slot, gbwt_hip_reference_path *out) {
    const uint64_t r = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (r >= rows.n) return;
    const uint64_t a = rows.offsets[r], b = rows.offsets[r + 1];
    out[r] = gbwt_hip_reference_path{ids[r], off[b] - off[a], slot[a], slot[b] - slot[a]};
}

template <bool FAST>
__global__ void __launch_bounds__(256) k_refpos_walk(DeviceIndex ix, RefposRows rows, RefposWalk w) {
    const uint64_t t = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (t >= w.walkers) return;
    const uint64_t r = last_at_or_before(w.seg_first, rows.n, t), j = t - w.seg_first[r], id = w.seq_ids[r];
    const uint64_t a = rows.offsets[r], len = rows.offsets[r + 1] - a;
    if (len == 0) return;
    // nodes [from, to) of the row are this lane's; Pos of node `from` = the endmarker entry (segment 0), or one step from the sample's state,
    // which is the position of the node in front of the segment (sample 0 is the state after the start node: segment 0 does not use it).
    // A lane that finds no such stretch where the host counted one for it -- no such sequence, no such segment, samples out of order --
    // says so: the marks of that stretch would stay unwritten.  (A last sample AT the end of the row is an empty stretch, not an error.)
    uint64_t from = 0, to = len, node = 0, offset = 0;
    bool ok = id < ix.n_sequences && id < ix.n_endmarker, step = false;
    if (ok && w.segmented) {
        const RowSegments rs = row_segments(ix, id);
        ok = j < rs.count;
        if (ok) {
            from = segment_position(ix, rs, id, j);
            if (j + 1 < rs.count) to = segment_position(ix, rs, id, j + 1);
            ok = from <= to && to <= len;
            if (j != 0) { const uint4 s = ix.samples[rs.base + j * rs.stride]; node = static_cast<uint64_t>(s.x) + ix.alphabet_offset; offset = s.y; step = true; }
        }
    } else ok = ok && j == 0;
    if (!ok) { atomicOr(w.flags + REFPOS_FLAG_MISMATCH, 1u); return; }
    if (from == to) return;
    // (the row's own pointers, one per lane: the loop keeps no base pointers of the request in scalar registers next to those of the index)
    const uint32_t *row_nodes = rows.nodes + a;
    const uint64_t *row_slot = w.slot + a, *row_off = w.off + a;
    const uint64_t last = row_slot[to], first_off = row_off[0];
    uint64_t slot = row_slot[from];
    if (slot == last) return;                        // no kept position in this segment: no step is taken
    if (j == 0) { const uint2 e = ix.endmarker[id]; node = e.x; offset = e.y; }
    for (uint64_t k = from;;) {                      // (one place where the step is taken: one copy of its code and of what it keeps in registers)
        if (step && !pos_step<FAST>(ix, node, offset)) { ok = false; break; }
        if (node != row_nodes[k]) { ok = false; break; }
        const uint64_t behind = row_slot[k + 1];
        if (behind != slot) w.out[slot] = gbwt_hip_reference_position{row_off[k] - first_off, gbwt_hip_pos{node, offset}};
        slot = behind;
        if (slot == last || ++k == to) break;
        step = true;
    }
    if (!ok) atomicOr(w.flags + REFPOS_FLAG_MISMATCH, 1u);
}


}  // namespace

void launch_refpos_lengths(const RefposRows &rows, const Labels &L, uint64_t *d_len, hipStream_t s) {
    if (rows.positions) hipLaunchKernelGGL(k_refpos_lengths, blocks_for(rows.positions), dim3(256), 0, s, rows.nodes, rows.positions, L, d_len);
}

void launch_refpos_succ(const RefposRows &rows, const uint64_t *d_off, uint64_t interval, uint32_t *d_jump, hipStream_t s) {
    hipLaunchKernelGGL(k_refpos_succ, blocks_for(rows.positions + 1), dim3(256), 0, s, rows, d_off, interval, d_jump);
}

void launch_refpos_first_marks(const RefposRows &rows, uint64_t *d_mark, hipStream_t s) {
    if (rows.n) hipLaunchKernelGGL(k_refpos_first_marks, blocks_for(rows.n), dim3(256), 0, s, rows, d_mark);
}

void launch_refpos_round(uint64_t *d_mark, const uint32_t *d_jump, uint32_t *d_next, uint64_t positions, uint32_t *d_flags, uint32_t t, hipStream_t s) {
    hipLaunchKernelGGL(k_refpos_round, blocks_for(positions + 1), dim3(256), 0, s, d_mark, d_jump, d_next, positions, d_flags, t);
}

void launch_refpos_paths(const RefposRows &rows, const uint64_t *d_ids, const uint64_t *d_off, const uint64_t *d_slot, gbwt_hip_reference_path *d_out, hipStream_t s) {
    if (rows.n) hipLaunchKernelGGL(k_refpos_paths, blocks_for(rows.n), dim3(256), 0, s, rows, d_ids, d_off, d_slot, d_out);
}

void launch_refpos_walk(const DeviceIndex &ix, const RefposRows &rows, const RefposWalk &w, bool fast, hipStream_t s) {
    if (w.walkers == 0) return;
    if (fast) hipLaunchKernelGGL(k_refpos_walk<true>, blocks_for(w.walkers), dim3(256), 0, s, ix, rows, w);
    else hipLaunchKernelGGL(k_refpos_walk<false>, blocks_for(w.walkers), dim3(256), 0, s, ix, rows, w);
}

}  // namespace gbwt_hip
