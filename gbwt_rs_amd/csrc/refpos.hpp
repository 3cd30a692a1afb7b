// refpos.hpp -- launch wrappers of the reference-position kernels (refpos.hip; the entry points are in capi_refpos.hip, the two scans of a
// request are scan.hpp's).
#pragma once

#include "capi_internal.hpp"

namespace gbwt_hip {

constexpr uint32_t REFPOS_MAX_ROUNDS = 32;            // pointer-doubling rounds of a request of at most 2^32 - 1 positions
constexpr uint32_t REFPOS_FLAG_MISMATCH = REFPOS_MAX_ROUNDS, REFPOS_FLAGS = REFPOS_MAX_ROUNDS + 8;   // u32 words of the flag block: one per round, then the walk's

// The extracted rows of a request: row r = nodes[offsets[r] .. offsets[r + 1]), `positions` = offsets[n] (<= 2^32 - 1: it is the sentinel of the u32 jumps)
struct RefposRows { const uint64_t *offsets; const uint32_t *nodes; uint64_t n, positions; };

// len[i] = label length of the node of position i
void launch_refpos_lengths(const RefposRows &rows, const Labels &L, uint64_t *d_len, hipStream_t s);
// jump[i] = the first k > i of the row of i with off_k >= off_i + interval (saturating, offsets inside the row), or `positions`; jump[positions] = positions
void launch_refpos_succ(const RefposRows &rows, const uint64_t *d_off, uint64_t interval, uint32_t *d_jump, hipStream_t s);
// mark[first position of every row with nodes] = 1 (d_mark zeroed by the caller)
void launch_refpos_first_marks(const RefposRows &rows, uint64_t *d_mark, hipStream_t s);
// Round t of the pointer doubling: every marked i marks jump[i], next[i] = jump[jump[i]]; flags[t] != 0 when a mark was new.  A round
// behind one that marked nothing new does nothing.
void launch_refpos_round(uint64_t *d_mark, const uint32_t *d_jump, uint32_t *d_next, uint64_t positions, uint32_t *d_flags, uint32_t t, hipStream_t s);
// out[r] = {ids[r], bases of row r, its first slot, its slots}
void launch_refpos_paths(const RefposRows &rows, const uint64_t *d_ids, const uint64_t *d_off, const uint64_t *d_slot, gbwt_hip_reference_path *d_out, hipStream_t s);

// The LF walk that carries the in-record offset: one lane per sample segment of every row (seg_first[r] = lanes in front of row r;
// segmented = 0: one lane per row, from its start).  fast: the handle has raw descriptors and rank blocks (the O(1) step of k_forward),
// else every step decodes the record bytes (gbwt_forward).  flags[REFPOS_FLAG_MISMATCH] != 0: a lane met another node than its row holds.
struct RefposWalk {
    const uint64_t *seq_ids, *seg_first;   // [n], [n + 1]
    uint64_t walkers;                      // = seg_first[n]
    uint32_t segmented;
    const uint64_t *off, *slot;            // [positions + 1] each
    gbwt_hip_reference_position *out;      // [slot[positions]]
    uint32_t *flags;
};
void launch_refpos_walk(const DeviceIndex &ix, const RefposRows &rows, const RefposWalk &w, bool fast, hipStream_t s);

}  // namespace gbwt_hip
