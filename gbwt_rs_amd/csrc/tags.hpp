// tags.hpp -- launch wrappers of tags.hip: the position map of a tag plan (node and label length of every position, the text offset of every
// row, the sampled top level; the scan of the lengths in between is scan.hpp's) and the gather of one batch of suffix array values.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "labels.hpp"

namespace gbwt_hip {

constexpr uint32_t TAG_SHIFT = 5;                                   // one hint per 32 text offsets

// What a request leaves behind: the runs counted so far, the last tag of the batches (two slots in turn: a batch reads the one its
// predecessor wrote while its own last workgroup writes the other), and whether a value was out of range.
struct TagState { unsigned long long runs; uint64_t last[2]; uint32_t bad, reserved; };
static_assert(sizeof(TagState) == 32, "copied as a whole");

// The position map of a plan as the host holds it: top has a hint per (1 << TAG_SHIFT) text offsets and one more, u64 when wide and u32
// otherwise; off[positions + 1]; node[positions]
struct TagTables { const void *top; bool wide; const uint64_t *off; const uint32_t *node; uint64_t text_len; };

// node and label length of every position of the rows (CSR: d_offsets[n + 1], d_nodes) with one endmarker position behind each row
void launch_tag_positions(const uint64_t *d_offsets, const uint32_t *d_nodes, uint64_t n, uint64_t positions, const Labels &L, uint32_t *d_pos_node, uint64_t *d_pos_len,
                          hipStream_t s);
// d_rows[n + 1]: the text offset of every row, and the text length behind the last
void launch_tag_rows(const uint64_t *d_offsets, uint64_t n, const uint64_t *d_pos_off, uint64_t positions, uint64_t *d_rows, hipStream_t s);
void launch_tag_top(const uint64_t *d_pos_off, uint64_t positions, uint64_t hints, void *d_top, bool wide, hipStream_t s);
// One batch of the gather (nothing is waited for): d_tags[i] = tag(d_sa[i]) for i < count, runs and the out-of-range flag into d_state.
// has_prev: a batch in front of this one has left its last tag in d_state->last[parity ^ 1].
void launch_tags(int device, const TagTables &t, const uint64_t *d_sa, uint64_t count, uint64_t *d_tags, TagState *d_state, bool has_prev, uint32_t parity, hipStream_t s);

}  // namespace gbwt_hip
