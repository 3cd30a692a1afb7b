// fm_seed_kernels.hpp -- the kernels of a seeds request (fm_seeds.hip) as the C ABI launches them (capi_fm_seeds.hip).  What a start, an anchor
// and a seed are is fm_seeds.hpp; the sizes of the buffers are fm_seed_plan.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gbwt_hip.h"
#include "fm_index.hpp"
#include "fm_seeds.hpp"

namespace gbwt_hip {

// The reads of a request and the arrays its kernels pass on.  ITEMS, strand-major: item q = read q % m on the (q / m)-th strand of the request.
// ANCHORS of item q: [anchor_offsets[q], anchor_offsets[q + 1]), ascending by end.  REFINED ends in front of anchor g:
// [refined_offsets[g], refined_offsets[g + 1]).  The ENDS whose start is known stand in one order -- items, and inside an item by end:
// anchor g at g + refined_offsets[g + 1], refined end j in front of anchor g at g + j.
struct SeedBatch {
    FmLayout L;
    FmTables t;
    const uint64_t *offsets;          // [m + 1]
    const uint8_t *bytes;             // [total_bytes]
    uint64_t m, total_bytes;
    uint32_t strands, min_length;
    uint64_t items, anchors, refined;
    uint64_t *anchor_counts, *anchor_offsets;                  // [items], [items + 1]
    uint32_t *anchor_start, *anchor_lo, *anchor_hi, *anchor_item;
    uint64_t *refined_counts, *refined_offsets;                // [anchors], [anchors + 1]
    uint32_t *refined_start, *refined_lo, *refined_hi;
    uint64_t *flags, *rank;                                    // [anchors + refined], one more
    uint64_t *words;                                           // [0] flags (FM_FLAG_OFFSETS), [1] += backward steps, [2] += the longest lane of every wave, [3] += seeds over max_occurrences
};

// anchor_counts[q] = the anchors of item q; offsets that descend or leave the bytes raise FM_FLAG_OFFSETS and count as an empty read
void launch_seed_anchor_count(const SeedBatch &b, hipStream_t s);
// One lane per anchor: its start and range, and its item
void launch_seed_anchors(const SeedBatch &b, hipStream_t s);
// refined_counts[g] = the ends in front of anchor g that have to be searched
void launch_seed_refine_count(const SeedBatch &b, hipStream_t s);
// One lane per refined end: its start and range
void launch_seed_refine(const SeedBatch &b, hipStream_t s);
// flags[position of an end] = 1 where the end closes a seed
void launch_seed_flags(const SeedBatch &b, hipStream_t s);
// Behind the scan of the flags into rank: the seeds, the offsets of the reads' rows [m + 1], and -- where d_hit_ranges is not null -- per
// seed the range to locate ((lo, lo) for more than max_occurrences) and its length
void launch_seed_fill(const SeedBatch &b, gbwt_hip_fm_seed *d_seeds, uint64_t *d_read_offsets, uint64_t max_occurrences, uint64_t *d_hit_ranges, uint64_t *d_hit_counts, hipStream_t s);

}  // namespace gbwt_hip
