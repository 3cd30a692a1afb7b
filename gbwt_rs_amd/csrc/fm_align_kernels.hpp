// fm_align_kernels.hpp -- the kernels of the alignment behind a chains request (fm_align.hip) as the C ABI launches them (capi_fm_align.hip).
// What a band, a cell and a direction are is fm_align.hpp; the sizes of the buffers are fm_align_plan.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/gbwt_hip.h"
#include "fm_align.hpp"
#include "fm_align_plan.hpp"

namespace gbwt_hip {

// One considered chain: what k_align_setup finds out about it, and what k_align_dp leaves
struct FmAlignTask {
    int64_t d0;
    uint64_t lo, hi;                  // the segment: [lo, hi) are its bases
    uint64_t read_first;              // the read: bytes [read_first, read_first + L)
    uint64_t text_start, text_end;
    uint32_t L, W, chain, status, strand, path, edit_distance, reserved;
};
static_assert(sizeof(FmAlignTask) == FM_ALIGN_TASK_BYTES, "a task as fm_align_plan.hpp counts it");

// The rows of the chains step and the arrays the alignment passes on.  ITEMS as in fm_chain_kernels.hpp; ALIGNMENTS of item q:
// [item_offsets[q], item_offsets[q + 1]), the first chains of the item in peeling order.
struct AlignBatch {
    // the reads and the chains step
    const uint64_t *q_offsets;                // [m + 1]
    const uint8_t *q_bytes;
    const uint64_t *chain_read_offsets;       // [m + 1]
    const gbwt_hip_fm_chain *chains;          // [total_chains]
    const uint64_t *chain_match_offsets;      // [total_chains + 1]
    const gbwt_hip_fm_chain_match *matches;
    uint64_t m;
    uint32_t strands, ns;
    // the text, and the segments: the text offsets of the paths [n_paths + 1], or null on an index of a plain text
    const uint8_t *text;
    uint64_t n;
    const uint64_t *path_offsets;
    uint64_t n_paths;
    // the options
    uint32_t band, max_width;
    uint64_t max_alignments;
    uint64_t items, alignments;
    uint64_t *item_counts, *item_offsets, *item_first;         // [items], [items + 1], [items]
    FmAlignTask *tasks;                                        // [alignments]
    uint64_t *direction_words, *direction_offsets;             // [alignments], [alignments + 1]: the alignments beyond the tile, in u32 words
    uint64_t *cigar_bound, *cigar_first, *cigar_count;         // [alignments], [alignments + 1], [alignments]
    uint32_t *directions, *cigar_scratch;
    uint64_t *words;                                           // fm_align_plan.hpp: FM_ALIGN_WORDS
};

// item_counts[q] = the chains of item q that are considered, item_first[q] = its first chain in the chains rows
void launch_align_select(const AlignBatch &b, hipStream_t s);
// Behind the scan of the counts: one lane per alignment reads the members of its chain: band, bounds, status, and what it needs of the scratch
void launch_align_setup(const AlignBatch &b, hipStream_t s);
// The DP and the walk back: one wave per alignment
void launch_align_dp(const AlignBatch &b, hipStream_t s);
// Behind the scan of the CIGAR counts (into d_cigar_offsets): the rows
void launch_align_rows(const AlignBatch &b, uint64_t *d_read_offsets, gbwt_hip_fm_alignment *d_alignments, const uint64_t *d_cigar_offsets, uint32_t *d_cigars, hipStream_t s);

}  // namespace gbwt_hip
