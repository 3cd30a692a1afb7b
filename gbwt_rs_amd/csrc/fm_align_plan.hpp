// fm_align_plan.hpp -- every decision of the alignment behind a chains request (fm_align.hip, capi_fm_align.hip) as arithmetic over numbers
// the host has before the first alignment kernel: plain C++, no HIP (tests/cpp/fm_align_plan.cpp runs it without a GPU).  From the items
// (reads x strands), the chains considered, the direction words of the alignments whose directions do not fit the LDS tile, the bound on
// the CIGAR entries, the temporary storage of the scans and the free device memory: the bytes of every scratch buffer, and whether the
// request is served.
//
// With Q items and A considered chains (one alignment each):
//   items       u64 count, u64 first alignment (Q + 1), u64 first chain of the item in the chains rows
//   tasks       one FM_ALIGN_TASK_BYTES record per alignment: band, bounds, read, status, and the result of the DP
//   sizes       u64 direction words and their offsets (A + 1), u64 CIGAR bound and its offsets (A + 1), u64 CIGAR entries written
//   directions  u32 per direction word of the alignments that run over global memory: L x ceil(W / 16) words each
//   cigars      u32 per entry of the bound
// and the temporary storage, and FM_ALIGN_WORDS words.  The selection (k_align_select, k_align_setup and their scans) yields A and the
// two sums; everything is allocated before k_align_dp, the first kernel that aligns, and freed before the request returns.  (The issue
// asked for a function of the sum of the cells; the directions in global memory are the sum over the alignments beyond the tile only, so
// the plan takes that sum instead: the cells are a count of the info and size nothing.)
//
// THE CIGAR BOUND of one computed alignment of a read of L bytes is 2 L entries.  An entry is a run.  Every run of =, X or I consumes at
// least one read byte, so there are at most L of them; a run of D is followed by a run that is not D (the smallest end: no trailing
// deletion), and two runs of D are never neighbours, so there are at most as many runs of D as of the others.  (Likewise a reachable cell
// holds at most L: from the start max(lo, d0) of row 0 a walk of insertions and then diagonals reaches every existing cell of row L
// inside the band at a cost of at most L.)  WIDE and NONE alignments have an empty CIGAR and a bound of 0.
#pragma once

#include <cstdint>
#include <string>

#include "fm_align.hpp"
#include "fm_plan.hpp"

namespace gbwt_hip {

constexpr uint64_t FM_ALIGN_MIN_BUFFER = 256;                  // counted_buffer.hpp allocates no less
constexpr uint64_t FM_ALIGN_WORDS = 8;                         // [0] computed, [1] wide, [2] unreachable, [3] cells, [4] LDS, [5] global, [6] reads too long
constexpr uint64_t FM_ALIGN_TASK_BYTES = 80;
constexpr uint64_t FM_ALIGN_MAX_ALIGNMENTS = 0x7FFFFFFFull;    // one wave each: the grid of k_align_dp

struct FmAlignPlan {
    FmStatus status = FmStatus::Ok;
    std::string message;
    uint64_t items = 0, alignments = 0;
    uint64_t item_bytes = 0, task_bytes = 0, size_bytes = 0, direction_bytes = 0, cigar_bytes = 0, temp_bytes = 0, words_bytes = 0, scratch_bytes = 0;
};

// temp_bytes: what the scans over max(items, alignments) + 1 values ask for; free_bytes: hipMemGetInfo, plus what the request already holds
inline FmAlignPlan fm_align_plan(uint64_t items, uint64_t alignments, uint64_t direction_words, uint64_t cigar_entries, uint64_t temp_bytes, uint64_t free_bytes) {
    FmAlignPlan p;
    p.items = items;
    p.alignments = alignments;
    if (alignments > FM_ALIGN_MAX_ALIGNMENTS) {
        p.status = FmStatus::Unsupported;
        p.message = "the alignments of " + std::to_string(alignments) + " chains in one request are not supported: 2^31 or more (ask for fewer reads per call, or a smaller max_alignments)";
        return p;
    }
    const auto buffer = [](uint64_t bytes) { return bytes < FM_ALIGN_MIN_BUFFER ? FM_ALIGN_MIN_BUFFER : bytes; };
    p.item_bytes = buffer(items * sizeof(uint64_t)) + buffer((items + 1) * sizeof(uint64_t)) + buffer(items * sizeof(uint64_t));
    p.task_bytes = buffer(alignments * FM_ALIGN_TASK_BYTES);
    p.size_bytes = 3 * buffer(alignments * sizeof(uint64_t)) + 2 * buffer((alignments + 1) * sizeof(uint64_t));
    p.direction_bytes = buffer(direction_words * sizeof(uint32_t));
    p.cigar_bytes = buffer(cigar_entries * sizeof(uint32_t));
    p.temp_bytes = buffer(temp_bytes);
    p.words_bytes = buffer(FM_ALIGN_WORDS * sizeof(uint64_t));
    p.scratch_bytes = p.item_bytes + p.task_bytes + p.size_bytes + p.direction_bytes + p.cigar_bytes + p.temp_bytes + p.words_bytes;
    if (p.scratch_bytes > free_bytes) {
        p.status = FmStatus::Capacity;
        p.message = "the alignments of " + std::to_string(alignments) + " chains of " + std::to_string(items) + " items need " + std::to_string(p.scratch_bytes) +
                    " bytes of device memory while they are aligned; " + std::to_string(free_bytes) + " are free";
    }
    return p;
}

}  // namespace gbwt_hip
