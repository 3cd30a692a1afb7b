// fm_chain_plan.hpp -- every decision of the chaining behind a seeds request (fm_chains.hip, capi_fm_chains.hip) as arithmetic over numbers
// the host has before the first chaining kernel: plain C++, no HIP (tests/cpp/fm_chain_plan.cpp runs it without a GPU).  From the hits of
// the seeds step, the items (reads x strands), the temporary storage of the sorts and scans and the free device memory: the bytes of every
// scratch buffer, and whether the request is served.
//
// The matches are the hits of the items that max_matches does not skip, so every buffer is sized by the hits H; with Q items:
//   items     u64 count, u64 first match (Q + 1), u64 first hit (Q + 1)
//   sort      2 x (u64 key, u64 value) per hit: the matches by (item, y), carrying (x, w); reused by the sort into visiting order
//   matches   y, x, w, low, segment, f, pred: u32 each
//   peel      a byte `used`; the slot of its chain and its distance from the head per match; score and tail per visiting slot: u32 each
//   rows      u64 flag and rank, u64 members and their rank per visiting slot (scan.hpp's sums are u64)
// and the temporary storage, and four words.  109 bytes per hit and 24 per item: all of it is allocated before the first chaining kernel
// and freed before the request returns; the rows of the result stay in the object and are not scratch.
#pragma once

#include <cstdint>
#include <string>

#include "fm_plan.hpp"

namespace gbwt_hip {

constexpr uint64_t FM_CHAIN_MAX_HITS = 0x7FFFFFFFull;          // the sorts count in int, indices of matches are u32 with one value kept free
constexpr uint64_t FM_CHAIN_MIN_BUFFER = 256;                  // counted_buffer.hpp allocates no less
constexpr uint64_t FM_CHAIN_WORDS = 4;                         // [0] skipped items, [1] pairs
constexpr uint64_t FM_CHAIN_TILE = 512;                        // matches of an item that k_chain_dp stages in LDS: 12 bytes each, 4 waves a workgroup

struct FmChainPlan {
    FmStatus status = FmStatus::Ok;
    std::string message;
    uint64_t hits = 0, items = 0;
    uint64_t item_bytes = 0, sort_bytes = 0, match_bytes = 0, peel_bytes = 0, row_bytes = 0, temp_bytes = 0, words_bytes = 0, scratch_bytes = 0;
};

// temp_bytes: the most that the two sorts over `hits` pairs and the scans over max(hits, items) + 1 values ask for; free_bytes: hipMemGetInfo
inline FmChainPlan fm_chain_plan(uint64_t hits, uint64_t items, uint64_t temp_bytes, uint64_t free_bytes) {
    FmChainPlan p;
    p.hits = hits;
    p.items = items;
    if (hits > FM_CHAIN_MAX_HITS) {
        p.status = FmStatus::Unsupported;
        p.message = "the chains of a request with " + std::to_string(hits) + " hits are not supported: 2^31 or more matches (ask for fewer reads per call, or a smaller max_occurrences)";
        return p;
    }
    const auto buffer = [](uint64_t bytes) { return bytes < FM_CHAIN_MIN_BUFFER ? FM_CHAIN_MIN_BUFFER : bytes; };
    p.item_bytes = buffer(items * sizeof(uint64_t)) + 2 * buffer((items + 1) * sizeof(uint64_t));
    p.sort_bytes = 4 * buffer(hits * sizeof(uint64_t));
    p.match_bytes = 7 * buffer(hits * sizeof(uint32_t));
    p.peel_bytes = buffer(hits) + 4 * buffer(hits * sizeof(uint32_t));
    p.row_bytes = 2 * buffer(hits * sizeof(uint64_t)) + 2 * buffer((hits + 1) * sizeof(uint64_t));
    p.temp_bytes = buffer(temp_bytes);
    p.words_bytes = buffer(FM_CHAIN_WORDS * sizeof(uint64_t));
    p.scratch_bytes = p.item_bytes + p.sort_bytes + p.match_bytes + p.peel_bytes + p.row_bytes + p.temp_bytes + p.words_bytes;
    if (p.scratch_bytes > free_bytes) {
        p.status = FmStatus::Capacity;
        p.message = "the chains of " + std::to_string(hits) + " hits of " + std::to_string(items) + " items need " + std::to_string(p.scratch_bytes) +
                    " bytes of device memory while they are chained; " + std::to_string(free_bytes) + " are free";
    }
    return p;
}

}  // namespace gbwt_hip
