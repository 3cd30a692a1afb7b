// fm_seed_plan.hpp -- every decision of a seeds request (fm_seeds.hip, capi_fm_seeds.hip) as arithmetic over numbers the host has before
// the first kernel: plain C++, no HIP (tests/cpp/fm_seed_plan.cpp runs it without a GPU).  From the reads, their bytes, the strands, whether
// hits are asked for, the temporary storage of the scan and the free device memory: the slots of every scratch buffer, their bytes, and
// whether the request is served.
//
// The host does not know the lengths of reads given on the device, so every buffer is sized by what (reads, bytes) allow at most.  With
// Q = reads x strands items and B = read bytes x strands:
//   anchors   at most Q + B / K     u64 count and offset per item; start, range (u32 each) and item per anchor; u64 count and offset of
//                                   the refined ends in front of every anchor
//   refined   at most B             start and range (u32 each) per refined end
//   ends      anchors + refined     u64 flag and rank per end whose start is known
//   hits      at most B seeds       the clamped range (2 x u64) and the row length (u64) per seed
// and the temporary storage of the scan over the ends, and four words.  All of it is allocated before the first kernel and freed before
// the request returns; the rows of the result -- seeds, offsets, hits -- stay in the object and are not scratch.
#pragma once

#include <cstdint>
#include <string>

#include "fm_plan.hpp"
#include "fm_seeds.hpp"

namespace gbwt_hip {

constexpr uint64_t FM_SEED_MAX_READS = 0x7FFFFFFFull;          // as every query: at most 2^31 - 2 patterns
constexpr uint64_t FM_SEED_MAX_BYTES = 0xFFFFFFFFull;          // starts and ends of seeds are u32
constexpr uint64_t FM_SEED_MIN_BUFFER = 256;                   // counted_buffer.hpp allocates no less
constexpr uint64_t FM_SEED_WORDS = 4;                          // [0] flags, [1] backward steps, [2] the longest lanes of the waves

struct FmSeedPlan {
    FmStatus status = FmStatus::Ok;
    bool bad_argument = false;        // with Unsupported: the request is malformed, not merely too large
    std::string message;
    uint32_t stride = FM_SEED_STRIDE, strands = 0;
    uint64_t items = 0, anchor_slots = 0, refined_slots = 0, end_slots = 0, seed_slots = 0;
    uint64_t item_bytes = 0, anchor_bytes = 0, refined_bytes = 0, end_bytes = 0, hit_bytes = 0, temp_bytes = 0, words_bytes = 0, scratch_bytes = 0;
};

// What is refused whatever the memory
inline FmSeedPlan fm_seed_check(uint64_t reads, uint64_t read_bytes, uint32_t strands) {
    FmSeedPlan p;
    p.strands = strands;
    if (strands < 1 || strands > 3) {
        p.status = FmStatus::Unsupported;
        p.bad_argument = true;
        p.message = "strands: 1 (forward), 2 (reverse) or 3 (both)";
    } else if (reads >= FM_SEED_MAX_READS) {
        p.status = FmStatus::Unsupported;
        p.bad_argument = true;
        p.message = "too many patterns in one request (at most 2^31 - 2)";
    } else if (read_bytes > FM_SEED_MAX_BYTES) {
        p.status = FmStatus::Unsupported;
        p.message = "reads of " + std::to_string(read_bytes) + " bytes in one request are not supported: more than 2^32 - 1 (u32 starts and ends of seeds)";
    }
    return p;
}

// the largest scan of a request runs over fm_seed_end_slots items
inline uint64_t fm_seed_end_slots(uint64_t reads, uint64_t read_bytes, uint32_t strands, uint32_t K = FM_SEED_STRIDE) {
    const uint64_t ns = fm_strand_count(strands), Q = reads * ns, B = read_bytes * ns;
    return Q + B / K + B;
}

// temp_bytes: what the scan over fm_seed_end_slots items asks for; free_bytes: hipMemGetInfo
inline FmSeedPlan fm_seed_plan(uint64_t reads, uint64_t read_bytes, uint32_t strands, bool hits, uint64_t temp_bytes, uint64_t free_bytes, uint32_t K = FM_SEED_STRIDE) {
    FmSeedPlan p = fm_seed_check(reads, read_bytes, strands);
    if (p.status != FmStatus::Ok) return p;
    const auto buffer = [](uint64_t bytes) { return bytes < FM_SEED_MIN_BUFFER ? FM_SEED_MIN_BUFFER : bytes; };
    const uint64_t ns = fm_strand_count(strands), B = read_bytes * ns;
    p.stride = K;
    p.items = reads * ns;
    p.anchor_slots = p.items + B / K;
    p.refined_slots = B;
    p.end_slots = p.anchor_slots + p.refined_slots;
    p.seed_slots = hits ? B : 0;
    p.item_bytes = buffer(p.items * sizeof(uint64_t)) + buffer((p.items + 1) * sizeof(uint64_t));
    p.anchor_bytes = 4 * buffer(p.anchor_slots * sizeof(uint32_t)) + buffer(p.anchor_slots * sizeof(uint64_t)) + buffer((p.anchor_slots + 1) * sizeof(uint64_t));
    p.refined_bytes = 3 * buffer(p.refined_slots * sizeof(uint32_t));
    p.end_bytes = buffer(p.end_slots * sizeof(uint64_t)) + buffer((p.end_slots + 1) * sizeof(uint64_t));
    p.hit_bytes = hits ? buffer(2 * p.seed_slots * sizeof(uint64_t)) + buffer(p.seed_slots * sizeof(uint64_t)) : 0;
    p.temp_bytes = buffer(temp_bytes);
    p.words_bytes = buffer(FM_SEED_WORDS * sizeof(uint64_t));
    p.scratch_bytes = p.item_bytes + p.anchor_bytes + p.refined_bytes + p.end_bytes + p.hit_bytes + p.temp_bytes + p.words_bytes;
    if (p.scratch_bytes > free_bytes) {
        p.status = FmStatus::Capacity;
        p.message = "the seeds of " + std::to_string(reads) + " reads of " + std::to_string(read_bytes) + " bytes need " + std::to_string(p.scratch_bytes) +
                    " bytes of device memory while they are searched; " + std::to_string(free_bytes) + " are free";
    }
    return p;
}

}  // namespace gbwt_hip
