// sa_plan.hpp -- every decision of a suffix array request (suffix_array.hip) as arithmetic over numbers the host has: plain C++, no HIP
// (tests/cpp/sa_plan.cpp runs it without a GPU).  From the length of the text, the temporary storage the library sorts, scans and selects
// ask for and the free device memory: the widths, the scratch of every phase, the peak, and whether the request is served.
//
// Ranks and positions inside the builder are 32 bits wide; a rank is 1 .. n, and n + 1 must still be a value: n <= 2^32 - 2.
//
// Scratch per position, all of it allocated before the first kernel and freed before the call returns:
//   rank, sa           u32 each    the inverse and the suffix array as they settle                         8
//   key a / b          u64 each    keys in front of and behind a sort                                     16
//   pos a / b          u32 each    the suffixes that travel with the keys                                  8
//   slot a / b         u32 each    the place in `sa` of every entry of the active set, this round / next   8
//   dense              u32         head marks, then the ranks a max-scan makes of them                     4
//   picked             u32         the entries that stay active, selected                                   4
//   flag               u8          stays active                                                             1
// = 49 bytes, + the temporary storage, + one smallest buffer (256 bytes) for the two counters.  The results (u64 suffix array, the BWT) are the caller's.
#pragma once

#include <cstdint>
#include <string>

#include "sa_key.hpp"

namespace gbwt_hip {

constexpr uint64_t SA_MAX_TEXT = 0xFFFFFFFEull;      // 2^32 - 2
constexpr uint64_t SA_MIN_BUFFER = 256;              // what the smallest device buffer takes (device_buffer.hpp)
constexpr uint32_t SA_INFO_ROUNDS = 64;              // rounds gbwt_hip_suffix_array_info has room for

enum class SaStatus { Ok, Unsupported, Capacity };

struct SaPlan {
    SaStatus status = SaStatus::Ok;
    std::string message;
    uint64_t n = 0;
    uint32_t rank_bits = 0, key_bits = 0, first_key_bits = 64;   // bits of a rank, of a round's key, of the first key
    // bytes of the buffers (each at least SA_MIN_BUFFER, none for an empty text)
    uint64_t rank_bytes = 0, sa_bytes = 0, key_bytes = 0, pos_bytes = 0, slot_bytes = 0, dense_bytes = 0, picked_bytes = 0, flag_bytes = 0, temp_bytes = 0, words_bytes = 0;
    uint64_t settled_bytes = 0;     // rank + sa: alive from the pack to the output
    uint64_t sort_bytes = 0;        // both keys and both positions
    uint64_t round_bytes = 0;       // slots, dense, picked, flag, temporary storage, counters
    uint64_t peak_bytes = 0;        // all three: nothing is allocated or freed between the pack and the output
};

// temp_bytes: the largest temporary storage any of the sorts, the scan and the select of n items asks for; free_bytes: hipMemGetInfo
inline SaPlan sa_plan(uint64_t n, uint64_t temp_bytes, uint64_t free_bytes) {
    SaPlan p;
    p.n = n;
    if (n > SA_MAX_TEXT) {
        p.status = SaStatus::Unsupported;
        p.message = "a text of " + std::to_string(n) + " positions is not supported: more than 2^32 - 2 (u32 ranks and positions on device)";
        return p;
    }
    if (n == 0) return p;
    const auto buffer = [](uint64_t bytes) { return bytes < SA_MIN_BUFFER ? SA_MIN_BUFFER : bytes; };
    p.rank_bits = sa_rank_bits(n);
    p.key_bits = 2 * p.rank_bits;
    p.rank_bytes = p.sa_bytes = p.pos_bytes = p.slot_bytes = p.dense_bytes = p.picked_bytes = buffer(4 * n);
    p.key_bytes = buffer(8 * n);
    p.flag_bytes = buffer(n);
    p.temp_bytes = buffer(temp_bytes);
    p.words_bytes = SA_MIN_BUFFER;
    p.settled_bytes = p.rank_bytes + p.sa_bytes;
    p.sort_bytes = 2 * p.key_bytes + 2 * p.pos_bytes;
    p.round_bytes = 2 * p.slot_bytes + p.dense_bytes + p.picked_bytes + p.flag_bytes + p.temp_bytes + p.words_bytes;
    p.peak_bytes = p.settled_bytes + p.sort_bytes + p.round_bytes;
    if (p.peak_bytes > free_bytes) {
        p.status = SaStatus::Capacity;
        p.message = "the suffix array of " + std::to_string(n) + " positions needs " + std::to_string(p.peak_bytes) + " bytes of device memory for its ranking; " +
                    std::to_string(free_bytes) + " are free";
    }
    return p;
}

}  // namespace gbwt_hip
