// fm_plan.hpp -- every decision of an FM-index build (fm_index.hip, capi_fm.hip) as arithmetic over numbers the host has: plain C++, no HIP
// (tests/cpp/fm_plan.cpp runs it without a GPU).  From the length of the text, its alphabet -- known once the histogram is back --, the
// temporary storage of the scan and the free device memory: the layout, the bytes the index keeps, the scratch of the build, the peak, and
// whether the request is served.
//
// The index (fm_layout.hpp), per position of a long text:
//   packed (sigma <= 8)   128 bytes per 96 rows                           1.33
//   plain  (sigma > 8)    1 byte per row + 4 sigma bytes per 256 rows     1 + sigma / 64   (5 at sigma = 256)
//   SA                    u32, unless the index is count-only             4
//   tables                code u16[256], C u32[256]                       1536 bytes
// Scratch, all of it allocated before the first build kernel and freed before the build returns:
//   histogram             u64[256]
//   counts, scanned       u32 each per (code, block): the occurrences in a block, then in front of it
//   temporary storage of the scan, one word for the primary row
//   the u64 suffix array  8 bytes per position, where the caller brings none (its ranking is sa_plan.hpp's, checked by that plan)
#pragma once

#include <cstdint>
#include <string>

#include "fm_layout.hpp"
#include "sa_plan.hpp"

namespace gbwt_hip {

constexpr uint64_t FM_TABLE_BYTES = 256 * sizeof(uint16_t) + 256 * sizeof(uint32_t);
constexpr uint64_t FM_HISTOGRAM_BYTES = 256 * sizeof(uint64_t);

enum class FmStatus { Ok, Unsupported, Capacity };

struct FmPlan {
    FmStatus status = FmStatus::Ok;
    std::string message;
    uint64_t n = 0, rows = 1, blocks = 1;
    uint32_t sigma = 0, block_rows = FM_PACKED_BLOCK;
    bool packed = true;
    // what the index keeps (each buffer at least SA_MIN_BUFFER; no counts buffer in the packed layout, no SA in a count-only index)
    uint64_t lines_bytes = 0, counts_bytes = 0, tables_bytes = 0, sa_bytes = 0, index_bytes = 0;
    // scratch of the build
    uint64_t histogram_bytes = 0, block_count_bytes = 0, temp_bytes = 0, words_bytes = 0, sa64_bytes = 0, scratch_bytes = 0;
    uint64_t peak_bytes = 0;          // index + scratch: nothing is freed before the fill is done
};

// The width alone: decided before any work, whatever the alphabet and the memory
inline FmPlan fm_check_width(uint64_t n) {
    FmPlan p;
    p.n = n;
    if (n > SA_MAX_TEXT) {
        p.status = FmStatus::Unsupported;
        p.message = "a text of " + std::to_string(n) + " positions is not supported: more than 2^32 - 2 (u32 suffix array and counts in the FM-index)";
    }
    return p;
}

// own_sa: the build makes the u64 suffix array itself; temp_bytes: what the scan of the block counts asks for; free_bytes: hipMemGetInfo
inline FmPlan fm_plan(uint64_t n, uint32_t sigma, bool count_only, bool own_sa, uint64_t temp_bytes, uint64_t free_bytes) {
    FmPlan p = fm_check_width(n);
    if (p.status != FmStatus::Ok) return p;
    const auto buffer = [](uint64_t bytes) { return bytes < SA_MIN_BUFFER ? SA_MIN_BUFFER : bytes; };
    p.sigma = sigma;
    p.packed = fm_is_packed(sigma);
    p.block_rows = fm_block_rows(p.packed);
    p.rows = n + 1;
    p.blocks = fm_blocks(p.rows, p.packed);
    p.lines_bytes = buffer(p.blocks * fm_block_bytes(p.packed));
    p.counts_bytes = p.packed ? 0 : buffer(p.blocks * sigma * sizeof(uint32_t));
    p.tables_bytes = FM_TABLE_BYTES;
    p.sa_bytes = count_only || n == 0 ? 0 : buffer(n * sizeof(uint32_t));
    p.index_bytes = p.lines_bytes + p.counts_bytes + p.tables_bytes + p.sa_bytes;
    p.histogram_bytes = FM_HISTOGRAM_BYTES;
    p.words_bytes = SA_MIN_BUFFER;
    if (n != 0) {
        p.block_count_bytes = buffer(p.blocks * sigma * sizeof(uint32_t));
        p.temp_bytes = buffer(temp_bytes);
        p.sa64_bytes = own_sa ? buffer(n * sizeof(uint64_t)) : 0;
    }
    p.scratch_bytes = p.histogram_bytes + p.words_bytes + 2 * p.block_count_bytes + p.temp_bytes + p.sa64_bytes;
    p.peak_bytes = p.index_bytes + p.scratch_bytes;
    if (p.peak_bytes > free_bytes) {
        p.status = FmStatus::Capacity;
        p.message = "the FM-index of " + std::to_string(n) + " positions needs " + std::to_string(p.peak_bytes) + " bytes of device memory while it is built; " +
                    std::to_string(free_bytes) + " are free";
    }
    return p;
}

}  // namespace gbwt_hip
