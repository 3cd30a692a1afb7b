// extract_knobs.hpp -- the GBWT_HIP_* settings of a workspace (plain C++: extract_plan.hpp decides from them, knobs.hpp includes this).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

// The GBWT_HIP_* tuning / measurement switches of an extraction, read ONCE when the workspace is created: gbwt_hip_extract_device
// itself never looks at the environment (getenv is not safe against a concurrent setenv, and several host threads extract from one
// index at the same time, each with its own workspace -- include/gbwt_hip.h).  -1 = not set: the library's default for the batch.
struct ExtractKnobs {
    int direct = 1, segments = 1, both_ends = 1;             // GBWT_HIP_DIRECT / _SEGMENTS / _BOTH_ENDS (0 switches the feature off)
    int all4 = 1;                                             // GBWT_HIP_ALL4: 0 = the uniform loop counts every node it stages (rounds 1-3)
    int sample_stride = -1;                                   // GBWT_HIP_SAMPLE_STRIDE: a walker per this many samples of a row; -1 = by the size of the batch (gbwt_hip_extract_device)
    int defer_total = 1;                                      // GBWT_HIP_DEFER_TOTAL: 0 = every request waits for the total of its row lengths before it launches the walk (rounds 1-3)
    int fused_offsets = 1;                                    // GBWT_HIP_FUSED_OFFSETS: 0 = the offsets of a batch of equally long rows come from k_row_offsets in front of the walk, as every batch's did until round 6 (WalkArgs::uniform_len)
    int ring_slots = -1, helper_naps = -1, xcd_map = -1, uniform_loop = -1, packed_blocks = -1, row_piece = -1, catch_up = -1, headroom = 0;
    int gather_reach = -1;                                    // GBWT_HIP_GATHER_REACH: look-ahead of mixed waves (WalkArgs::gather_reach); -1 = by the index (rows per record), 0 = none
    bool wide_addresses = false;                              // GBWT_HIP_WIDE_ADDRESSES set (any value)
    uint32_t debug = 0;                                       // GBWT_HIP_DEBUG_DRY_ROWS (measurement switches, WalkArgs::debug)
    unsigned copy_threads = 8;                                // GBWT_HIP_COPY_THREADS
    uint64_t locate_sort_piece = 0x7FFFFFFFull;               // GBWT_HIP_LOCATE_SORT_PIECE: items of one radix sort of a unique locate request (hipcub counts in int; tests lower it)
    uint64_t scan_piece = uint64_t(1) << 30;                  // GBWT_HIP_SCAN_PIECE: items of one launch of a prefix sum (scan.hpp: SCAN_PIECE; 1024 .. 2^30, tests lower it)
    // GBWT_HIP_WALK_MODE (0-3) / _PATHS_PER_WAVE (0-64; 0 = automatic) / _SMALL_RECORD: what gbwt_hip_workspace_tune sets, and overwrites
    uint32_t walk_mode = 0, paths_per_wave = 0, small_record = 16;
    static ExtractKnobs from_env() {
        ExtractKnobs k;
        const auto num = [](const char *name, int unset) { const char *v = std::getenv(name); return v ? std::atoi(v) : unset; };
        k.direct = num("GBWT_HIP_DIRECT", 1); k.segments = num("GBWT_HIP_SEGMENTS", 1); k.both_ends = num("GBWT_HIP_BOTH_ENDS", 1);
        k.ring_slots = num("GBWT_HIP_RING_SLOTS", -1); if (k.ring_slots != 32 && k.ring_slots != 64 && k.ring_slots != 128) k.ring_slots = -1;
        k.helper_naps = std::max(-1, num("GBWT_HIP_HELPER_NAPS", -1));
        k.xcd_map = num("GBWT_HIP_XCD_MAP", -1); k.uniform_loop = num("GBWT_HIP_UNIFORM_LOOP", -1); k.packed_blocks = num("GBWT_HIP_PACKED_BLOCKS", -1);
        k.catch_up = num("GBWT_HIP_CATCH_UP", -1);
        k.gather_reach = std::min(64, std::max(-1, num("GBWT_HIP_GATHER_REACH", -1)));
        k.sample_stride = num("GBWT_HIP_SAMPLE_STRIDE", -1);
        k.defer_total = num("GBWT_HIP_DEFER_TOTAL", 1);
        k.fused_offsets = num("GBWT_HIP_FUSED_OFFSETS", 1);
        k.all4 = num("GBWT_HIP_ALL4", 1);
        k.headroom = std::min(32, std::max(0, num("GBWT_HIP_HEADROOM", 0)));
        k.row_piece = num("GBWT_HIP_ROW_PIECE", -1); if (k.row_piece != 0 && k.row_piece != 16 && k.row_piece != 32) k.row_piece = -1;
        k.wide_addresses = std::getenv("GBWT_HIP_WIDE_ADDRESSES") != nullptr;
        k.debug = static_cast<uint32_t>(num("GBWT_HIP_DEBUG_DRY_ROWS", 0));
        k.copy_threads = static_cast<unsigned>(std::min(64, std::max(1, num("GBWT_HIP_COPY_THREADS", 8))));
        k.locate_sort_piece = static_cast<uint64_t>(std::max(1, num("GBWT_HIP_LOCATE_SORT_PIECE", 0x7FFFFFFF)));
        if (const char *v = std::getenv("GBWT_HIP_SCAN_PIECE")) k.scan_piece = std::min<uint64_t>(uint64_t(1) << 30, std::max<uint64_t>(1024, std::strtoull(v, nullptr, 10)));
        if (const int m = num("GBWT_HIP_WALK_MODE", -1); m >= 0 && m <= 3) k.walk_mode = static_cast<uint32_t>(m);
        if (const int p = num("GBWT_HIP_PATHS_PER_WAVE", -1); p >= 0 && p <= 64) k.paths_per_wave = static_cast<uint32_t>(p);
        if (const char *v = std::getenv("GBWT_HIP_SMALL_RECORD")) { const long r = std::atol(v); if (r >= 0) k.small_record = static_cast<uint32_t>(r); }
        return k;
    }
};
