// extract_plan.hpp -- every decision of an extraction request (capi_extract.hip: gbwt_hip_extract_part_device) as arithmetic over numbers
// the host has: plain C++, no HIP (tests/cpp/extract_plan.cpp runs it without a GPU).  The request makes an IdSummary of its ids, a
// RowsPlan before the lengths of its rows are known and a WalkPlan once the longest row is, and copies them into DeviceIndex / WalkArgs.
#pragma once

#include <algorithm>
#include <cstdint>

#include "extract_knobs.hpp"

namespace gbwt_hip {

// What the decisions read of a handle (gbwt_hip_index, handle.hpp)
struct PlanIndex {
    uint64_t sequences = 0, size = 0, records = 0;     // host.sequences, host.size, stats.records
    bool has_samples = false;                          // dev.samples != nullptr
    uint32_t max_samples = 0, sample_coarse = 1, uniform_samples = 0, uniform_len = 0;
    const uint32_t *sample_counts = nullptr;           // [n_sample_counts] samples of every sequence (none on a handle without samples)
    uint64_t n_sample_counts = 0;
    bool orientation_pairs = false, lean = false, packed_blocks = false;
};

// One pass over the ids of a request
struct IdSummary {
    bool ids_valid = true;     // every id < sequences
    uint64_t fine = 0;         // samples of all valid ids together
    uint32_t common = 0;       // the number of samples every id has, 0 where they differ (or n == 0, or an id without a sequence)
};
inline IdSummary summarize_ids(const uint64_t *seq_ids, uint64_t n, const PlanIndex &ix) {
    IdSummary s;
    bool same = true;
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t id = seq_ids[k];
        if (id >= ix.sequences) { s.ids_valid = false; continue; }
        const uint32_t count = id < ix.n_sample_counts ? ix.sample_counts[id] : 0u;
        s.fine += count;
        if (k == 0) s.common = count;
        else if (count != s.common) same = false;
    }
    if (!s.ids_valid || !same) s.common = 0;
    return s;
}

// ---- stage 1: before the lengths of the rows are known ---------------------------------------------------------------------------
struct RowsPlan {
    bool can_cut = false, parted = false;
    bool empty_part = false;   // an early part of rows that cannot be cut: n empty rows, nothing else is decided
    uint32_t stride = 1;       // DeviceIndex::sample_stride
    uint32_t common = 0;       // samples of every row, 0 = they differ (or it is not known without the device)
    bool all_valid = false, fused_offsets = false, defer = false;
    uint64_t total = 0;        // all_valid: the total; defer: the capacity, which stands in until the wait at the end; else the device says
    uint32_t max_len = 0;      // all_valid: the length of every row; defer: 1 (a row may have nodes: the walk is a segmented one)
};
inline RowsPlan plan_rows(const ExtractKnobs &knobs, const PlanIndex &ix, const IdSummary &ids, uint64_t n, uint32_t part, uint32_t parts, uint64_t capacity) {
    RowsPlan p;
    // ONE PART OF EVERY ROW (gbwt_hip_extract_part_device; round 4): rows are cut where their walkers start anyway, at sequence samples.
    // An index without samples (GBWT_HIP_SAMPLE_INTERVAL=0, GBWT_HIP_SEGMENTS=0) cannot cut: the last part is the whole row there.
    p.can_cut = ix.has_samples && ix.max_samples > 0 && knobs.segments != 0 && n <= 0x7FFFFFFFull;
    if (parts > 1 && !p.can_cut && part + 1 < parts) { p.empty_part = true; return p; }
    p.parted = parts > 1 && p.can_cut;
    // a walker per `stride` samples of a row (fine samples, gbwt_hip_open): about 2.9 million walkers for the biggest batches, no segments
    // shorter than two samples unless the batch is so small that it needs every walker it can get
    p.stride = static_cast<uint32_t>(std::max(1, knobs.sample_stride));
    if (knobs.sample_stride < 0 && p.can_cut && ix.sample_coarse > 1) {
        const uint64_t fine = p.parted ? ids.fine / parts : ids.fine;
        const uint64_t want = (fine + 1450000) / 2900000;
        p.stride = static_cast<uint32_t>(std::min<uint64_t>(2 * ix.sample_coarse, std::max<uint64_t>(want, fine >= 524288 ? 2 : 1)));
    }
    // every row of one, known length (the headline's shape, config 5): no table of offsets is needed to walk, and the walk kernel
    // writes the one the caller gets (WalkArgs::uniform_len) -- nothing is launched in front of it
    p.all_valid = ids.ids_valid && ix.uniform_len != 0 && !p.parted;
    p.fused_offsets = p.all_valid && knobs.fused_offsets != 0;
    // every row of the batch with the same number of samples (the forward sequences of haplotypes over one reference frame: the
    // headline's shape): walker w = segment * n + row, no order to compute -- and nothing the host has to ask the device for
    p.common = ix.uniform_samples;
    if (p.can_cut && ids.ids_valid && p.common == 0 && n != 0) p.common = ids.common;
    // ROWS SIZED AFTER THE LAUNCH (round 4): a request that knows its walkers without the device (above) and finds rows in its
    // workspace does not wait for the total of its row lengths either -- 20 us of a round trip in front of a walk of 0.6 ms: the walk
    // is launched into the rows that are there with their size as `capacity`, every workgroup looks at offsets[n] first, and
    // if the rows were too small (the first request of its size) the host makes them and launches again.  One host wait per request.
    p.defer = knobs.defer_total != 0 && !p.all_valid && p.can_cut && ids.ids_valid && p.common != 0 && capacity != 0;
    if (p.all_valid) {
        // every row has the same, known length: total and extremes without a round trip to the device
        p.total = n * static_cast<uint64_t>(ix.uniform_len);
        p.max_len = ix.uniform_len;
    } else if (p.defer) {
        p.total = capacity;
        p.max_len = 1;
    }
    return p;
}

// ---- stage 2: once the longest row is known ---------------------------------------------------------------------------------------
struct WalkPlan {
    bool segmented = false;
    bool refused = false;          // a lean handle asked for walkers that do not start from sequence samples: nothing is launched
    bool same_segments = false;    // every row has every segment: walker w = segment * n + row
    bool needs_order = false;      // rows with different numbers of segments: the device computes the walker order, and `walkers`
    uint32_t segments = 0;
    uint64_t walkers = 0;          // (needs_order: until the device has counted them, one per row or per end of a row)
    uint32_t paths_per_wave = 0, ring_slots = 0, helper_naps = 0, xcd_map = 0, uniform_loop = 0, catch_up = 0, gather_reach = 0, all4 = 0, headroom = 0,
             packed_blocks = 0, row_piece = 0, both_ends = 0, wide_addresses = 0, debug = 0;
    uint64_t capacity = 0;
    uint32_t uniform_len = 0;      // > 0: the walk kernel writes the offsets itself (fused_offsets)
};
inline WalkPlan plan_walk(const ExtractKnobs &knobs, const PlanIndex &ix, const RowsPlan &rows, bool ids_valid, uint64_t n, uint32_t part, uint32_t parts, uint32_t max_len,
                          uint64_t capacity) {
    WalkPlan a;
    const uint32_t stride = rows.stride;
    // many walkers per row when the index has sequence samples (GBWT_HIP_SEGMENTS=0: one walker per end instead)
    a.segmented = ix.has_samples && max_len > 0 && n <= 0x7FFFFFFFull && ix.max_samples > 0 && knobs.segments != 0;   // (the walker order sorts 32-bit row numbers)
    // A lean handle (open_common) has given back the raw descriptors that a walker without a sample to start from reads when it arrives
    // on its first record (walk_loops.hpp: arrive): whole-row walkers -- GBWT_HIP_SEGMENTS=0, more than 2^31 - 1 rows -- are refused
    // there like the pool-output modes, before anything is launched (rows of no nodes have no walker and are served).
    if (ix.lean && !a.segmented && max_len > 0) { a.refused = true; return a; }
    // the samples lie where the sequences pass checkpoint records, so the number of segments of a row comes from its samples, not from its length
    a.segments = a.segmented ? (ix.max_samples + stride - 1) / stride : 0u;
    if (rows.parted) a.segments = a.segments / parts + 1;          // (no row has more segments in one part)
    a.walkers = ix.orientation_pairs ? 2 * n : n;
    a.same_segments = a.segmented && ids_valid && rows.common != 0;
    a.needs_order = a.segmented && !a.same_segments;   // walkers segment by segment over the rows that have the segment (rows sorted by their segment count)
    if (a.same_segments) {
        a.segments = (rows.common + stride - 1) / stride;
        if (rows.parted) a.segments = static_cast<uint32_t>(uint64_t(a.segments) * (part + 1) / parts - uint64_t(a.segments) * part / parts);   // (device_index.hpp: row_segments)
        a.walkers = static_cast<uint64_t>(a.segments) * n;   // every row has every segment: no order to compute
    }
    // many walkers: the walk is a throughput problem, full waves; few walkers (one or two per row): latency, and
    // about one workgroup per four SIMDs keeps every workgroup resident (32 KB of LDS each)
    a.paths_per_wave = knobs.paths_per_wave ? knobs.paths_per_wave
                       : a.segmented ? 64u : static_cast<uint32_t>(std::min<uint64_t>(64, std::max<uint64_t>(16, (a.walkers + 1023) / 1024)));
    a.wide_addresses = knobs.wide_addresses ? 1u : 0u;
    a.ring_slots = knobs.ring_slots > 0 ? static_cast<uint32_t>(knobs.ring_slots) : (a.segmented ? 64u : 128u);   // many walkers: smaller rings, more workgroups per CU (7.4 vs 8.1 ms on the headline)
    // many walkers per CU: a helper that polls less leaves more issue slots and LDS cycles to them (6 until the packed half-blocks
    // made the walkers faster: 3 / 4 / 6 / 8 / 10 naps = 4.30 / 4.31 / 4.35 / 4.42 / 4.51 ms)
    a.helper_naps = knobs.helper_naps >= 0 ? static_cast<uint32_t>(knobs.helper_naps) : (a.segmented ? 4u : 1u);
    a.xcd_map = knobs.xcd_map >= 0 ? (knobs.xcd_map ? 1u : 0u) : (a.segmented ? 1u : 0u);
    a.uniform_loop = knobs.uniform_loop >= 0 ? (knobs.uniform_loop ? 1u : 0u) : 1u;
    // without packed half-blocks every wave starts on the full-width loops (the packed ones load before they look at GATHER_OK)
    a.packed_blocks = (ix.packed_blocks && knobs.packed_blocks != 0) ? 1u : 0u;
    // (2: single steps on the two-step descriptors + packed half-blocks: what a lean handle has -- and GBWT_HIP_CATCH_UP=2 on any)
    a.catch_up = knobs.catch_up >= 0 ? static_cast<uint32_t>(std::min(knobs.catch_up, 2)) : 1u;
    if (ix.lean && a.catch_up == 1u) a.catch_up = 2u;
    if (a.catch_up == 2u && !a.packed_blocks) a.catch_up = ix.lean ? 0u : 1u;
    // look-ahead in mixed waves where few rows pass a record (fewer than 512 BWT positions per record on average: config 4 has 52, the
    // headline 3 300 -- there seventy waves share every line and the extra load of the gather loop costs what it saves, round 2)
    a.gather_reach = knobs.gather_reach >= 0 ? static_cast<uint32_t>(knobs.gather_reach) : (ix.records != 0 && ix.size / ix.records < 512 ? 1u : 0u);
    a.all4 = knobs.all4 != 0 ? 1u : 0u;
    a.headroom = static_cast<uint32_t>(knobs.headroom);
    a.row_piece = knobs.row_piece >= 0 ? static_cast<uint32_t>(knobs.row_piece) : 32u;
    if (a.ring_slots < 2 * a.row_piece) a.ring_slots = 2 * a.row_piece;   // a walker stops staging 8 slots before its ring is full: a ring of one piece would never hold one
    // GBWT_HIP_HEADROOM: the walkers wait while more than ring - headroom nodes are pending, the cooperative helper moves whole pieces only:
    // a headroom above ring - piece would leave a row with fewer than a piece pending and its walker waiting for ever
    if (a.headroom > a.ring_slots - std::max(a.row_piece, 1u)) a.headroom = a.ring_slots - std::max(a.row_piece, 1u);
    a.debug = knobs.debug;                               // timing experiments only, see WalkArgs::debug
    a.both_ends = (ix.orientation_pairs && knobs.both_ends != 0) ? 1u : 0u;
    a.capacity = rows.defer ? capacity : 0;
    a.uniform_len = rows.fused_offsets ? ix.uniform_len : 0u;
    return a;
}

// ---- the pool-output walk (no sequence lengths, GBWT_HIP_DIRECT=0, a tuned walk mode) ------------------------------------------------
// Pool bound for distinct ids: all sequences together hold size - sequences nodes (src/gbwt.rs:108-122), and every path wastes less
// than one block of `block_nodes` (kernels.hpp: POOL_BLOCK_NODES).
inline uint64_t plan_pool_blocks(const PlanIndex &ix, uint64_t n, uint32_t block_nodes) {
    const uint64_t all_nodes = ix.size >= ix.sequences ? ix.size - ix.sequences : 0;
    return all_nodes / block_nodes + n + 1;
}
// automatic: the walk is latency-bound and every lane of a wave runs the same instructions whether it owns a
// sequence or not, so owners per wave cost nothing; at least 32 measured best (fewer, fuller waves keep the walks
// of an XCD closer together, which is what the look-ahead relies on), more only when there are > 32k sequences
inline uint32_t plan_pool_paths_per_wave(const ExtractKnobs &knobs, uint64_t n) {
    return knobs.paths_per_wave ? knobs.paths_per_wave : static_cast<uint32_t>(std::min<uint64_t>(64, std::max<uint64_t>(32, (n + 1023) / 1024)));
}

}  // namespace gbwt_hip
