// capi_fm_seeds.hip -- the C ABI of the seeds of reads (include/gbwt_hip.h, "Seeds of reads"), next to capi_fm.hip, whose
// object it shares (fm_object.hpp).  The kernels are fm_seeds.hip, the sizes and refusals fm_seed_plan.hpp; the rows of hits are filled by
// the locate kernel of fm_index.hip, their tags by the tags family (capi_tags.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "capi_internal.hpp"
#include "counted_buffer.hpp"
#include "device_common.hpp"
#include "fm_index.hpp"
#include "fm_object.hpp"
#include "fm_seed_kernels.hpp"
#include "fm_seed_plan.hpp"
#include "scan.hpp"

using namespace gbwt_hip;

namespace {

constexpr gbwt_hip_fm_seed_options DEFAULT_OPTIONS{1, GBWT_HIP_STRAND_BOTH, 0, 0, 0};

// The checks that answer before a device is touched: the reads, the options, then the object
gbwt_hip_status check_request(const gbwt_hip_fm_index *fm, const uint64_t *offsets, const void *bytes, uint64_t m, bool on_host, const gbwt_hip_fm_seed_options *&opts, bool graph,
                              const gbwt_hip_index *ix, const gbwt_hip_workspace *ws) {
    gbwt_hip_status st = fm_check_patterns(offsets, bytes, m, on_host);
    if (st != GBWT_HIP_OK) return st;
    if (!opts) opts = &DEFAULT_OPTIONS;
    st = fm_check_seed_options(*opts);
    if (st != GBWT_HIP_OK) return st;
    if (graph && opts->max_occurrences == 0) return fail(GBWT_HIP_BAD_ARGUMENT, "graph positions of seeds need max_occurrences > 0: the tags are the hits");
    return fm_check_object(fm, graph ? FM_GRAPH : opts->max_occurrences != 0 ? FM_LOCATE : FM_COUNT, ix, ws, 0);
}

}  // namespace

// The rows of a request into the object (fm_object.hpp)
gbwt_hip_status gbwt_hip::fm_seeds_compute(gbwt_hip_fm_index *fm, const uint64_t *h_offsets, const void *h_bytes, const uint64_t *d_offsets, const uint8_t *d_bytes, uint64_t m, uint64_t bytes,
                                           const gbwt_hip_fm_seed_options &opts, bool graph, const gbwt_hip_index *ix, gbwt_hip_workspace *ws) {
    gbwt_hip_fm_seed_state &st = fm->seed;
    const bool hits = opts.max_occurrences != 0;
    if (h_offsets) {
        bytes = h_offsets[m];
        if (st.memo.matches({{h_offsets, (m + 1) * sizeof(uint64_t)}, {h_bytes, bytes}},
                            {graph, opts.min_length, opts.strands, static_cast<int64_t>(opts.max_occurrences), static_cast<int64_t>(m)}))
            return GBWT_HIP_OK;
    }
    st.memo.drop();
    st.m = st.total_seeds = st.total_hits = 0;
    st.with_hits = st.with_tags = false;
    try {
        HIP_CHECK(hipSetDevice(fm->device));
        hipStream_t s = fm->stream;
        // 1. the plan: everything the search needs, sized by (reads, bytes, strands, hits) and refused before the first kernel
        const uint64_t most = fm_seed_end_slots(m, bytes, opts.strands);
        size_t free_bytes = 0, all_bytes = 0;
        HIP_CHECK(hipMemGetInfo(&free_bytes, &all_bytes));
        const FmSeedPlan plan = fm_seed_plan(m, bytes, opts.strands, hits, bytes > FM_SEED_MAX_BYTES ? 0 : scan_temp_bytes(most), free_bytes);
        if (plan.status == FmStatus::Unsupported) return fail(plan.bad_argument ? GBWT_HIP_BAD_ARGUMENT : GBWT_HIP_UNSUPPORTED, plan.message);
        if (plan.status == FmStatus::Capacity) return fail(GBWT_HIP_CAPACITY, plan.message);
        st.ev.ensure();
        CountedScratch sc;
        CountedBuf anchor_counts(sc, plan.items * sizeof(uint64_t)), anchor_offsets(sc, (plan.items + 1) * sizeof(uint64_t));
        CountedBuf anchor_start(sc, plan.anchor_slots * sizeof(uint32_t)), anchor_lo(sc, plan.anchor_slots * sizeof(uint32_t)), anchor_hi(sc, plan.anchor_slots * sizeof(uint32_t)),
            anchor_item(sc, plan.anchor_slots * sizeof(uint32_t));
        CountedBuf refined_counts(sc, plan.anchor_slots * sizeof(uint64_t)), refined_offsets(sc, (plan.anchor_slots + 1) * sizeof(uint64_t));
        CountedBuf refined_start(sc, plan.refined_slots * sizeof(uint32_t)), refined_lo(sc, plan.refined_slots * sizeof(uint32_t)), refined_hi(sc, plan.refined_slots * sizeof(uint32_t));
        CountedBuf flags(sc, plan.end_slots * sizeof(uint64_t)), rank(sc, (plan.end_slots + 1) * sizeof(uint64_t));
        CountedBuf temp(sc, plan.temp_bytes), words(sc, plan.words_bytes);
        CountedBuf hit_ranges, hit_counts;
        if (hits) {
            hit_ranges.alloc(sc, 2 * plan.seed_slots * sizeof(uint64_t));
            hit_counts.alloc(sc, plan.seed_slots * sizeof(uint64_t));
        }
        st.read_offsets.reserve((m + 1) * sizeof(uint64_t));
        if (h_offsets) {
            st.q_offsets.reserve((m + 1) * sizeof(uint64_t));
            st.q_bytes.reserve(std::max<uint64_t>(bytes, 1));
            HIP_CHECK(hipMemcpyAsync(st.q_offsets.ptr, h_offsets, (m + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            if (bytes) HIP_CHECK(hipMemcpyAsync(st.q_bytes.ptr, h_bytes, bytes, hipMemcpyHostToDevice, s));
            d_offsets = st.q_offsets.as<uint64_t>();
            d_bytes = st.q_bytes.as<uint8_t>();
        }
        uint64_t *d_words = words.as<uint64_t>();
        HIP_CHECK(hipMemsetAsync(d_words, 0, FM_SEED_WORDS * sizeof(uint64_t), s));
        HIP_CHECK(hipMemsetAsync(st.read_offsets.ptr, 0, (m + 1) * sizeof(uint64_t), s));
        SeedBatch b{};
        b.L = fm->layout;
        b.t = FmTables{fm->tables.as<uint16_t>(), reinterpret_cast<const uint32_t *>(fm->tables.as<uint16_t>() + 256)};
        b.offsets = d_offsets; b.bytes = d_bytes; b.m = m; b.total_bytes = bytes;
        b.strands = opts.strands; b.min_length = opts.min_length;
        b.items = plan.items;
        b.anchor_counts = anchor_counts.as<uint64_t>(); b.anchor_offsets = anchor_offsets.as<uint64_t>();
        b.anchor_start = anchor_start.as<uint32_t>(); b.anchor_lo = anchor_lo.as<uint32_t>(); b.anchor_hi = anchor_hi.as<uint32_t>(); b.anchor_item = anchor_item.as<uint32_t>();
        b.refined_counts = refined_counts.as<uint64_t>(); b.refined_offsets = refined_offsets.as<uint64_t>();
        b.refined_start = refined_start.as<uint32_t>(); b.refined_lo = refined_lo.as<uint32_t>(); b.refined_hi = refined_hi.as<uint32_t>();
        b.flags = flags.as<uint64_t>(); b.rank = rank.as<uint64_t>();
        b.words = d_words;
        // 2. the anchors.  The one look at the offsets comes first: only offsets that ascend inside the bytes keep the ends within the plan
        HIP_CHECK(hipEventRecord(st.ev[0], s));
        launch_seed_anchor_count(b, s);
        launch_scan(b.anchor_counts, b.anchor_offsets, b.items, temp.ptr, temp.bytes, s);
        HIP_CHECK(hipGetLastError());
        b.anchors = read_value(b.anchor_offsets + b.items, s);
        if (static_cast<uint32_t>(read_value(d_words, s)) & FM_FLAG_OFFSETS) return fail(GBWT_HIP_BAD_ARGUMENT, "pattern offsets descend or leave the pattern bytes");
        if (b.anchors > plan.anchor_slots) return fail(GBWT_HIP_DEVICE_ERROR, "more anchors than the plan of the seeds request holds");
        launch_seed_anchors(b, s);
        HIP_CHECK(hipEventRecord(st.ev[1], s));
        // 3. the ends between anchors whose starts differ
        uint64_t total_seeds = 0, total_hits = 0;
        if (b.anchors) {
            launch_seed_refine_count(b, s);
            launch_scan(b.refined_counts, b.refined_offsets, b.anchors, temp.ptr, temp.bytes, s);
            HIP_CHECK(hipGetLastError());
            b.refined = read_value(b.refined_offsets + b.anchors, s);
            if (b.refined > plan.refined_slots) return fail(GBWT_HIP_DEVICE_ERROR, "more refined ends than the plan of the seeds request holds");
            launch_seed_refine(b, s);
        }
        HIP_CHECK(hipEventRecord(st.ev[2], s));
        // 4. the seeds: a flag per end, their scan, the rows
        if (b.anchors) {
            const uint64_t ends = b.anchors + b.refined;
            launch_seed_flags(b, s);
            launch_scan(b.flags, b.rank, ends, temp.ptr, temp.bytes, s);
            HIP_CHECK(hipGetLastError());
            total_seeds = read_value(b.rank + ends, s);
            if (hits && total_seeds > plan.seed_slots) return fail(GBWT_HIP_DEVICE_ERROR, "more seeds than the plan of the seeds request holds");
            st.seeds.reserve(std::max<uint64_t>(total_seeds, 1) * sizeof(gbwt_hip_fm_seed));
            launch_seed_fill(b, st.seeds.as<gbwt_hip_fm_seed>(), st.read_offsets.as<uint64_t>(), opts.max_occurrences, hits ? hit_ranges.as<uint64_t>() : nullptr,
                             hits ? hit_counts.as<uint64_t>() : nullptr, s);
        }
        HIP_CHECK(hipEventRecord(st.ev[3], s));
        // 5. the hits: rows of the suffix array over the seeds' ranges, and their tags
        if (hits) {
            st.hit_offsets.reserve((total_seeds + 1) * sizeof(uint64_t));
            launch_scan(hit_counts.as<uint64_t>(), st.hit_offsets.as<uint64_t>(), total_seeds, temp.ptr, temp.bytes, s);
            HIP_CHECK(hipGetLastError());
            total_hits = read_value(st.hit_offsets.as<uint64_t>() + total_seeds, s);
            st.positions.reserve(std::max<uint64_t>(total_hits, 1) * sizeof(uint64_t));
            launch_fm_locate_fill(fm->sa.as<uint32_t>(), hit_ranges.as<uint64_t>(), st.hit_offsets.as<uint64_t>(), total_seeds, st.positions.as<uint64_t>(), nullptr, s);
        }
        HIP_CHECK(hipEventRecord(st.ev[4], s));
        uint64_t host_words[FM_SEED_WORDS] = {};
        HIP_CHECK(hipMemcpyAsync(host_words, d_words, sizeof(host_words), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        if (graph) {
            st.tags.reserve(std::max<uint64_t>(total_hits, 1) * sizeof(uint64_t));
            const gbwt_hip_status tagged = gbwt_hip_tags_device(ix, ws, fm->path_ids.data(), fm->path_ids.size(), st.positions.as<uint64_t>(), total_hits, st.tags.as<uint64_t>(), nullptr);
            if (tagged != GBWT_HIP_OK) return tagged;
            HIP_CHECK(hipSetDevice(fm->device));
        }
        gbwt_hip_fm_seed_info &info = st.info;
        const uint64_t requests = info.requests + 1;
        info = gbwt_hip_fm_seed_info{};
        info.requests = requests;
        info.reads = m; info.read_bytes = bytes; info.anchors = b.anchors; info.refined_ends = b.refined;
        info.steps = host_words[1]; info.seeds = total_seeds; info.hits = total_hits; info.over_max = host_words[3];
        info.planned_scratch_bytes = plan.scratch_bytes; info.peak_scratch_bytes = sc.peak;
        info.stride = plan.stride; info.strands = opts.strands;
        info.idle_share = host_words[2] ? static_cast<float>(1.0 - double(host_words[1]) / (64.0 * double(host_words[2]))) : 0.0f;
        HIP_CHECK(hipEventElapsedTime(&info.anchor_ms, st.ev[0], st.ev[1]));
        HIP_CHECK(hipEventElapsedTime(&info.refine_ms, st.ev[1], st.ev[2]));
        HIP_CHECK(hipEventElapsedTime(&info.emit_ms, st.ev[2], st.ev[3]));
        HIP_CHECK(hipEventElapsedTime(&info.hits_ms, st.ev[3], st.ev[4]));
        st.m = m; st.total_seeds = total_seeds; st.total_hits = total_hits;
        st.with_hits = hits; st.with_tags = graph;
        if (h_offsets) st.memo.store({{h_offsets, (m + 1) * sizeof(uint64_t)}, {h_bytes, bytes}},
                                     {graph, opts.min_length, opts.strands, static_cast<int64_t>(opts.max_occurrences), static_cast<int64_t>(m)});
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        (void)hipDeviceSynchronize();                    // (the scratch goes: nothing of the request may still run)
        return status_of(e, "a seeds request");
    }
}

namespace {

gbwt_hip_fm_seed_rows rows_of(const gbwt_hip_fm_index *fm) {
    const gbwt_hip_fm_seed_state &st = fm->seed;
    return gbwt_hip_fm_seed_rows{st.read_offsets.as<uint64_t>(), st.seeds.as<gbwt_hip_fm_seed>(), st.with_hits ? st.hit_offsets.as<uint64_t>() : nullptr,
                                 st.with_hits ? (st.with_tags ? st.tags : st.positions).as<uint64_t>() : nullptr, st.total_seeds, st.total_hits, st.m};
}

// The host form: offsets and totals always; seeds, hit offsets and hits when asked for and the capacities hold them
gbwt_hip_status rows_to_host(gbwt_hip_fm_index *fm, uint64_t *out_read_offsets, gbwt_hip_fm_seed *seeds, uint64_t seed_capacity, uint64_t *total_seeds, uint64_t *out_hit_offsets,
                             uint64_t *hits, uint64_t hit_capacity, uint64_t *total_hits) {
    const gbwt_hip_fm_seed_rows rows = rows_of(fm);
    *total_seeds = rows.total_seeds;
    if (total_hits) *total_hits = rows.total_hits;
    try {
        HIP_CHECK(hipSetDevice(fm->device));
        if (seeds && seed_capacity < rows.total_seeds) return fail(GBWT_HIP_CAPACITY, "seed capacity too small: the rows hold " + std::to_string(rows.total_seeds) + " seeds");
        if (hits && hit_capacity < rows.total_hits) return fail(GBWT_HIP_CAPACITY, "hit capacity too small: the rows hold " + std::to_string(rows.total_hits) + " hits");
        HIP_CHECK(hipMemcpy(out_read_offsets, rows.d_read_offsets, (rows.m + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (seeds && rows.total_seeds) HIP_CHECK(hipMemcpy(seeds, rows.d_seeds, rows.total_seeds * sizeof(gbwt_hip_fm_seed), hipMemcpyDeviceToHost));
        if (seeds && out_hit_offsets && rows.d_hit_offsets) HIP_CHECK(hipMemcpy(out_hit_offsets, rows.d_hit_offsets, (rows.total_seeds + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (hits && rows.total_hits) HIP_CHECK(hipMemcpy(hits, rows.d_hits, rows.total_hits * sizeof(uint64_t), hipMemcpyDeviceToHost));
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
}

gbwt_hip_status host_request(gbwt_hip_fm_index *fm, bool graph, const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *offsets, const void *bytes, uint64_t m,
                             const gbwt_hip_fm_seed_options *opts, uint64_t *out_read_offsets, gbwt_hip_fm_seed *seeds, uint64_t seed_capacity, uint64_t *total_seeds,
                             uint64_t *out_hit_offsets, uint64_t *hits, uint64_t hit_capacity, uint64_t *total_hits) {
    if (total_seeds) *total_seeds = 0;
    if (total_hits) *total_hits = 0;
    if (!total_seeds || !out_read_offsets) return fail(GBWT_HIP_BAD_ARGUMENT, "null total / read offsets");
    const bool wants_hits = graph || (opts && opts->max_occurrences != 0);
    if (wants_hits && !total_hits) return fail(GBWT_HIP_BAD_ARGUMENT, "null total of the hits");
    if (wants_hits && seeds && !out_hit_offsets) return fail(GBWT_HIP_BAD_ARGUMENT, "null hit offsets (one more than the seeds)");
    gbwt_hip_status st = check_request(fm, offsets, bytes, m, true, opts, graph, ix, ws);
    if (st == GBWT_HIP_OK) st = fm_seeds_compute(fm, offsets, bytes, nullptr, nullptr, m, 0, *opts, graph, ix, ws);
    if (st != GBWT_HIP_OK) return st;
    return rows_to_host(fm, out_read_offsets, seeds, seed_capacity, total_seeds, out_hit_offsets, hits, hit_capacity, total_hits);
}

gbwt_hip_status device_request(gbwt_hip_fm_index *fm, bool graph, const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *d_offsets, const void *d_bytes, uint64_t m,
                               uint64_t bytes, const gbwt_hip_fm_seed_options *opts, gbwt_hip_fm_seed_rows *out) {
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_fm_seed_rows{nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
    gbwt_hip_status st = check_request(fm, d_offsets, d_bytes, m, false, opts, graph, ix, ws);
    if (st == GBWT_HIP_OK) st = fm_seeds_compute(fm, nullptr, nullptr, d_offsets, static_cast<const uint8_t *>(d_bytes), m, bytes, *opts, graph, ix, ws);
    if (st != GBWT_HIP_OK) return st;
    *out = rows_of(fm);
    return GBWT_HIP_OK;
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_fm_last_seed_info(const gbwt_hip_fm_index *fm, gbwt_hip_fm_seed_info *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!fm || !out) return fail(GBWT_HIP_BAD_ARGUMENT, "null argument");
    *out = fm->seed.info;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_seeds(gbwt_hip_fm_index *fm, const uint64_t *offsets, const void *bytes, uint64_t m, const gbwt_hip_fm_seed_options *opts, uint64_t *out_read_offsets,
                                  gbwt_hip_fm_seed *seeds, uint64_t seed_capacity, uint64_t *total_seeds, uint64_t *out_hit_offsets, uint64_t *hits, uint64_t hit_capacity,
                                  uint64_t *total_hits) {
    GBWT_HIP_GUARD_BEGIN
    return host_request(fm, false, nullptr, nullptr, offsets, bytes, m, opts, out_read_offsets, seeds, seed_capacity, total_seeds, out_hit_offsets, hits, hit_capacity, total_hits);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_seed_graph_positions(gbwt_hip_fm_index *fm, const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *offsets, const void *bytes, uint64_t m,
                                                 const gbwt_hip_fm_seed_options *opts, uint64_t *out_read_offsets, gbwt_hip_fm_seed *seeds, uint64_t seed_capacity,
                                                 uint64_t *total_seeds, uint64_t *out_hit_offsets, uint64_t *tags, uint64_t hit_capacity, uint64_t *total_hits) {
    GBWT_HIP_GUARD_BEGIN
    return host_request(fm, true, ix, ws, offsets, bytes, m, opts, out_read_offsets, seeds, seed_capacity, total_seeds, out_hit_offsets, tags, hit_capacity, total_hits);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_seeds_device(gbwt_hip_fm_index *fm, const uint64_t *d_offsets, const void *d_bytes, uint64_t m, uint64_t bytes, const gbwt_hip_fm_seed_options *opts,
                                         gbwt_hip_fm_seed_rows *out) {
    GBWT_HIP_GUARD_BEGIN
    return device_request(fm, false, nullptr, nullptr, d_offsets, d_bytes, m, bytes, opts, out);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_seed_graph_positions_device(gbwt_hip_fm_index *fm, const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *d_offsets, const void *d_bytes,
                                                        uint64_t m, uint64_t bytes, const gbwt_hip_fm_seed_options *opts, gbwt_hip_fm_seed_rows *out) {
    GBWT_HIP_GUARD_BEGIN
    return device_request(fm, true, ix, ws, d_offsets, d_bytes, m, bytes, opts, out);
    GBWT_HIP_GUARD_END
}

}  // extern "C"
