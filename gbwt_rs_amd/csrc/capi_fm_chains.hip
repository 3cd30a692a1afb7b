// capi_fm_chains.hip -- the C ABI of the chains of seeds (include/gbwt_hip.h, "Chains of seeds"), next to capi_fm_seeds.hip, whose
// request it starts with (fm_object.hpp: fm_seeds_compute).  The kernels are fm_chains.hip, the sizes and refusals fm_chain_plan.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "capi_internal.hpp"
#include "counted_buffer.hpp"
#include "device_common.hpp"
#include "fm_chain_kernels.hpp"
#include "fm_chain_plan.hpp"
#include "fm_object.hpp"
#include "fm_seeds.hpp"
#include "scan.hpp"

using namespace gbwt_hip;

namespace {

constexpr gbwt_hip_fm_seed_options DEFAULT_SEED_OPTIONS{1, GBWT_HIP_STRAND_BOTH, 0, 0, 0};
constexpr gbwt_hip_fm_chain_options DEFAULT_CHAIN_OPTIONS{0, 0, 0, 0, 0, 0, 0};

// The checks that answer before a device is touched: the reads, the seed options, the chain options, then the object
gbwt_hip_status check_request(const gbwt_hip_fm_index *fm, const uint64_t *offsets, const void *bytes, uint64_t m, bool on_host, const gbwt_hip_fm_seed_options *&seed_opts,
                              const gbwt_hip_fm_chain_options *&chain_opts) {
    const gbwt_hip_status st = fm_check_chain_request(offsets, bytes, m, on_host, seed_opts, chain_opts);
    return st != GBWT_HIP_OK ? st : fm_check_object(fm, FM_LOCATE, nullptr, nullptr, 0);
}

}  // namespace

gbwt_hip_status gbwt_hip::fm_check_chain_request(const uint64_t *offsets, const void *bytes, uint64_t m, bool on_host, const gbwt_hip_fm_seed_options *&seed_opts,
                                                 const gbwt_hip_fm_chain_options *&chain_opts) {
    gbwt_hip_status st = fm_check_patterns(offsets, bytes, m, on_host);
    if (st != GBWT_HIP_OK) return st;
    if (!seed_opts) seed_opts = &DEFAULT_SEED_OPTIONS;
    st = fm_check_seed_options(*seed_opts);
    if (st != GBWT_HIP_OK) return st;
    if (seed_opts->max_occurrences == 0) return fail(GBWT_HIP_BAD_ARGUMENT, "chains need hits: max_occurrences of the seed options must be > 0");
    if (!chain_opts) chain_opts = &DEFAULT_CHAIN_OPTIONS;
    if (chain_opts->flags != 0 || chain_opts->reserved != 0) return fail(GBWT_HIP_BAD_ARGUMENT, "flags and reserved of the chain options must be 0");
    if (chain_opts->max_gap > FM_CHAIN_MAX_OPTION || chain_opts->max_skew > FM_CHAIN_MAX_OPTION) return fail(GBWT_HIP_BAD_ARGUMENT, "max_gap and max_skew: at most 2^31 - 1");
    const FmChainParams P = fm_chain_params(chain_opts->max_gap, chain_opts->max_skew, chain_opts->gap_cost, chain_opts->min_score);
    if (uint64_t(P.gap_cost) * P.max_skew > FM_CHAIN_MAX_OPTION) return fail(GBWT_HIP_BAD_ARGUMENT, "gap_cost x max_skew must stay below 2^31");
    return GBWT_HIP_OK;
}

namespace {

// The chains of the seeds rows the object holds, into its chains state
gbwt_hip_status chains_of_seeds(gbwt_hip_fm_index *fm, const gbwt_hip_fm_seed_options &seed_opts, const gbwt_hip_fm_chain_options &chain_opts, float seeds_ms) {
    const gbwt_hip_fm_seed_state &seed = fm->seed;
    gbwt_hip_fm_chain_state &st = fm->chain;
    st.m = st.total_chains = st.total_matches = 0;
    try {
        HIP_CHECK(hipSetDevice(fm->device));
        hipStream_t s = fm->stream;
        const uint64_t m = seed.m, hits = seed.total_hits, ns = fm_strand_count(seed_opts.strands), items = m * ns;
        // 1. the plan: a function of (hits, items), refused before the first chaining kernel
        size_t free_bytes = 0, all_bytes = 0;
        HIP_CHECK(hipMemGetInfo(&free_bytes, &all_bytes));
        const bool fits = hits <= FM_CHAIN_MAX_HITS;
        size_t sort_bytes = 0;
        if (fits) HIP_CHECK(chain_sort_temp_bytes(hits, items, sort_bytes));
        const uint64_t temp_bytes = fits ? std::max<uint64_t>(sort_bytes, scan_temp_bytes(std::max(hits, items) + 1)) : 0;
        const FmChainPlan plan = fm_chain_plan(hits, items, temp_bytes, free_bytes);
        if (plan.status == FmStatus::Unsupported) return fail(GBWT_HIP_UNSUPPORTED, plan.message);
        if (plan.status == FmStatus::Capacity) return fail(GBWT_HIP_CAPACITY, plan.message);
        st.ev.ensure();
        CountedScratch sc;
        CountedBuf counts(sc, items * sizeof(uint64_t)), match_offsets(sc, (items + 1) * sizeof(uint64_t)), hit_first(sc, (items + 1) * sizeof(uint64_t));
        CountedBuf key_a(sc, hits * sizeof(uint64_t)), val_a(sc, hits * sizeof(uint64_t)), key_b(sc, hits * sizeof(uint64_t)), val_b(sc, hits * sizeof(uint64_t));
        CountedBuf y(sc, hits * sizeof(uint32_t)), x(sc, hits * sizeof(uint32_t)), w(sc, hits * sizeof(uint32_t)), low(sc, hits * sizeof(uint32_t)), seg(sc, hits * sizeof(uint32_t)),
            f(sc, hits * sizeof(uint32_t)), pred(sc, hits * sizeof(uint32_t));
        CountedBuf used(sc, hits), member_slot(sc, hits * sizeof(uint32_t)), member_pos(sc, hits * sizeof(uint32_t)), slot_score(sc, hits * sizeof(uint32_t)),
            slot_tail(sc, hits * sizeof(uint32_t));
        CountedBuf flags(sc, hits * sizeof(uint64_t)), rank(sc, (hits + 1) * sizeof(uint64_t)), members(sc, hits * sizeof(uint64_t)), member_rank(sc, (hits + 1) * sizeof(uint64_t));
        CountedBuf temp(sc, plan.temp_bytes), words(sc, plan.words_bytes);
        ChainBatch b{};
        b.seed_read_offsets = seed.read_offsets.as<uint64_t>(); b.seeds = seed.seeds.as<gbwt_hip_fm_seed>();
        b.hit_offsets = seed.hit_offsets.as<uint64_t>(); b.positions = seed.positions.as<uint64_t>();
        b.m = m; b.total_seeds = seed.total_seeds; b.total_hits = hits;
        b.strands = seed_opts.strands; b.ns = static_cast<uint32_t>(ns);
        b.path_offsets = fm->index ? fm->path_offsets.as<uint64_t>() : nullptr;
        b.n_paths = fm->path_ids.size();
        b.P = fm_chain_params(chain_opts.max_gap, chain_opts.max_skew, chain_opts.gap_cost, chain_opts.min_score);
        b.max_matches = chain_opts.max_matches;
        b.items = items;
        b.counts = counts.as<uint64_t>(); b.match_offsets = match_offsets.as<uint64_t>(); b.hit_first = hit_first.as<uint64_t>();
        b.key_a = key_a.as<uint64_t>(); b.val_a = val_a.as<uint64_t>(); b.key_b = key_b.as<uint64_t>(); b.val_b = val_b.as<uint64_t>();
        b.y = y.as<uint32_t>(); b.x = x.as<uint32_t>(); b.w = w.as<uint32_t>(); b.low = low.as<uint32_t>(); b.seg = seg.as<uint32_t>(); b.f = f.as<uint32_t>(); b.pred = pred.as<uint32_t>();
        b.used = used.as<uint8_t>();
        b.member_slot = member_slot.as<uint32_t>(); b.member_pos = member_pos.as<uint32_t>(); b.slot_score = slot_score.as<uint32_t>(); b.slot_tail = slot_tail.as<uint32_t>();
        b.flags = flags.as<uint64_t>(); b.rank = rank.as<uint64_t>(); b.members = members.as<uint64_t>(); b.member_rank = member_rank.as<uint64_t>();
        b.words = words.as<uint64_t>();
        HIP_CHECK(hipMemsetAsync(b.words, 0, FM_CHAIN_WORDS * sizeof(uint64_t), s));
        HIP_CHECK(hipMemsetAsync(b.used, 0, std::max<uint64_t>(hits, 1), s));
        // 2. the matches of every item, in seed and hit order
        HIP_CHECK(hipEventRecord(st.ev[0], s));
        launch_chain_item_counts(b, s);
        launch_scan(b.counts, b.match_offsets, items, temp.ptr, temp.bytes, s);
        HIP_CHECK(hipGetLastError());
        b.matches = read_value(b.match_offsets + items, s);
        if (b.matches > hits) return fail(GBWT_HIP_DEVICE_ERROR, "more matches than the seeds request has hits");
        launch_chain_expand(b, s);
        HIP_CHECK(hipEventRecord(st.ev[1], s));
        // 3. by (item, y, x); 4. f and pred; 5. the visiting order, the walks, the rows
        HIP_CHECK(launch_chain_sort_matches(b, temp.ptr, temp.bytes, s));
        HIP_CHECK(hipEventRecord(st.ev[2], s));
        launch_chain_dp(b, s);
        HIP_CHECK(hipEventRecord(st.ev[3], s));
        HIP_CHECK(launch_chain_sort_visits(b, temp.ptr, temp.bytes, s));
        launch_chain_peel(b, s);
        launch_scan(b.flags, b.rank, b.matches, temp.ptr, temp.bytes, s);
        launch_scan(b.members, b.member_rank, b.matches, temp.ptr, temp.bytes, s);
        HIP_CHECK(hipGetLastError());
        const uint64_t total_chains = read_value(b.rank + b.matches, s), total_members = read_value(b.member_rank + b.matches, s);
        HIP_CHECK(hipEventRecord(st.ev[4], s));
        st.read_offsets.reserve((m + 1) * sizeof(uint64_t));
        st.chains.reserve(std::max<uint64_t>(total_chains, 1) * sizeof(gbwt_hip_fm_chain));
        st.match_offsets.reserve((total_chains + 1) * sizeof(uint64_t));
        st.matches.reserve(std::max<uint64_t>(total_members, 1) * sizeof(gbwt_hip_fm_chain_match));
        launch_chain_fill(b, total_chains, st.read_offsets.as<uint64_t>(), st.chains.as<gbwt_hip_fm_chain>(), st.match_offsets.as<uint64_t>(), st.matches.as<gbwt_hip_fm_chain_match>(), s);
        HIP_CHECK(hipEventRecord(st.ev[5], s));
        uint64_t host_words[FM_CHAIN_WORDS] = {};
        HIP_CHECK(hipMemcpyAsync(host_words, b.words, sizeof(host_words), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        gbwt_hip_fm_chain_info &info = st.info;
        const uint64_t requests = info.requests + 1;
        info = gbwt_hip_fm_chain_info{};
        info.requests = requests;
        info.items = items; info.matches = b.matches; info.skipped_items = host_words[0]; info.pairs = host_words[1];
        info.chains = total_chains; info.chain_matches = total_members;
        info.planned_scratch_bytes = plan.scratch_bytes; info.peak_scratch_bytes = sc.peak;
        info.seeds_ms = seeds_ms;
        HIP_CHECK(hipEventElapsedTime(&info.expand_ms, st.ev[0], st.ev[1]));
        HIP_CHECK(hipEventElapsedTime(&info.sort_ms, st.ev[1], st.ev[2]));
        HIP_CHECK(hipEventElapsedTime(&info.dp_ms, st.ev[2], st.ev[3]));
        HIP_CHECK(hipEventElapsedTime(&info.peel_ms, st.ev[3], st.ev[4]));
        HIP_CHECK(hipEventElapsedTime(&info.fill_ms, st.ev[4], st.ev[5]));
        st.m = m; st.total_chains = total_chains; st.total_matches = total_members;
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        (void)hipDeviceSynchronize();                    // (the scratch goes: nothing of the request may still run)
        return status_of(e, "a chains request");
    }
}

}  // namespace

// A seeds request with hits as text positions through the object's seeds state and memo, then the chaining.  Exactly one of h_offsets / d_offsets.
gbwt_hip_status gbwt_hip::fm_chains_compute(gbwt_hip_fm_index *fm, const uint64_t *h_offsets, const void *h_bytes, const uint64_t *d_offsets, const uint8_t *d_bytes, uint64_t m,
                                            uint64_t bytes, const gbwt_hip_fm_seed_options &seed_opts, const gbwt_hip_fm_chain_options &chain_opts) {
    gbwt_hip_fm_chain_state &st = fm->chain;
    const std::initializer_list<int64_t> params = {seed_opts.min_length, seed_opts.strands, static_cast<int64_t>(seed_opts.max_occurrences), static_cast<int64_t>(m),
                                                   chain_opts.max_gap, chain_opts.max_skew, chain_opts.gap_cost, chain_opts.min_score, static_cast<int64_t>(chain_opts.max_matches)};
    if (h_offsets && st.memo.matches({{h_offsets, (m + 1) * sizeof(uint64_t)}, {h_bytes, h_offsets[m]}}, params)) return GBWT_HIP_OK;
    st.memo.drop();
    const uint64_t seed_requests = fm->seed.info.requests;
    gbwt_hip_status status = fm_seeds_compute(fm, h_offsets, h_bytes, d_offsets, d_bytes, m, bytes, seed_opts, false, nullptr, nullptr);
    if (status != GBWT_HIP_OK) return status;
    const gbwt_hip_fm_seed_info &si = fm->seed.info;
    status = chains_of_seeds(fm, seed_opts, chain_opts, si.requests != seed_requests ? si.anchor_ms + si.refine_ms + si.emit_ms + si.hits_ms : 0.0f);
    if (status != GBWT_HIP_OK) return status;
    if (h_offsets) st.memo.store({{h_offsets, (m + 1) * sizeof(uint64_t)}, {h_bytes, h_offsets[m]}}, params);
    return GBWT_HIP_OK;
}

namespace {

gbwt_hip_fm_chain_rows rows_of(const gbwt_hip_fm_index *fm) {
    const gbwt_hip_fm_chain_state &st = fm->chain;
    return gbwt_hip_fm_chain_rows{st.read_offsets.as<uint64_t>(), st.chains.as<gbwt_hip_fm_chain>(), st.match_offsets.as<uint64_t>(), st.matches.as<gbwt_hip_fm_chain_match>(),
                                  st.total_chains, st.total_matches, st.m};
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_fm_last_chain_info(const gbwt_hip_fm_index *fm, gbwt_hip_fm_chain_info *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!fm || !out) return fail(GBWT_HIP_BAD_ARGUMENT, "null argument");
    *out = fm->chain.info;
    out->tile_matches = FM_CHAIN_TILE;
    out->path_offset_bytes = fm->index ? fm->path_offsets.bytes : 0;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_chains(gbwt_hip_fm_index *fm, const uint64_t *offsets, const void *bytes, uint64_t m, const gbwt_hip_fm_seed_options *seed_opts,
                                   const gbwt_hip_fm_chain_options *chain_opts, uint64_t *out_read_offsets, gbwt_hip_fm_chain *chains, uint64_t chain_capacity, uint64_t *total_chains,
                                   uint64_t *out_match_offsets, gbwt_hip_fm_chain_match *matches, uint64_t match_capacity, uint64_t *total_matches) {
    GBWT_HIP_GUARD_BEGIN
    if (total_chains) *total_chains = 0;
    if (total_matches) *total_matches = 0;
    if (!total_chains || !total_matches || !out_read_offsets) return fail(GBWT_HIP_BAD_ARGUMENT, "null totals / read offsets");
    if (chains && !out_match_offsets) return fail(GBWT_HIP_BAD_ARGUMENT, "null match offsets (one more than the chains)");
    gbwt_hip_status st = check_request(fm, offsets, bytes, m, true, seed_opts, chain_opts);
    if (st == GBWT_HIP_OK) st = fm_chains_compute(fm, offsets, bytes, nullptr, nullptr, m, 0, *seed_opts, *chain_opts);
    if (st != GBWT_HIP_OK) return st;
    const gbwt_hip_fm_chain_rows rows = rows_of(fm);
    *total_chains = rows.total_chains;
    *total_matches = rows.total_matches;
    try {
        HIP_CHECK(hipSetDevice(fm->device));
        if (chains && chain_capacity < rows.total_chains) return fail(GBWT_HIP_CAPACITY, "chain capacity too small: the rows hold " + std::to_string(rows.total_chains) + " chains");
        if (matches && match_capacity < rows.total_matches) return fail(GBWT_HIP_CAPACITY, "match capacity too small: the rows hold " + std::to_string(rows.total_matches) + " matches");
        HIP_CHECK(hipMemcpy(out_read_offsets, rows.d_read_offsets, (rows.m + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (chains && rows.total_chains) HIP_CHECK(hipMemcpy(chains, rows.d_chains, rows.total_chains * sizeof(gbwt_hip_fm_chain), hipMemcpyDeviceToHost));
        if (chains) HIP_CHECK(hipMemcpy(out_match_offsets, rows.d_match_offsets, (rows.total_chains + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (matches && rows.total_matches) HIP_CHECK(hipMemcpy(matches, rows.d_matches, rows.total_matches * sizeof(gbwt_hip_fm_chain_match), hipMemcpyDeviceToHost));
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_chains_device(gbwt_hip_fm_index *fm, const uint64_t *d_offsets, const void *d_bytes, uint64_t m, uint64_t bytes, const gbwt_hip_fm_seed_options *seed_opts,
                                          const gbwt_hip_fm_chain_options *chain_opts, gbwt_hip_fm_chain_rows *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_fm_chain_rows{nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
    gbwt_hip_status st = check_request(fm, d_offsets, d_bytes, m, false, seed_opts, chain_opts);
    if (st == GBWT_HIP_OK) st = fm_chains_compute(fm, nullptr, nullptr, d_offsets, static_cast<const uint8_t *>(d_bytes), m, bytes, *seed_opts, *chain_opts);
    if (st != GBWT_HIP_OK) return st;
    *out = rows_of(fm);
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

}  // extern "C"
