// capi_fm_align.hip -- the C ABI of the alignments of chains (include/gbwt_hip.h, "Alignments of chains"), next to
// capi_fm_chains.hip, whose request it starts with (fm_object.hpp: fm_chains_compute), and the calls that give the object its text.  The
// kernels are fm_align.hip, the sizes and refusals fm_align_plan.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "capi_internal.hpp"
#include "counted_buffer.hpp"
#include "device_common.hpp"
#include "fm_align_kernels.hpp"
#include "fm_align_plan.hpp"
#include "fm_index.hpp"
#include "fm_object.hpp"
#include "fm_plan.hpp"
#include "fm_seeds.hpp"
#include "scan.hpp"

using namespace gbwt_hip;

namespace {

constexpr gbwt_hip_fm_align_options DEFAULT_ALIGN_OPTIONS{FM_ALIGN_DEFAULT_BAND, FM_ALIGN_DEFAULT_WIDTH, 0, 0, 0};

// The checks that answer before a device is touched: the reads, the seed options, the chain options, the align options, then the object
gbwt_hip_status check_request(const gbwt_hip_fm_index *fm, const uint64_t *offsets, const void *bytes, uint64_t m, bool on_host, const gbwt_hip_fm_seed_options *&seed_opts,
                              const gbwt_hip_fm_chain_options *&chain_opts, const gbwt_hip_fm_align_options *&align_opts) {
    gbwt_hip_status st = fm_check_chain_request(offsets, bytes, m, on_host, seed_opts, chain_opts);
    if (st != GBWT_HIP_OK) return st;
    if (!align_opts) align_opts = &DEFAULT_ALIGN_OPTIONS;
    if (align_opts->flags != 0 || align_opts->reserved != 0) return fail(GBWT_HIP_BAD_ARGUMENT, "flags and reserved of the align options must be 0");
    if (align_opts->max_width > FM_ALIGN_MAX_WIDTH || align_opts->band > FM_ALIGN_MAX_WIDTH)
        return fail(GBWT_HIP_BAD_ARGUMENT, "max_width and band of the align options: at most " + std::to_string(FM_ALIGN_MAX_WIDTH));
    st = fm_check_object(fm, FM_LOCATE, nullptr, nullptr, 0);
    if (st != GBWT_HIP_OK) return st;
    if (!fm->has_text) return fail(GBWT_HIP_UNSUPPORTED, "the FM-index keeps no text to align against: give it one with gbwt_hip_fm_set_text or gbwt_hip_fm_keep_path_text");
    return GBWT_HIP_OK;
}

// The text d_text[0, n) on stream s into the object, if its byte histogram is that of the index
gbwt_hip_status keep_text(gbwt_hip_fm_index *fm, const uint8_t *d_text, uint64_t n, hipStream_t s) {
    DeviceBuffer histogram;
    histogram.reserve(FM_HISTOGRAM_BYTES);
    std::vector<uint64_t> hist(256, 0);
    struct Tables { uint16_t code[256]; uint32_t C[256]; } tables{};
    static_assert(sizeof(Tables) == FM_TABLE_BYTES, "the tables as fm_plan.hpp counts them");
    HIP_CHECK(hipMemsetAsync(histogram.ptr, 0, FM_HISTOGRAM_BYTES, s));
    launch_fm_histogram(d_text, n, histogram.as<uint64_t>(), s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(hist.data(), histogram.ptr, FM_HISTOGRAM_BYTES, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&tables, fm->tables.ptr, sizeof(tables), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    uint64_t smaller = 0;
    for (int b = 0; b < 256; b++) {
        const bool absent = tables.code[b] == FM_ABSENT;
        if (absent != (hist[b] == 0) || (!absent && tables.C[tables.code[b]] != smaller))
            return fail(GBWT_HIP_INVALID_DATA, "the text is not the one the FM-index was built from: byte " + std::to_string(b) + " occurs " + std::to_string(hist[b]) + " times in it");
        smaller += hist[b];
    }
    fm->has_text = false;
    fm->align.memo.drop();                               // (the rows of an alignments request answer for the text they read)
    fm->text.reserve(std::max<uint64_t>(n, 1));
    if (n) HIP_CHECK(hipMemcpyAsync(fm->text.ptr, d_text, n, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    fm->has_text = true;
    return GBWT_HIP_OK;
}

// The alignments of the chains rows the object holds, into its align state.  d_offsets / d_bytes: the reads of the request in HBM
gbwt_hip_status align_chains(gbwt_hip_fm_index *fm, const uint64_t *d_offsets, const uint8_t *d_bytes, const gbwt_hip_fm_seed_options &seed_opts,
                             const gbwt_hip_fm_align_options &align_opts, float chains_ms) {
    const gbwt_hip_fm_chain_state &chain = fm->chain;
    gbwt_hip_fm_align_state &st = fm->align;
    st.m = st.total_alignments = st.total_cigars = 0;
    try {
        HIP_CHECK(hipSetDevice(fm->device));
        hipStream_t s = fm->stream;
        const uint64_t m = chain.m, ns = fm_strand_count(seed_opts.strands), items = m * ns;
        st.ev.ensure();
        CountedScratch sc;
        // 1. the selection: the considered chains of every item, then the band, the bounds and the sizes of each
        CountedBuf item_counts(sc, items * sizeof(uint64_t)), item_offsets(sc, (items + 1) * sizeof(uint64_t)), item_first(sc, items * sizeof(uint64_t));
        CountedBuf words(sc, FM_ALIGN_WORDS * sizeof(uint64_t));
        const uint64_t item_temp = scan_temp_bytes(items + 1);
        CountedBuf temp(sc, item_temp);
        AlignBatch b{};
        b.q_offsets = d_offsets; b.q_bytes = d_bytes;
        b.chain_read_offsets = chain.read_offsets.as<uint64_t>(); b.chains = chain.chains.as<gbwt_hip_fm_chain>();
        b.chain_match_offsets = chain.match_offsets.as<uint64_t>(); b.matches = chain.matches.as<gbwt_hip_fm_chain_match>();
        b.m = m; b.strands = seed_opts.strands; b.ns = static_cast<uint32_t>(ns);
        b.text = fm->text.as<uint8_t>(); b.n = fm->n;
        b.path_offsets = fm->index ? fm->path_offsets.as<uint64_t>() : nullptr;
        b.n_paths = fm->path_ids.size();
        b.band = align_opts.band; b.max_width = fm_align_max_width(align_opts.max_width); b.max_alignments = align_opts.max_alignments;
        b.items = items;
        b.item_counts = item_counts.as<uint64_t>(); b.item_offsets = item_offsets.as<uint64_t>(); b.item_first = item_first.as<uint64_t>();
        b.words = words.as<uint64_t>();
        HIP_CHECK(hipMemsetAsync(b.words, 0, FM_ALIGN_WORDS * sizeof(uint64_t), s));
        HIP_CHECK(hipEventRecord(st.ev[0], s));
        launch_align_select(b, s);
        launch_scan(b.item_counts, b.item_offsets, items, temp.ptr, temp.bytes, s);
        HIP_CHECK(hipGetLastError());
        const uint64_t total = read_value(b.item_offsets + items, s);
        if (total > chain.total_chains) return fail(GBWT_HIP_DEVICE_ERROR, "more considered chains than the chains request has chains");
        if (total > FM_ALIGN_MAX_ALIGNMENTS) return fail(GBWT_HIP_UNSUPPORTED, fm_align_plan(items, total, 0, 0, 0, 0).message);
        b.alignments = total;
        CountedBuf tasks(sc, total * sizeof(FmAlignTask));
        CountedBuf direction_words(sc, total * sizeof(uint64_t)), cigar_bound(sc, total * sizeof(uint64_t)), cigar_count(sc, total * sizeof(uint64_t));
        CountedBuf direction_offsets(sc, (total + 1) * sizeof(uint64_t)), cigar_first(sc, (total + 1) * sizeof(uint64_t));
        const uint64_t temp_bytes = std::max<uint64_t>(item_temp, scan_temp_bytes(total + 1));
        if (temp_bytes > temp.bytes) temp.alloc(sc, temp_bytes);
        b.tasks = tasks.as<FmAlignTask>();
        b.direction_words = direction_words.as<uint64_t>(); b.direction_offsets = direction_offsets.as<uint64_t>();
        b.cigar_bound = cigar_bound.as<uint64_t>(); b.cigar_first = cigar_first.as<uint64_t>(); b.cigar_count = cigar_count.as<uint64_t>();
        launch_align_setup(b, s);
        launch_scan(b.direction_words, b.direction_offsets, total, temp.ptr, temp.bytes, s);
        launch_scan(b.cigar_bound, b.cigar_first, total, temp.ptr, temp.bytes, s);
        HIP_CHECK(hipGetLastError());
        const uint64_t all_direction_words = read_value(b.direction_offsets + total, s), all_cigar_entries = read_value(b.cigar_first + total, s);
        if (read_value(b.words + 6, s) != 0) return fail(GBWT_HIP_UNSUPPORTED, "a read of 2^28 bytes or more has a chain to align: the runs of its CIGAR would not fit their 28 bits");
        // 2. the plan: refused before the first kernel that aligns
        size_t free_bytes = 0, all_bytes = 0;
        HIP_CHECK(hipMemGetInfo(&free_bytes, &all_bytes));
        const FmAlignPlan plan = fm_align_plan(items, total, all_direction_words, all_cigar_entries, temp_bytes, uint64_t(free_bytes) + sc.now);
        if (plan.status == FmStatus::Capacity) return fail(GBWT_HIP_CAPACITY, plan.message);
        CountedBuf directions(sc, all_direction_words * sizeof(uint32_t)), cigar_scratch(sc, all_cigar_entries * sizeof(uint32_t));
        b.directions = directions.as<uint32_t>(); b.cigar_scratch = cigar_scratch.as<uint32_t>();
        HIP_CHECK(hipEventRecord(st.ev[1], s));
        // 3. the DP and the walk back; 4. the rows
        launch_align_dp(b, s);
        HIP_CHECK(hipEventRecord(st.ev[2], s));
        st.read_offsets.reserve((m + 1) * sizeof(uint64_t));
        st.alignments.reserve(std::max<uint64_t>(total, 1) * sizeof(gbwt_hip_fm_alignment));
        st.cigar_offsets.reserve((total + 1) * sizeof(uint64_t));
        launch_scan(b.cigar_count, st.cigar_offsets.as<uint64_t>(), total, temp.ptr, temp.bytes, s);
        HIP_CHECK(hipGetLastError());
        const uint64_t total_cigars = read_value(st.cigar_offsets.as<uint64_t>() + total, s);
        if (total_cigars > all_cigar_entries) return fail(GBWT_HIP_DEVICE_ERROR, "more CIGAR entries than their bound");
        st.cigars.reserve(std::max<uint64_t>(total_cigars, 1) * sizeof(uint32_t));
        launch_align_rows(b, st.read_offsets.as<uint64_t>(), st.alignments.as<gbwt_hip_fm_alignment>(), st.cigar_offsets.as<uint64_t>(), st.cigars.as<uint32_t>(), s);
        HIP_CHECK(hipEventRecord(st.ev[3], s));
        uint64_t host_words[FM_ALIGN_WORDS] = {};
        HIP_CHECK(hipMemcpyAsync(host_words, b.words, sizeof(host_words), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        gbwt_hip_fm_align_info &info = st.info;
        const uint64_t requests = info.requests + 1;
        info = gbwt_hip_fm_align_info{};
        info.requests = requests;
        info.items = items; info.chains = total; info.alignments = total;
        info.wide = host_words[1]; info.unreachable = host_words[2]; info.cells = host_words[3]; info.cigar_ops = total_cigars;
        info.lds_alignments = host_words[4]; info.global_alignments = host_words[5];
        info.planned_scratch_bytes = plan.scratch_bytes; info.peak_scratch_bytes = sc.peak;
        info.chains_ms = chains_ms;
        HIP_CHECK(hipEventElapsedTime(&info.select_ms, st.ev[0], st.ev[1]));
        HIP_CHECK(hipEventElapsedTime(&info.dp_ms, st.ev[1], st.ev[2]));
        HIP_CHECK(hipEventElapsedTime(&info.rows_ms, st.ev[2], st.ev[3]));
        st.m = m; st.total_alignments = total; st.total_cigars = total_cigars;
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        (void)hipDeviceSynchronize();                    // (the scratch goes: nothing of the request may still run)
        return status_of(e, "an alignments request");
    }
}

// A chains request through the object's chains state and memo, then the alignment.  Exactly one of h_offsets / d_offsets.
gbwt_hip_status alignments_compute(gbwt_hip_fm_index *fm, const uint64_t *h_offsets, const void *h_bytes, const uint64_t *d_offsets, const uint8_t *d_bytes, uint64_t m, uint64_t bytes,
                                   const gbwt_hip_fm_seed_options &seed_opts, const gbwt_hip_fm_chain_options &chain_opts, const gbwt_hip_fm_align_options &align_opts) {
    gbwt_hip_fm_align_state &st = fm->align;
    const std::initializer_list<int64_t> params = {seed_opts.min_length, seed_opts.strands, static_cast<int64_t>(seed_opts.max_occurrences), static_cast<int64_t>(m),
                                                   chain_opts.max_gap, chain_opts.max_skew, chain_opts.gap_cost, chain_opts.min_score, static_cast<int64_t>(chain_opts.max_matches),
                                                   align_opts.band, fm_align_max_width(align_opts.max_width), static_cast<int64_t>(align_opts.max_alignments)};
    if (h_offsets && st.memo.matches({{h_offsets, (m + 1) * sizeof(uint64_t)}, {h_bytes, h_offsets[m]}}, params)) return GBWT_HIP_OK;
    st.memo.drop();
    const uint64_t chain_requests = fm->chain.info.requests;
    gbwt_hip_status status = fm_chains_compute(fm, h_offsets, h_bytes, d_offsets, d_bytes, m, bytes, seed_opts, chain_opts);
    if (status != GBWT_HIP_OK) return status;
    const gbwt_hip_fm_chain_info &ci = fm->chain.info;
    const float chains_ms = ci.requests != chain_requests ? ci.seeds_ms + ci.expand_ms + ci.sort_ms + ci.dp_ms + ci.peel_ms + ci.fill_ms : 0.0f;
    if (h_offsets) {                                     // the reads in HBM: a copy of the request's own, whatever the seeds state was last asked
        try {
            HIP_CHECK(hipSetDevice(fm->device));
            st.q_offsets.reserve((m + 1) * sizeof(uint64_t));
            st.q_bytes.reserve(std::max<uint64_t>(h_offsets[m], 1));
            HIP_CHECK(hipMemcpyAsync(st.q_offsets.ptr, h_offsets, (m + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, fm->stream));
            if (h_offsets[m]) HIP_CHECK(hipMemcpyAsync(st.q_bytes.ptr, h_bytes, h_offsets[m], hipMemcpyHostToDevice, fm->stream));
        } catch (const HipError &e) {
            return status_of(e, "the reads of an alignments request");
        }
        d_offsets = st.q_offsets.as<uint64_t>();
        d_bytes = st.q_bytes.as<uint8_t>();
    }
    status = align_chains(fm, d_offsets, d_bytes, seed_opts, align_opts, chains_ms);
    if (status != GBWT_HIP_OK) return status;
    if (h_offsets) st.memo.store({{h_offsets, (m + 1) * sizeof(uint64_t)}, {h_bytes, h_offsets[m]}}, params);
    return GBWT_HIP_OK;
}

gbwt_hip_fm_alignment_rows rows_of(const gbwt_hip_fm_index *fm) {
    const gbwt_hip_fm_align_state &st = fm->align;
    return gbwt_hip_fm_alignment_rows{st.read_offsets.as<uint64_t>(), st.alignments.as<gbwt_hip_fm_alignment>(), st.cigar_offsets.as<uint64_t>(), st.cigars.as<uint32_t>(),
                                      st.total_alignments, st.total_cigars, st.m};
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_fm_set_text_device(gbwt_hip_fm_index *fm, const void *d_text, uint64_t n, void *stream) {
    GBWT_HIP_GUARD_BEGIN
    if (!fm) return fail(GBWT_HIP_BAD_ARGUMENT, "null FM-index");
    if (n != fm->n) return fail(GBWT_HIP_BAD_ARGUMENT, "the text has " + std::to_string(n) + " bytes, the text of the FM-index " + std::to_string(fm->n));
    if (n && !d_text) return fail(GBWT_HIP_BAD_ARGUMENT, "null text");
    try {
        HIP_CHECK(hipSetDevice(fm->device));
        return keep_text(fm, static_cast<const uint8_t *>(d_text), n, static_cast<hipStream_t>(stream));
    } catch (const HipError &e) {
        (void)hipDeviceSynchronize();
        return status_of(e, "the text of the FM-index");
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_set_text(gbwt_hip_fm_index *fm, const void *text, uint64_t n) {
    GBWT_HIP_GUARD_BEGIN
    if (!fm) return fail(GBWT_HIP_BAD_ARGUMENT, "null FM-index");
    if (n != fm->n) return fail(GBWT_HIP_BAD_ARGUMENT, "the text has " + std::to_string(n) + " bytes, the text of the FM-index " + std::to_string(fm->n));
    if (n && !text) return fail(GBWT_HIP_BAD_ARGUMENT, "null text");
    try {
        HIP_CHECK(hipSetDevice(fm->device));
        DeviceBuffer d_text;
        d_text.reserve(std::max<uint64_t>(n, 1));
        if (n) HIP_CHECK(hipMemcpyAsync(d_text.ptr, text, n, hipMemcpyHostToDevice, fm->stream));
        const gbwt_hip_status st = keep_text(fm, d_text.as<uint8_t>(), n, fm->stream);
        (void)hipStreamSynchronize(fm->stream);          // (the upload goes)
        return st;
    } catch (const HipError &e) {
        (void)hipDeviceSynchronize();
        return status_of(e, "the text of the FM-index");
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_keep_path_text(gbwt_hip_fm_index *fm, const gbwt_hip_index *ix, gbwt_hip_workspace *ws) {
    GBWT_HIP_GUARD_BEGIN
    gbwt_hip_status st = fm_check_object(fm, FM_GRAPH, ix, ws, 0);
    if (st != GBWT_HIP_OK) return st;
    gbwt_hip_lines text{};                               // the bases family's, valid until the next request for bases on `ws`
    st = gbwt_hip_path_sequences_device(ix, ws, fm->path_ids.data(), fm->path_ids.size(), 0, fm->endmarker, &text);
    if (st != GBWT_HIP_OK) return st;
    if (text.total != fm->n) return fail(GBWT_HIP_DEVICE_ERROR, "the text of the paths is not as long as the one the FM-index was built from");
    try {
        HIP_CHECK(hipSetDevice(fm->device));
        HIP_CHECK(hipStreamSynchronize(ws->stream));
        return keep_text(fm, reinterpret_cast<const uint8_t *>(text.d_text), fm->n, fm->stream);
    } catch (const HipError &e) {
        (void)hipDeviceSynchronize();
        return status_of(e, "the text of the FM-index");
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_last_align_info(const gbwt_hip_fm_index *fm, gbwt_hip_fm_align_info *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!fm || !out) return fail(GBWT_HIP_BAD_ARGUMENT, "null argument");
    *out = fm->align.info;
    out->tile_bytes = FM_ALIGN_TILE_BYTES;
    out->text_bytes = fm->has_text ? fm->text.bytes : 0;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_alignments(gbwt_hip_fm_index *fm, const uint64_t *offsets, const void *bytes, uint64_t m, const gbwt_hip_fm_seed_options *seed_opts,
                                       const gbwt_hip_fm_chain_options *chain_opts, const gbwt_hip_fm_align_options *align_opts, uint64_t *out_read_offsets,
                                       gbwt_hip_fm_alignment *alignments, uint64_t capacity, uint64_t *total_alignments, uint64_t *out_cigar_offsets, uint32_t *cigars,
                                       uint64_t cigar_capacity, uint64_t *total_cigars) {
    GBWT_HIP_GUARD_BEGIN
    if (total_alignments) *total_alignments = 0;
    if (total_cigars) *total_cigars = 0;
    if (!total_alignments || !total_cigars || !out_read_offsets) return fail(GBWT_HIP_BAD_ARGUMENT, "null totals / read offsets");
    if (alignments && !out_cigar_offsets) return fail(GBWT_HIP_BAD_ARGUMENT, "null cigar offsets (one more than the alignments)");
    gbwt_hip_status st = check_request(fm, offsets, bytes, m, true, seed_opts, chain_opts, align_opts);
    if (st == GBWT_HIP_OK) st = alignments_compute(fm, offsets, bytes, nullptr, nullptr, m, 0, *seed_opts, *chain_opts, *align_opts);
    if (st != GBWT_HIP_OK) return st;
    const gbwt_hip_fm_alignment_rows rows = rows_of(fm);
    *total_alignments = rows.total_alignments;
    *total_cigars = rows.total_cigars;
    try {
        HIP_CHECK(hipSetDevice(fm->device));
        if (alignments && capacity < rows.total_alignments)
            return fail(GBWT_HIP_CAPACITY, "alignment capacity too small: the rows hold " + std::to_string(rows.total_alignments) + " alignments");
        if (cigars && cigar_capacity < rows.total_cigars) return fail(GBWT_HIP_CAPACITY, "cigar capacity too small: the rows hold " + std::to_string(rows.total_cigars) + " entries");
        HIP_CHECK(hipMemcpy(out_read_offsets, rows.d_read_offsets, (rows.m + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (alignments && rows.total_alignments) HIP_CHECK(hipMemcpy(alignments, rows.d_alignments, rows.total_alignments * sizeof(gbwt_hip_fm_alignment), hipMemcpyDeviceToHost));
        if (alignments) HIP_CHECK(hipMemcpy(out_cigar_offsets, rows.d_cigar_offsets, (rows.total_alignments + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (cigars && rows.total_cigars) HIP_CHECK(hipMemcpy(cigars, rows.d_cigars, rows.total_cigars * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_alignments_device(gbwt_hip_fm_index *fm, const uint64_t *d_offsets, const void *d_bytes, uint64_t m, uint64_t bytes,
                                              const gbwt_hip_fm_seed_options *seed_opts, const gbwt_hip_fm_chain_options *chain_opts, const gbwt_hip_fm_align_options *align_opts,
                                              gbwt_hip_fm_alignment_rows *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_fm_alignment_rows{nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
    gbwt_hip_status st = check_request(fm, d_offsets, d_bytes, m, false, seed_opts, chain_opts, align_opts);
    if (st == GBWT_HIP_OK) st = alignments_compute(fm, nullptr, nullptr, d_offsets, static_cast<const uint8_t *>(d_bytes), m, bytes, *seed_opts, *chain_opts, *align_opts);
    if (st != GBWT_HIP_OK) return st;
    *out = rows_of(fm);
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

}  // extern "C"
