// capi_fm.hip -- the C ABI of the FM-index family (include/gbwt_hip.h, "FM-index over a text"): the build from a text in host or device
// memory or from the text of paths on a workspace, and the batched queries -- count, locate, graph positions -- in their host-pointer and
// device-pointer forms.  The kernels are fm_index.hip, the layout fm_layout.hpp, the sizes and refusals fm_plan.hpp; the suffix array is
// the suffix array family's (suffix_array.hip), the tags of located positions the tags family's (capi_tags.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "capi_internal.hpp"
#include "device_common.hpp"
#include "extract_files.hpp"
#include "fm_index.hpp"
#include "fm_object.hpp"
#include "fm_plan.hpp"
#include "kernels.hpp"
#include "scan.hpp"
#include "suffix_array.hpp"

using namespace gbwt_hip;

namespace {

constexpr uint64_t WORDS = 4;
using Kind = FmKind;
constexpr Kind COUNT = FM_COUNT, LOCATE = FM_LOCATE, GRAPH = FM_GRAPH;

gbwt_hip_status check_build(int sentinel, uint32_t flags, gbwt_hip_fm_index **out) {
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = nullptr;
    if (sentinel < 0 || sentinel > 255) return fail(GBWT_HIP_BAD_ARGUMENT, "sentinel must be a byte value 0..255");
    if ((flags & ~uint32_t(GBWT_HIP_FM_COUNT_ONLY)) != 0) return fail(GBWT_HIP_BAD_ARGUMENT, "flags: 0 or GBWT_HIP_FM_COUNT_ONLY");
    return GBWT_HIP_OK;
}

gbwt_hip_status check_width(uint64_t n) {
    const FmPlan width = fm_check_width(n);
    if (width.status != FmStatus::Ok) return fail(GBWT_HIP_UNSUPPORTED, width.message);
    return GBWT_HIP_OK;
}

// The index of d_text[0, n) into `fm` on stream s; d_sa: its suffix array, or null: made here.  Done, with all scratch freed, on return.
gbwt_hip_status build_index(gbwt_hip_fm_index &fm, const uint8_t *d_text, uint64_t n, uint8_t sentinel, const uint64_t *d_sa, bool count_only, hipStream_t s) {
    fm.n = n;
    fm.count_only = count_only;
    gbwt_hip_fm_index_info &info = fm.info;
    info = gbwt_hip_fm_index_info{};
    info.n = n;
    info.count_only = count_only ? 1 : 0;
    EventSet<7> ev;
    // 1. the alphabet
    DeviceBuffer histogram, words;
    histogram.reserve(FM_HISTOGRAM_BYTES);
    words.reserve(SA_MIN_BUFFER);
    std::vector<uint64_t> hist(256, 0);
    HIP_CHECK(hipMemsetAsync(histogram.ptr, 0, FM_HISTOGRAM_BYTES, s));
    HIP_CHECK(hipMemsetAsync(words.ptr, 0, SA_MIN_BUFFER, s));
    HIP_CHECK(hipEventRecord(ev[0], s));
    launch_fm_histogram(d_text, n, histogram.as<uint64_t>(), s);
    HIP_CHECK(hipEventRecord(ev[1], s));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(hist.data(), histogram.ptr, FM_HISTOGRAM_BYTES, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));                  // the alphabet decides the layout
    struct Tables { uint16_t code[256]; uint32_t C[256]; } tables{};
    static_assert(sizeof(Tables) == FM_TABLE_BYTES, "the tables as fm_plan.hpp counts them");
    uint32_t sigma = 0;
    uint64_t smaller = 0;
    for (int b = 0; b < 256; b++) {
        tables.code[b] = FM_ABSENT;
        if (hist[b] == 0) continue;
        tables.code[b] = static_cast<uint16_t>(sigma);
        tables.C[sigma++] = static_cast<uint32_t>(smaller);
        smaller += hist[b];
    }
    // 2. the plan
    const bool packed = fm_is_packed(sigma);
    const uint64_t rows = n + 1, blocks = fm_blocks(rows, packed);
    size_t free_bytes = 0, all_bytes = 0;
    HIP_CHECK(hipMemGetInfo(&free_bytes, &all_bytes));
    const FmPlan plan = fm_plan(n, sigma, count_only, d_sa == nullptr, n ? fm_scan_temp_bytes(blocks, sigma) : 0, uint64_t(free_bytes) + histogram.bytes + words.bytes);
    if (plan.status == FmStatus::Capacity) return fail(GBWT_HIP_CAPACITY, plan.message);
    DeviceBuffer block_counts, scanned, temp, sa64;
    fm.lines.reserve(plan.lines_bytes);
    if (plan.counts_bytes) fm.counts.reserve(plan.counts_bytes);
    fm.tables.reserve(plan.tables_bytes);
    if (plan.sa_bytes) fm.sa.reserve(plan.sa_bytes);
    if (n) {
        block_counts.reserve(plan.block_count_bytes);
        scanned.reserve(plan.block_count_bytes);
        temp.reserve(plan.temp_bytes);
        if (d_sa == nullptr) sa64.reserve(plan.sa64_bytes);
    }
    info.sigma = sigma;
    info.packed = packed ? 1 : 0;
    info.block_rows = plan.block_rows;
    info.blocks = blocks;
    info.planned_index_bytes = plan.index_bytes;
    info.planned_scratch_bytes = plan.scratch_bytes;
    info.peak_scratch_bytes = bytes_of({&histogram, &words, &block_counts, &scanned, &temp, &sa64});
    // 3. the suffix array, unless the caller brought it
    if (n && d_sa == nullptr) {
        SaContext ctx;
        ctx.ensure();
        gbwt_hip_suffix_array_info sa_info{};
        const gbwt_hip_status st = build_suffix_array(d_text, n, sentinel, sa64.as<uint64_t>(), nullptr, ctx, s, sa_info);
        if (st != GBWT_HIP_OK) return st;
        info.suffix_array_ms = sa_info.pack_ms + sa_info.rank_ms + sa_info.output_ms;
        d_sa = sa64.as<uint64_t>();
    }
    // 4. codes, block counts, their sums across the blocks, the fill, the narrow suffix array
    uint64_t *d_words = words.as<uint64_t>();            // [0] primary row, [1] a suffix array value outside the text
    HIP_CHECK(hipMemsetAsync(fm.lines.ptr, 0, fm.lines.bytes, s));
    HIP_CHECK(hipMemcpyAsync(fm.tables.ptr, &tables, sizeof(tables), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(ev[2], s));
    if (n) {
        launch_fm_codes(d_text, d_sa, n, fm.tables.as<uint16_t>(), packed, fm.lines.as<uint8_t>(), d_words, s);
        HIP_CHECK(hipEventRecord(ev[3], s));
        launch_fm_block_counts(fm.lines.as<uint8_t>(), rows, blocks, sigma, packed, d_words, block_counts.as<uint32_t>(), s);
        launch_fm_scan(block_counts.as<uint32_t>(), scanned.as<uint32_t>(), blocks, sigma, temp.ptr, temp.bytes, s);
        HIP_CHECK(hipEventRecord(ev[4], s));
        launch_fm_fill(scanned.as<uint32_t>(), blocks, sigma, packed, fm.lines.as<uint8_t>(), fm.counts.as<uint32_t>(), s);
        HIP_CHECK(hipEventRecord(ev[5], s));
        if (!count_only) launch_fm_narrow_sa(d_sa, n, fm.sa.as<uint32_t>(), s);
        HIP_CHECK(hipEventRecord(ev[6], s));
    }
    uint64_t head[2] = {0, 0};
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(head, d_words, sizeof(head), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));                  // (`tables` and `head` leave the stack; the scratch goes)
    HIP_CHECK(hipGetLastError());
    if (n && (head[1] != 0 || head[0] == 0 || head[0] > n)) return fail(GBWT_HIP_INVALID_DATA, "the suffix array holds a value outside the text, or no entry 0");
    HIP_CHECK(hipEventElapsedTime(&info.histogram_ms, ev[0], ev[1]));
    if (n) {
        HIP_CHECK(hipEventElapsedTime(&info.codes_ms, ev[2], ev[3]));
        HIP_CHECK(hipEventElapsedTime(&info.counts_ms, ev[3], ev[4]));
        HIP_CHECK(hipEventElapsedTime(&info.fill_ms, ev[4], ev[5]));
        HIP_CHECK(hipEventElapsedTime(&info.narrow_ms, ev[5], ev[6]));
    }
    fm.layout.sigma = sigma;
    fm.layout.packed = packed ? 1 : 0;
    fm.layout.rows = rows;
    fm.layout.blocks = blocks;
    fm.layout.primary = head[0];
    fm.layout.lines = fm.lines.as<uint8_t>();
    fm.layout.counts = fm.counts.as<uint32_t>();
    info.primary = n ? head[0] - 1 : 0;
    info.index_bytes = fm.index_bytes();
    info.sa_bytes = fm.sa.bytes;
    return GBWT_HIP_OK;
}

// A new object on `device` with its stream, built by `build`; nothing is left behind a failure
template <class Build>
gbwt_hip_status make_index(int device, gbwt_hip_fm_index **out, Build build) {
    gbwt_hip_status st = require_device();
    if (st != GBWT_HIP_OK) return st;
    gbwt_hip_fm_index *fm = nullptr;
    try {
        HIP_CHECK(hipSetDevice(device));
        fm = new gbwt_hip_fm_index();
        fm->device = device;
        fm->stream.create(hipStreamNonBlocking);
        st = build(*fm);
        if (st != GBWT_HIP_OK) { (void)hipDeviceSynchronize(); delete fm; return st; }
        *out = fm;
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        (void)hipDeviceSynchronize();
        delete fm;
        return status_of(e, "the FM-index");
    } catch (...) {
        delete fm;
        throw;
    }
}

// The rows of a request into the object.  Exactly one of h_offsets / d_offsets; bytes: the pattern bytes behind d_bytes (the host form: offsets[m]).
gbwt_hip_status fm_compute(gbwt_hip_fm_index *fm, Kind kind, const uint64_t *h_offsets, const void *h_bytes, const uint64_t *d_offsets, const uint8_t *d_bytes, uint64_t m, uint64_t bytes,
                           int unique, const gbwt_hip_index *ix, gbwt_hip_workspace *ws) {
    if (h_offsets) {
        bytes = h_offsets[m];
        if (fm->memo.matches({{h_offsets, (m + 1) * sizeof(uint64_t)}, {h_bytes, bytes}}, {kind, unique, static_cast<int64_t>(m)})) return GBWT_HIP_OK;
    }
    fm->memo.drop();
    try {
        HIP_CHECK(hipSetDevice(fm->device));
        hipStream_t s = fm->stream;
        fm->ev.ensure();
        const uint64_t slots = std::max<uint64_t>(m, 1);
        fm->ranges.reserve(2 * slots * sizeof(uint64_t));
        fm->occ.reserve(slots * sizeof(uint64_t));
        fm->roff.reserve((slots + 1) * sizeof(uint64_t));
        fm->words.reserve(WORDS * sizeof(uint64_t));
        fm->temp.reserve(scan_temp_bytes(m));
        uint64_t *d_words = fm->words.as<uint64_t>();
        HIP_CHECK(hipMemsetAsync(d_words, 0, WORDS * sizeof(uint64_t), s));
        if (h_offsets) {
            fm->q_offsets.reserve((m + 1) * sizeof(uint64_t));
            fm->q_bytes.reserve(std::max<uint64_t>(bytes, 1));
            HIP_CHECK(hipMemcpyAsync(fm->q_offsets.ptr, h_offsets, (m + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            if (bytes) HIP_CHECK(hipMemcpyAsync(fm->q_bytes.ptr, h_bytes, bytes, hipMemcpyHostToDevice, s));
            d_offsets = fm->q_offsets.as<uint64_t>();
            d_bytes = fm->q_bytes.as<uint8_t>();
        }
        // 1. the ranges
        HIP_CHECK(hipEventRecord(fm->ev[0], s));
        launch_fm_count(fm->layout, FmTables{fm->tables.as<uint16_t>(), reinterpret_cast<const uint32_t *>(fm->tables.as<uint16_t>() + 256)}, d_offsets, d_bytes, m, bytes,
                        fm->ranges.as<uint64_t>(), fm->occ.as<uint64_t>(), d_words, s);
        HIP_CHECK(hipEventRecord(fm->ev[1], s));
        HIP_CHECK(hipGetLastError());
        uint64_t total = 0;
        fm->unique_rows = false;
        if (kind != COUNT) {
            // 2. the rows' offsets; the one wait in front of the rows: the total sizes them
            launch_scan(fm->occ.as<uint64_t>(), fm->roff.as<uint64_t>(), m, fm->temp.ptr, fm->temp.bytes, s);
            HIP_CHECK(hipMemcpyAsync(&total, fm->roff.as<uint64_t>() + m, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            const bool sorted = kind == GRAPH && unique != 0 && total != 0;
            if (sorted && total > 0x7FFFFFFFull) return fail(GBWT_HIP_UNSUPPORTED, "a unique request of " + std::to_string(total) + " positions: more than one sort takes (2^31 - 1)");
            fm->positions.reserve(std::max<uint64_t>(total, 1) * sizeof(uint64_t));
            if (sorted) fm->rows.reserve(total * sizeof(uint32_t));
            // 3. the positions
            launch_fm_locate_fill(fm->sa.as<uint32_t>(), fm->ranges.as<uint64_t>(), fm->roff.as<uint64_t>(), m, fm->positions.as<uint64_t>(), sorted ? fm->rows.as<uint32_t>() : nullptr, s);
        }
        HIP_CHECK(hipEventRecord(fm->ev[2], s));
        uint64_t words[WORDS] = {};
        HIP_CHECK(hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        if (static_cast<uint32_t>(words[0]) & FM_FLAG_OFFSETS) return fail(GBWT_HIP_BAD_ARGUMENT, "pattern offsets descend or leave the pattern bytes");
        if (kind == GRAPH) {
            // 4. the tags of the positions, by the tags family on its workspace; distinct per row for a unique request
            fm->tags.reserve(std::max<uint64_t>(total, 1) * sizeof(uint64_t));
            const gbwt_hip_status st = gbwt_hip_tags_device(ix, ws, fm->path_ids.data(), fm->path_ids.size(), fm->positions.as<uint64_t>(), total, fm->tags.as<uint64_t>(), nullptr);
            if (st != GBWT_HIP_OK) return st;
            HIP_CHECK(hipSetDevice(fm->device));
            if (unique != 0 && total != 0) {
                for (DeviceBuffer *b : {&fm->tmp_values, &fm->sorted_values, &fm->flag, &fm->kept}) b->reserve(total * sizeof(uint64_t));
                for (DeviceBuffer *b : {&fm->tmp_rows, &fm->sorted_rows}) b->reserve(total * sizeof(uint32_t));
                fm->rank.reserve((total + 1) * sizeof(uint64_t));
                fm->uoff.reserve((m + 1) * sizeof(uint64_t));
                fm->temp.reserve(std::max<size_t>(fm_sort_temp_bytes(total), scan_temp_bytes(total)));
                launch_fm_sort_rows(fm->tags.as<uint64_t>(), fm->rows.as<uint32_t>(), total, bits_for(m, 32), fm->tmp_values.as<uint64_t>(), fm->tmp_rows.as<uint32_t>(),
                                    fm->sorted_values.as<uint64_t>(), fm->sorted_rows.as<uint32_t>(), fm->temp.ptr, fm->temp.bytes, s);
                launch_fm_run_flags(fm->sorted_values.as<uint64_t>(), fm->sorted_rows.as<uint32_t>(), total, fm->flag.as<uint64_t>(), s);
                launch_scan(fm->flag.as<uint64_t>(), fm->rank.as<uint64_t>(), total, fm->temp.ptr, fm->temp.bytes, s);
                launch_fm_compact(fm->sorted_values.as<uint64_t>(), fm->rank.as<uint64_t>(), total, fm->roff.as<uint64_t>(), m, fm->kept.as<uint64_t>(), fm->uoff.as<uint64_t>(), s);
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipMemcpyAsync(&total, fm->rank.as<uint64_t>() + total, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
                HIP_CHECK(hipGetLastError());
                fm->unique_rows = true;
            }
        }
        HIP_CHECK(hipEventElapsedTime(&fm->info.last_count_ms, fm->ev[0], fm->ev[1]));
        HIP_CHECK(hipEventElapsedTime(&fm->info.last_fill_ms, fm->ev[1], fm->ev[2]));
        fm->info.queries++;
        fm->info.last_patterns = m;
        fm->info.last_steps = words[1];
        fm->info.last_total = total;
        fm->last_m = m;
        fm->last_total = total;
        if (h_offsets) fm->memo.store({{h_offsets, (m + 1) * sizeof(uint64_t)}, {h_bytes, bytes}}, {kind, unique, static_cast<int64_t>(m)});
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e, "an FM-index request");
    }
}

const uint64_t *result_offsets(const gbwt_hip_fm_index *fm) { return (fm->unique_rows ? fm->uoff : fm->roff).as<uint64_t>(); }
const uint64_t *result_values(const gbwt_hip_fm_index *fm, Kind kind) { return kind == LOCATE ? fm->positions.as<uint64_t>() : (fm->unique_rows ? fm->kept : fm->tags).as<uint64_t>(); }

// The host form of a request with rows: offsets always, values when asked for and the capacity holds them
gbwt_hip_status rows_to_host(gbwt_hip_fm_index *fm, Kind kind, uint64_t m, uint64_t *out_offsets, uint64_t *out_values, uint64_t capacity, uint64_t *total) {
    *total = fm->last_total;
    try {
        HIP_CHECK(hipSetDevice(fm->device));
        HIP_CHECK(hipMemcpyAsync(out_offsets, result_offsets(fm), (m + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, fm->stream));
        HIP_CHECK(hipStreamSynchronize(fm->stream));
        if (!out_values) return GBWT_HIP_OK;
        if (capacity < *total) return fail(GBWT_HIP_CAPACITY, "output capacity too small: the rows hold " + std::to_string(*total) + " values");
        if (*total) HIP_CHECK(hipMemcpy(out_values, result_values(fm, kind), *total * sizeof(uint64_t), hipMemcpyDeviceToHost));
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
}

gbwt_hip_fm_located located_of(const gbwt_hip_fm_index *fm, Kind kind) {
    return gbwt_hip_fm_located{result_offsets(fm), result_values(fm, kind), fm->ranges.as<uint64_t>(), fm->last_total, fm->last_m};
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_fm_build_text_device(int device, const void *d_text, uint64_t n, int sentinel, const uint64_t *d_sa, uint32_t flags, void *stream, gbwt_hip_fm_index **out) {
    GBWT_HIP_GUARD_BEGIN
    gbwt_hip_status st = check_build(sentinel, flags, out);
    if (st != GBWT_HIP_OK) return st;
    if (n && !d_text) return fail(GBWT_HIP_BAD_ARGUMENT, "null text");
    st = check_width(n);
    if (st != GBWT_HIP_OK) return st;
    return make_index(device, out, [&](gbwt_hip_fm_index &fm) {
        return build_index(fm, static_cast<const uint8_t *>(d_text), n, static_cast<uint8_t>(sentinel), d_sa, (flags & GBWT_HIP_FM_COUNT_ONLY) != 0, static_cast<hipStream_t>(stream));
    });
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_build_text(int device, const void *text, uint64_t n, int sentinel, uint32_t flags, gbwt_hip_fm_index **out) {
    GBWT_HIP_GUARD_BEGIN
    gbwt_hip_status st = check_build(sentinel, flags, out);
    if (st != GBWT_HIP_OK) return st;
    if (n && !text) return fail(GBWT_HIP_BAD_ARGUMENT, "null text");
    st = check_width(n);
    if (st != GBWT_HIP_OK) return st;
    return make_index(device, out, [&](gbwt_hip_fm_index &fm) {
        DeviceBuffer d_text;
        d_text.reserve(std::max<uint64_t>(n, 1));
        if (n) HIP_CHECK(hipMemcpyAsync(d_text.ptr, text, n, hipMemcpyHostToDevice, fm.stream));
        const gbwt_hip_status built = build_index(fm, d_text.as<uint8_t>(), n, static_cast<uint8_t>(sentinel), nullptr, (flags & GBWT_HIP_FM_COUNT_ONLY) != 0, fm.stream);
        (void)hipStreamSynchronize(fm.stream);           // (the text goes)
        return built;
    });
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_path_fm_index(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int endmarker, uint32_t flags, gbwt_hip_fm_index **out) {
    GBWT_HIP_GUARD_BEGIN
    gbwt_hip_status st = check_build(0, flags, out);
    if (st != GBWT_HIP_OK) return st;
    if (!ix || !ws || ws->index != ix) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    if (n && !path_ids) return fail(GBWT_HIP_BAD_ARGUMENT, "null path_ids");
    if (endmarker < 0 || endmarker > 255) return fail(GBWT_HIP_BAD_ARGUMENT, "endmarker must be a byte value 0..255: the tags of the text count one behind every path");
    gbwt_hip_suffix_array sa{};
    st = gbwt_hip_path_suffix_array_device(ix, ws, path_ids, n, endmarker, &sa);
    if (st != GBWT_HIP_OK) return st;
    gbwt_hip_lines text{};                               // the text the suffix array was made of: still the bases family's
    st = gbwt_hip_path_sequences_device(ix, ws, path_ids, n, 0, endmarker, &text);
    if (st != GBWT_HIP_OK) return st;
    if (text.total != sa.total) return fail(GBWT_HIP_DEVICE_ERROR, "the text of the paths changed under its suffix array");
    return make_index(ix->device, out, [&](gbwt_hip_fm_index &fm) {
        HIP_CHECK(hipStreamSynchronize(ws->stream));
        const gbwt_hip_status built = build_index(fm, reinterpret_cast<const uint8_t *>(text.d_text), sa.total, static_cast<uint8_t>(endmarker), sa.d_sa,
                                                  (flags & GBWT_HIP_FM_COUNT_ONLY) != 0, fm.stream);
        if (built != GBWT_HIP_OK) return built;
        fm.info.path_level = 1;
        fm.index = ix;
        fm.path_ids.assign(path_ids, path_ids + n);
        fm.endmarker = endmarker;
        // the segments of the chains: the rows of the text, each with its endmarker (sequences.hip counts it into the row)
        fm.path_offsets.reserve((n + 1) * sizeof(uint64_t));
        if (n) HIP_CHECK(hipMemcpyAsync(fm.path_offsets.ptr, text.d_line_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, fm.stream));
        else HIP_CHECK(hipMemsetAsync(fm.path_offsets.ptr, 0, sizeof(uint64_t), fm.stream));
        HIP_CHECK(hipStreamSynchronize(fm.stream));
        return GBWT_HIP_OK;
    });
    GBWT_HIP_GUARD_END
}

void gbwt_hip_fm_close(gbwt_hip_fm_index *fm) {
    if (!fm) return;
    (void)hipSetDevice(fm->device);
    if (fm->stream.s) (void)hipStreamSynchronize(fm->stream);
    delete fm;
}

gbwt_hip_status gbwt_hip_fm_info(const gbwt_hip_fm_index *fm, gbwt_hip_fm_index_info *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!fm || !out) return fail(GBWT_HIP_BAD_ARGUMENT, "null argument");
    *out = fm->info;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_count(gbwt_hip_fm_index *fm, const uint64_t *offsets, const void *bytes, uint64_t m, uint64_t *ranges) {
    GBWT_HIP_GUARD_BEGIN
    if (m && !ranges) return fail(GBWT_HIP_BAD_ARGUMENT, "null ranges");
    gbwt_hip_status st = fm_check_patterns(offsets, bytes, m, true);
    if (st == GBWT_HIP_OK) st = fm_check_object(fm, COUNT, nullptr, nullptr, 0);
    if (st == GBWT_HIP_OK) st = fm_compute(fm, COUNT, offsets, bytes, nullptr, nullptr, m, 0, 0, nullptr, nullptr);
    if (st != GBWT_HIP_OK || m == 0) return st;
    try {
        HIP_CHECK(hipMemcpy(ranges, fm->ranges.ptr, 2 * m * sizeof(uint64_t), hipMemcpyDeviceToHost));
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_count_device(gbwt_hip_fm_index *fm, const uint64_t *d_offsets, const void *d_bytes, uint64_t m, uint64_t bytes, gbwt_hip_fm_located *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_fm_located{nullptr, nullptr, nullptr, 0, 0};
    gbwt_hip_status st = fm_check_patterns(d_offsets, d_bytes, m, false);
    if (st == GBWT_HIP_OK) st = fm_check_object(fm, COUNT, nullptr, nullptr, 0);
    if (st == GBWT_HIP_OK) st = fm_compute(fm, COUNT, nullptr, nullptr, d_offsets, static_cast<const uint8_t *>(d_bytes), m, bytes, 0, nullptr, nullptr);
    if (st != GBWT_HIP_OK) return st;
    *out = gbwt_hip_fm_located{nullptr, nullptr, fm->ranges.as<uint64_t>(), 0, m};
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_locate(gbwt_hip_fm_index *fm, const uint64_t *offsets, const void *bytes, uint64_t m, uint64_t *out_offsets, uint64_t *positions, uint64_t capacity,
                                   uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (total) *total = 0;
    if (!total || !out_offsets) return fail(GBWT_HIP_BAD_ARGUMENT, "null total / row offsets");
    gbwt_hip_status st = fm_check_patterns(offsets, bytes, m, true);
    if (st == GBWT_HIP_OK) st = fm_check_object(fm, LOCATE, nullptr, nullptr, 0);
    if (st == GBWT_HIP_OK) st = fm_compute(fm, LOCATE, offsets, bytes, nullptr, nullptr, m, 0, 0, nullptr, nullptr);
    if (st != GBWT_HIP_OK) return st;
    return rows_to_host(fm, LOCATE, m, out_offsets, positions, capacity, total);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_locate_device(gbwt_hip_fm_index *fm, const uint64_t *d_offsets, const void *d_bytes, uint64_t m, uint64_t bytes, gbwt_hip_fm_located *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_fm_located{nullptr, nullptr, nullptr, 0, 0};
    gbwt_hip_status st = fm_check_patterns(d_offsets, d_bytes, m, false);
    if (st == GBWT_HIP_OK) st = fm_check_object(fm, LOCATE, nullptr, nullptr, 0);
    if (st == GBWT_HIP_OK) st = fm_compute(fm, LOCATE, nullptr, nullptr, d_offsets, static_cast<const uint8_t *>(d_bytes), m, bytes, 0, nullptr, nullptr);
    if (st != GBWT_HIP_OK) return st;
    *out = located_of(fm, LOCATE);
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_graph_positions(gbwt_hip_fm_index *fm, const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *offsets, const void *bytes, uint64_t m, int unique,
                                            uint64_t *out_offsets, uint64_t *tags, uint64_t capacity, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (total) *total = 0;
    if (!total || !out_offsets) return fail(GBWT_HIP_BAD_ARGUMENT, "null total / row offsets");
    gbwt_hip_status st = fm_check_patterns(offsets, bytes, m, true);
    if (st == GBWT_HIP_OK) st = fm_check_object(fm, GRAPH, ix, ws, unique);
    if (st == GBWT_HIP_OK) st = fm_compute(fm, GRAPH, offsets, bytes, nullptr, nullptr, m, 0, unique, ix, ws);
    if (st != GBWT_HIP_OK) return st;
    return rows_to_host(fm, GRAPH, m, out_offsets, tags, capacity, total);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_fm_graph_positions_device(gbwt_hip_fm_index *fm, const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *d_offsets, const void *d_bytes, uint64_t m,
                                                   uint64_t bytes, int unique, gbwt_hip_fm_located *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_fm_located{nullptr, nullptr, nullptr, 0, 0};
    gbwt_hip_status st = fm_check_patterns(d_offsets, d_bytes, m, false);
    if (st == GBWT_HIP_OK) st = fm_check_object(fm, GRAPH, ix, ws, unique);
    if (st == GBWT_HIP_OK) st = fm_compute(fm, GRAPH, nullptr, nullptr, d_offsets, static_cast<const uint8_t *>(d_bytes), m, bytes, unique, ix, ws);
    if (st != GBWT_HIP_OK) return st;
    *out = located_of(fm, GRAPH);
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

}  // extern "C"
