// capi_locate.hip -- locate queries over the C ABI (include/gbwt_hip.h, "locate"): the locate index of a handle, built by the first call
// that needs it, and the requests for states and positions, computed by the kernels of locate.hip.
#include <string>
#include <vector>

#include "capi_internal.hpp"
#include "device_common.hpp"
#include "scan.hpp"

using namespace gbwt_hip;

namespace {

bool fast_steps(const DeviceIndex &d) { return d.desc_raw != nullptr && d.blocks != nullptr; }

// the index as the locate walks see it: every sample of a sequence starts a segment (as the walk of refpos.hip)
DeviceIndex locate_view(const gbwt_hip_index *ix) {
    DeviceIndex d = ix->dev;
    d.sample_stride = 1; d.sample_part = 0; d.sample_parts = 0;
    return d;
}

uint64_t step_limit(const gbwt_hip_index *ix) { return ix->stats.size + 1; }   // no walk of a consistent index is longer than the BWT

void build_locate(const gbwt_hip_index *ix, hipStream_t s) {
    const DeviceIndex d = locate_view(ix);
    const uint64_t records = d.n_records, sequences = d.n_sequences;
    if (sequences > 0x7FFFFFFFull) throw Unsupported("locate: " + std::to_string(sequences) + " sequences; the locate index holds 32-bit sequence ids and sorts at most 2^31 - 1 end entries");
    EventSet<2> ev;
    DeviceBuffer lens, temp, seg, words, keys_in, ids_in;
    uint32_t launches = 0;
    words.reserve(4 * sizeof(uint64_t));             // [0] slots written, [1] end entries, [2] sampled records with positions, [3] flags (low half)
    uint64_t *d_words = words.as<uint64_t>();
    uint32_t *d_flags = reinterpret_cast<uint32_t *>(d_words + 3);
    HIP_CHECK(hipMemsetAsync(words.ptr, 0, 4 * sizeof(uint64_t), s));
    HIP_CHECK(hipEventRecord(ev.e[0], s));
    // 1. the sampled records and where their positions go
    lens.reserve(std::max<uint64_t>(records, 1) * sizeof(uint64_t));
    ix->locate.base.reserve((records + 1) * sizeof(uint64_t));
    const size_t scan_bytes = scan_temp_bytes(records);
    temp.reserve(std::max(scan_bytes, locate_sort_temp_bytes(sequences)));
    launch_locate_lengths(d, locate_threshold(ix->knobs.locate_interval), lens.as<uint64_t>(), d_flags, s);
    if (records) { launch_scan(lens.as<uint64_t>(), ix->locate.base.as<uint64_t>(), records, temp.ptr, scan_bytes, s); launches += 2; }
    else HIP_CHECK(hipMemsetAsync(ix->locate.base.ptr, 0, sizeof(uint64_t), s));
    launch_locate_bases(lens.as<uint64_t>(), ix->locate.base.as<uint64_t>(), records, d_words + 2, s);
    launches += records ? 1 : 0;
    HIP_CHECK(hipGetLastError());
    uint64_t head[4] = {0, 0, 0, 0}, positions = 0;
    HIP_CHECK(hipMemcpyAsync(&positions, ix->locate.base.as<uint64_t>() + records, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(head, d_words, sizeof(head), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));              // the table is sized by the total
    if (head[3] & LOCATE_FLAG_WIDE) throw Unsupported("locate: a record holds 2^32 - 1 positions or more; the locate index keeps 32-bit offsets");
    const uint64_t sampled = head[2];
    // 2. the table and the end entries, empty
    ix->locate.table.reserve(std::max<uint64_t>(positions, 1) * sizeof(uint32_t));
    ix->locate.end_keys.reserve(std::max<uint64_t>(sequences, 1) * sizeof(uint64_t));
    ix->locate.end_ids.reserve(std::max<uint64_t>(sequences, 1) * sizeof(uint32_t));
    keys_in.reserve(std::max<uint64_t>(sequences, 1) * sizeof(uint64_t));
    ids_in.reserve(std::max<uint64_t>(sequences, 1) * sizeof(uint32_t));
    HIP_CHECK(hipMemsetAsync(ix->locate.table.ptr, 0xFF, std::max<uint64_t>(positions, 1) * sizeof(uint32_t), s));
    HIP_CHECK(hipMemsetAsync(keys_in.ptr, 0xFF, std::max<uint64_t>(sequences, 1) * sizeof(uint64_t), s));
    HIP_CHECK(hipMemsetAsync(ids_in.ptr, 0xFF, std::max<uint64_t>(sequences, 1) * sizeof(uint32_t), s));
    // 3. the walk of every sequence: a lane per sample segment where the handle has samples
    const bool segmented = d.samples != nullptr && d.sample_base != nullptr && ix->max_samples > 0 && ix->sample_counts.size() == sequences;
    uint64_t walkers = sequences;
    if (segmented) {
        std::vector<uint64_t> first(sequences + 1);
        first[0] = 0;
        for (uint64_t k = 0; k < sequences; k++) first[k + 1] = first[k] + ix->sample_counts[k];
        walkers = first[sequences];
        seg.reserve(first.size() * sizeof(uint64_t));
        HIP_CHECK(hipMemcpyAsync(seg.ptr, first.data(), first.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));          // (`first` goes out of scope)
    }
    LocateIndex L{ix->locate.base.as<uint64_t>(), ix->locate.table.as<uint32_t>(), keys_in.as<uint64_t>(), ids_in.as<uint32_t>(), positions, 0};
    launch_locate_build(d, L, seg.as<uint64_t>(), walkers, segmented, step_limit(ix), d_words, d_flags, fast_steps(d), s);
    launches += walkers ? 1 : 0;
    // 4. the ends, sorted by (record, offset): the entries of the empty sequences, all ones, come last
    launch_locate_sort_ends(keys_in.as<uint64_t>(), ix->locate.end_keys.as<uint64_t>(), ids_in.as<uint32_t>(), ix->locate.end_ids.as<uint32_t>(), sequences, temp.ptr, temp.bytes, s);
    launches += sequences ? 1 : 0;
    HIP_CHECK(hipEventRecord(ev.e[1], s));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(head, d_words, sizeof(head), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    const uint32_t flags = static_cast<uint32_t>(head[3]);
    if ((flags & (LOCATE_FLAG_WALK | LOCATE_FLAG_TWICE)) != 0 || head[0] != positions)
        throw InvalidData("locate: the walk of the sequences wrote " + std::to_string(head[0]) + " of the " + std::to_string(positions) + " slots of the table" +
                          ((flags & LOCATE_FLAG_TWICE) ? ", one of them twice" : "") + ((flags & LOCATE_FLAG_WALK) ? "; a walker lost its way" : "") + " (an inconsistent index)");
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    ix->locate.index = LocateIndex{ix->locate.base.as<uint64_t>(), ix->locate.table.as<uint32_t>(), ix->locate.end_keys.as<uint64_t>(), ix->locate.end_ids.as<uint32_t>(), positions, head[1]};
    ix->locate.sampled_records = sampled;
    ix->locate.build_ms = ms;
    ix->locate.build_launches = launches;
}

// The locate index of the handle, built on first use on the stream of the workspace that asks; a build that fails leaves nothing behind
void ensure_locate(const gbwt_hip_index *ix, gbwt_hip_workspace *ws) {
    ix->locate.built.ensure([&] {
        try {
            build_locate(ix, ws->stream);
        } catch (...) {
            (void)hipStreamSynchronize(ws->stream);
            ix->locate.release();
            throw;
        }
    });
}

gbwt_hip_status check_request(const gbwt_hip_index *ix, const gbwt_hip_workspace *ws, const void *items, uint64_t n, int unique) {
    if (unique != 0 && unique != 1) return fail(GBWT_HIP_BAD_ARGUMENT, "unique must be 0 or 1");
    if (!ix || !ws || ws->index != ix) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    if (n && !items) return fail(GBWT_HIP_BAD_ARGUMENT, "null states / positions");
    if (n >= 0xFFFFFFFFull) return fail(GBWT_HIP_BAD_ARGUMENT, "too many rows in one request (32-bit row numbers)");
    return GBWT_HIP_OK;
}

// words of locate.words: [0] flags (low half), [2] LF steps of a counting launch
constexpr uint64_t WORDS = 4;

// The rows of a request, computed into the workspace (locate.off or uoff, ids, valid, total).  Exactly one of h_states / d_states.
// count_steps: the plain rows once more with the step counter, nothing else kept.
gbwt_hip_status locate_compute(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const gbwt_hip_state *h_states, const gbwt_hip_state *d_states, const uint8_t *d_given, uint64_t n,
                               int unique, bool count_steps = false) {
    const size_t state_bytes = n * sizeof(gbwt_hip_state);
    if (h_states != nullptr && !count_steps && ws->locate.memo.matches({{h_states, state_bytes}}, {unique, static_cast<int64_t>(n)})) return GBWT_HIP_OK;
    ws->locate.memo.drop();
    ws->locate.timed = false;
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        hipStream_t s = ws->stream;
        ensure_locate(ix, ws);
        ws->locate.ev.ensure();
        const DeviceIndex d = locate_view(ix);
        const uint64_t rows = std::max<uint64_t>(n, 1);
        ws->locate.counts.reserve(rows * sizeof(uint64_t));
        ws->locate.off.reserve((rows + 1) * sizeof(uint64_t));
        ws->locate.valid.reserve(rows);
        ws->locate.words.reserve(WORDS * sizeof(uint64_t));
        const size_t scan_bytes = scan_temp_bytes(n, ws->knobs.scan_piece);
        ws->scratch.scan_temp.reserve(scan_bytes);
        uint64_t *d_words = ws->locate.words.as<uint64_t>();
        uint32_t *d_flags = reinterpret_cast<uint32_t *>(d_words);
        HIP_CHECK(hipMemsetAsync(d_words, 0, WORDS * sizeof(uint64_t), s));
        if (h_states != nullptr || n == 0) {
            ws->locate.states.reserve(rows * sizeof(gbwt_hip_state));
            if (n) HIP_CHECK(hipMemcpyAsync(ws->locate.states.ptr, h_states, state_bytes, hipMemcpyHostToDevice, s));
            d_states = ws->locate.states.as<gbwt_hip_state>();
            d_given = nullptr;
        }
        // 1. which states are ranges of a record, and the rows' offsets
        launch_locate_valid(d, d_states, d_given, n, ws->locate.counts.as<uint64_t>(), ws->locate.valid.as<uint8_t>(), s);
        launch_scan(ws->locate.counts.as<uint64_t>(), ws->locate.off.as<uint64_t>(), n, ws->scratch.scan_temp.ptr, scan_bytes, s, ws->knobs.scan_piece);
        HIP_CHECK(hipGetLastError());
        const uint64_t total = read_value(ws->locate.off.as<uint64_t>() + n, s);     // the one wait in front of the rows: the total sizes them
        if (total > (~uint64_t(0)) / 64) return fail(GBWT_HIP_CAPACITY, "too many ids for device memory");
        const uint64_t items = std::max<uint64_t>(total, 1);
        const bool keyed = unique != 0 && total != 0 && !count_steps;
        ws->locate.ids.reserve(items * sizeof(uint64_t));
        if (keyed) ws->locate.keys.reserve(items * sizeof(uint64_t));
        // 2. the owner of every position
        HIP_CHECK(hipEventRecord(ws->locate.ev[0], s));
        launch_locate(d, ix->locate.index, d_states, ws->locate.off.as<uint64_t>(), n, total, keyed, step_limit(ix), (keyed ? ws->locate.keys : ws->locate.ids).as<uint64_t>(),
                      count_steps ? d_words + 2 : nullptr, d_flags, fast_steps(d), s);
        HIP_CHECK(hipEventRecord(ws->locate.ev[1], s));
        uint64_t kept = total;
        if (keyed) {
            // 3. unique rows: sorted by (row, id) in pieces of whole rows, the first of every run kept
            const uint64_t piece = std::max<uint64_t>(1, std::min<uint64_t>(ws->knobs.locate_sort_piece, 0x7FFFFFFFull));
            std::vector<uint64_t> cuts{0, total};
            if (total > piece) {
                std::vector<uint64_t> off(n + 1);
                HIP_CHECK(hipMemcpyAsync(off.data(), ws->locate.off.ptr, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
                cuts.assign(1, 0);
                for (uint64_t k = 0; k < n; k++) {
                    if (off[k + 1] - off[k] > piece)
                        return fail(GBWT_HIP_UNSUPPORTED, "locate: row " + std::to_string(k) + " holds " + std::to_string(off[k + 1] - off[k]) + " ids, more than one sort takes (" +
                                                              std::to_string(piece) + ")");
                    if (off[k + 1] - cuts.back() > piece) cuts.push_back(off[k]);
                }
                cuts.push_back(total);
            }
            ws->locate.sorted.reserve(items * sizeof(uint64_t));
            ws->locate.flag.reserve(items * sizeof(uint64_t));
            ws->locate.rank.reserve((items + 1) * sizeof(uint64_t));
            ws->locate.uoff.reserve((rows + 1) * sizeof(uint64_t));
            ws->locate.temp.reserve(locate_sort_temp_bytes(std::min(total, piece)));
            ws->scratch.scan_temp.reserve(scan_temp_bytes(total, ws->knobs.scan_piece));
            const int bits = 32 + bits_for(n, 32);
            for (size_t c = 0; c + 1 < cuts.size(); c++)
                launch_locate_sort_keys(ws->locate.keys.as<uint64_t>() + cuts[c], ws->locate.sorted.as<uint64_t>() + cuts[c], cuts[c + 1] - cuts[c], bits, ws->locate.temp.ptr, ws->locate.temp.bytes, s);
            launch_locate_run_flags(ws->locate.sorted.as<uint64_t>(), total, ws->locate.flag.as<uint64_t>(), s);
            launch_scan(ws->locate.flag.as<uint64_t>(), ws->locate.rank.as<uint64_t>(), total, ws->scratch.scan_temp.ptr, ws->scratch.scan_temp.bytes, s, ws->knobs.scan_piece);
            launch_locate_compact(ws->locate.sorted.as<uint64_t>(), ws->locate.rank.as<uint64_t>(), total, ws->locate.off.as<uint64_t>(), n, ws->locate.ids.as<uint64_t>(), ws->locate.uoff.as<uint64_t>(), s);
            HIP_CHECK(hipMemcpyAsync(&kept, ws->locate.rank.as<uint64_t>() + total, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipEventRecord(ws->locate.ev[2], s));
        uint64_t words[WORDS] = {};
        HIP_CHECK(hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        if (static_cast<uint32_t>(words[0]) & LOCATE_FLAG_LOST)
            return fail(GBWT_HIP_DEVICE_ERROR, "locate: a position met neither a sampled record nor the end of a sequence (an inconsistent index)");
        HIP_CHECK(hipEventElapsedTime(&ws->locate.walk_ms, ws->locate.ev[0], ws->locate.ev[1]));
        ws->locate.sort_ms = 0;
        if (keyed) HIP_CHECK(hipEventElapsedTime(&ws->locate.sort_ms, ws->locate.ev[1], ws->locate.ev[2]));
        ws->locate.steps = words[2];
        ws->locate.compacted = keyed;                    // (a unique request without ids has no compacted offsets: its rows are the empty ones of locate.off)
        ws->locate.n = n; ws->locate.total = kept;
        if (count_steps) { ws->locate.total = total; return GBWT_HIP_OK; }
        ws->locate.timed = true;
        if (h_states != nullptr || n == 0) ws->locate.memo.store({{h_states, state_bytes}}, {unique, static_cast<int64_t>(n)});
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e, "a locate request");
    }
}

// the offsets that answer the last request
const uint64_t *result_offsets(const gbwt_hip_workspace *ws) { return (ws->locate.compacted ? ws->locate.uoff : ws->locate.off).as<uint64_t>(); }

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_locate(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const gbwt_hip_state *states, uint64_t n, int unique, uint64_t *offsets, uint64_t *ids,
                                uint64_t capacity, uint64_t *total, uint8_t *valid) {
    GBWT_HIP_GUARD_BEGIN
    if (total) *total = 0;
    if (!total || !offsets || (n && !valid)) return fail(GBWT_HIP_BAD_ARGUMENT, "null buffer");
    offsets[0] = 0;
    gbwt_hip_status st = check_request(ix, ws, states, n, unique);
    if (st != GBWT_HIP_OK) return st;
    st = locate_compute(ix, ws, states, nullptr, nullptr, n, unique);
    if (st != GBWT_HIP_OK) return st;
    *total = ws->locate.total;
    if (n == 0) return GBWT_HIP_OK;
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        hipStream_t s = ws->stream;
        HIP_CHECK(hipMemcpyAsync(offsets, result_offsets(ws), (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(valid, ws->locate.valid.ptr, n, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (!ids) return GBWT_HIP_OK;
        if (capacity < *total) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the sequence ids");
        if (*total) copy_to_host(ws, ids, ws->locate.ids.ptr, *total * sizeof(uint64_t));
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_locate_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const gbwt_hip_state *states, uint64_t n, int unique, gbwt_hip_located *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_located{nullptr, nullptr, nullptr, 0, 0};
    gbwt_hip_status st = check_request(ix, ws, states, n, unique);
    if (st != GBWT_HIP_OK) return st;
    st = locate_compute(ix, ws, states, nullptr, nullptr, n, unique);
    if (st != GBWT_HIP_OK) return st;
    *out = gbwt_hip_located{result_offsets(ws), ws->locate.ids.as<uint64_t>(), ws->locate.valid.as<uint8_t>(), ws->locate.total, n};
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_locate_states_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const gbwt_hip_state *d_states, const uint8_t *d_valid, uint64_t n, int unique,
                                              gbwt_hip_located *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_located{nullptr, nullptr, nullptr, 0, 0};
    gbwt_hip_status st = check_request(ix, ws, d_states, n, unique);
    if (st != GBWT_HIP_OK) return st;
    st = locate_compute(ix, ws, nullptr, d_states, d_valid, n, unique);
    if (st != GBWT_HIP_OK) return st;
    *out = gbwt_hip_located{result_offsets(ws), ws->locate.ids.as<uint64_t>(), ws->locate.valid.as<uint8_t>(), ws->locate.total, n};
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_locate_positions(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const gbwt_hip_pos *positions, uint64_t n, uint64_t *ids, uint8_t *valid) {
    GBWT_HIP_GUARD_BEGIN
    if (n && (!ids || !valid)) return fail(GBWT_HIP_BAD_ARGUMENT, "null buffer");
    const gbwt_hip_status st = check_request(ix, ws, positions, n, 0);
    if (st != GBWT_HIP_OK) return st;
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        hipStream_t s = ws->stream;
        ensure_locate(ix, ws);
        if (n == 0) return GBWT_HIP_OK;
        const DeviceIndex d = locate_view(ix);
        ws->locate.pos.reserve(n * sizeof(gbwt_hip_pos));
        ws->locate.pos_ids.reserve(n * sizeof(uint64_t));
        ws->locate.pos_valid.reserve(n);
        ws->locate.words.reserve(WORDS * sizeof(uint64_t));
        uint64_t *d_words = ws->locate.words.as<uint64_t>();
        HIP_CHECK(hipMemsetAsync(d_words, 0, WORDS * sizeof(uint64_t), s));
        HIP_CHECK(hipMemcpyAsync(ws->locate.pos.ptr, positions, n * sizeof(gbwt_hip_pos), hipMemcpyHostToDevice, s));
        launch_locate_positions(d, ix->locate.index, ws->locate.pos.as<gbwt_hip_pos>(), n, step_limit(ix), ws->locate.pos_ids.as<uint64_t>(), ws->locate.pos_valid.as<uint8_t>(),
                                reinterpret_cast<uint32_t *>(d_words), fast_steps(d), s);
        HIP_CHECK(hipGetLastError());
        uint64_t flags = 0;
        HIP_CHECK(hipMemcpyAsync(&flags, d_words, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(valid, ws->locate.pos_valid.ptr, n, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        copy_to_host(ws, ids, ws->locate.pos_ids.ptr, n * sizeof(uint64_t));
        if (static_cast<uint32_t>(flags) & LOCATE_FLAG_LOST)
            return fail(GBWT_HIP_DEVICE_ERROR, "locate: a position met neither a sampled record nor the end of a sequence (an inconsistent index)");
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e, "a locate request");
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_locate_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *sort_ms) {
    GBWT_HIP_GUARD_BEGIN
    if (!ws || !ws->locate.timed) return fail(GBWT_HIP_BAD_ARGUMENT, "no timed locate request on this workspace");
    if (walk_ms) *walk_ms = ws->locate.walk_ms;
    if (sort_ms) *sort_ms = ws->locate.sort_ms;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_locate_count_steps(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const gbwt_hip_state *states, uint64_t n, uint64_t *steps, uint64_t *positions) {
    GBWT_HIP_GUARD_BEGIN
    if (steps) *steps = 0;
    if (positions) *positions = 0;
    if (!steps || !positions) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    gbwt_hip_status st = check_request(ix, ws, states, n, 0);
    if (st != GBWT_HIP_OK) return st;
    st = locate_compute(ix, ws, states, nullptr, nullptr, n, 0, true);
    if (st != GBWT_HIP_OK) return st;
    *steps = ws->locate.steps;
    *positions = ws->locate.total;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_locate_index_info(const gbwt_hip_index *ix, gbwt_hip_locate_info *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !out) return fail(GBWT_HIP_BAD_ARGUMENT, "null argument");
    *out = gbwt_hip_locate_info{};
    if (!ix->locate.built.made()) return GBWT_HIP_OK;
    out->built = 1;
    out->interval = ix->knobs.locate_interval;
    out->sampled_records = ix->locate.sampled_records;
    out->table_positions = ix->locate.index.table_positions;
    out->end_entries = ix->locate.index.end_entries;
    out->device_bytes = ix->locate.base.bytes + ix->locate.table.bytes + ix->locate.end_keys.bytes + ix->locate.end_ids.bytes;
    out->build_ms = ix->locate.build_ms;
    out->build_launches = ix->locate.build_launches;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

}  // extern "C"
