// capi_refpos.hip -- GBZ::reference_positions over the C ABI (src/gbz.rs:600-657): which paths are reference paths (the host's metadata and
// tags, src/gbz.rs:146-196), and the positions of any list of forward paths, computed on the device by the passes of refpos.hip.
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "refpos.hpp"
#include "scan.hpp"

using namespace gbwt_hip;

namespace {

struct OutOfMemory { std::string what; };

// Growing `buffers` to `need` bytes each: what that takes beyond what they hold must be free on the device (a buffer that grows gives its
// old memory back first)
void require_fits(std::initializer_list<std::pair<const DeviceBuffer *, uint64_t>> buffers, const char *what) {
    uint64_t more = 0, back = 0, total = 0;
    for (const auto &b : buffers) { total += b.second; if (b.second > b.first->bytes) { more += b.second; back += b.first->bytes; } }
    size_t free_bytes = 0, all = 0;
    HIP_CHECK(hipMemGetInfo(&free_bytes, &all));
    if (more > static_cast<uint64_t>(free_bytes) + back)
        throw OutOfMemory{std::string(what) + " need " + std::to_string(total) + " bytes of device memory, " + std::to_string(more - back) + " more than the workspace holds for them; " +
                          std::to_string(free_bytes) + " are free"};
}

// GBZ::reference_samples_impl filtered as reference_sample_names does (src/gbz.rs:148-160, 183-196): (name, sample id) in the order of the tag
std::vector<std::pair<std::string, uint64_t>> reference_samples(const HostIndex &h, bool also_generic) {
    std::vector<std::string> names;
    if (const std::string *tag = h.tag("reference_samples")) {
        size_t at = 0;
        for (;;) {                                   // str::split(' '): an empty piece between two blanks is a piece
            const size_t blank = tag->find(' ', at);
            names.push_back(tag->substr(at, blank == std::string::npos ? std::string::npos : blank - at));
            if (blank == std::string::npos) break;
            at = blank + 1;
        }
    }
    if (also_generic) names.push_back("_gbwt_ref");
    std::vector<std::pair<std::string, uint64_t>> found;
    for (const std::string &name : names) {
        uint64_t id = 0;
        if (h.sample_names.find(name, id)) found.emplace_back(name, id);
    }
    return found;
}

// the reference paths (src/gbz.rs:609-629); throws InvalidData without metadata
std::vector<uint64_t> reference_paths(const gbwt_hip_index *ix, bool also_generic) {
    const HostIndex &h = ix->host;
    if (!h.has_metadata) throw InvalidData("reference paths need GBWT metadata");
    std::set<uint64_t> samples;
    for (const auto &s : reference_samples(h, also_generic)) samples.insert(s.second);
    std::vector<uint64_t> paths;
    if (samples.empty()) return paths;
    for (uint64_t p = 0; p < h.path_names.size(); p++)
        if (samples.count(h.path_names[p].sample)) paths.push_back(p);
    return paths;
}

uint32_t rounds_for(uint64_t positions) {
    uint32_t r = 1;
    while (r < REFPOS_MAX_ROUNDS && (uint64_t(1) << r) < positions) r++;
    return r;
}

// The positions of a list of paths, computed once into the workspace (refpos.paths, positions, total) unless it holds them already
gbwt_hip_status positions_compute(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, uint64_t interval) {
    if (!ix || !ws || ws->index != ix) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    if (n && !path_ids) return fail(GBWT_HIP_BAD_ARGUMENT, "null path_ids");
    const HostIndex &h = ix->host;
    if (!h.is_gbz) return fail(GBWT_HIP_UNSUPPORTED, "reference positions need a GBZ (node labels), this handle holds a bare GBWT");
    if ((ix->caps & GBWT_HIP_OPEN_GFA) != GBWT_HIP_OPEN_GFA || !(ix->caps & GBWT_HIP_OPEN_EXTRACT))
        return fail(GBWT_HIP_BAD_ARGUMENT, "the handle was not opened for GFA lines (GBWT_HIP_OPEN_GFA): reference positions need rows and label lengths");
    if (n > (~uint64_t(0)) / 64) return fail(GBWT_HIP_BAD_ARGUMENT, "too many paths");
    for (uint64_t k = 0; k < n; k++)
        if (path_ids[k] >= h.sequences / 2) return fail(GBWT_HIP_BAD_ARGUMENT, "path id out of range: " + std::to_string(path_ids[k]));
    if (ws->refpos.memo.matches({{path_ids, n * sizeof(uint64_t)}}, {static_cast<int64_t>(interval)})) return GBWT_HIP_OK;
    ws->refpos.memo.drop();
    ws->refpos.timed = false;
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        hipStream_t s = ws->stream;
        ws->refpos.ev.ensure();
        ws->refpos.walk_ms = ws->refpos.select_ms = ws->refpos.offsets_ms = 0;
        ws->refpos.rounds = ws->refpos.launches = 0;
        ws->refpos.total = 0;
        ws->refpos.paths.reserve(std::max<uint64_t>(n, 1) * sizeof(gbwt_hip_reference_path));
        if (n == 0) {
            ws->refpos.positions.reserve(sizeof(gbwt_hip_reference_position));
            ws->refpos.memo.store({{nullptr, 0}}, {static_cast<int64_t>(interval)});
            ws->refpos.timed = true;
            return GBWT_HIP_OK;
        }
        ensure_labels(ix);
        // 1. the rows: sequences 2 p (GBZ::path(p, Forward), support::encode_path)
        const bool segmented = ix->dev.samples != nullptr && ix->max_samples > 0 && ix->sample_counts.size() == h.sequences;
        std::vector<uint64_t> host_rows(3 * n + 1);  // sequence ids, path ids, lanes of the walk in front of every row
        uint64_t *seq_ids = host_rows.data(), *seg_first = host_rows.data() + 2 * n;
        seg_first[0] = 0;
        for (uint64_t k = 0; k < n; k++) {
            seq_ids[k] = 2 * path_ids[k];
            host_rows[n + k] = path_ids[k];
            seg_first[k + 1] = seg_first[k] + (segmented ? ix->sample_counts[seq_ids[k]] : 1u);
        }
        gbwt_hip_paths paths{};
        const gbwt_hip_status st = gbwt_hip_extract_device(ix, ws, seq_ids, n, &paths);
        if (st != GBWT_HIP_OK) return st;
        HIP_CHECK(hipEventElapsedTime(&ws->refpos.walk_ms, ws->extract.ev[0], ws->extract.ev[1]));
        const uint64_t P = paths.total;
        if (P > 0xFFFFFFFFull) return fail(GBWT_HIP_UNSUPPORTED, "the requested paths hold " + std::to_string(P) + " nodes: a request for positions is limited to 2^32 - 1");
        const RefposRows rows{paths.d_offsets, paths.d_nodes, n, P};
        const uint64_t words = (P + 1) * sizeof(uint64_t);
        const uint64_t piece = ws->knobs.scan_piece;
        const size_t tb = scan_temp_bytes(P, piece);
        require_fits({{&ws->refpos.off, words}, {&ws->refpos.mark, words}, {&ws->refpos.jump, words}, {&ws->scratch.scan_temp, tb}}, "the offsets, marks and jumps of a request for positions");
        ws->refpos.off.reserve(words); ws->refpos.mark.reserve(words); ws->refpos.jump.reserve(words);
        ws->scratch.scan_temp.reserve(tb);
        ws->refpos.rows.reserve(host_rows.size() * sizeof(uint64_t));
        ws->refpos.flags.reserve(REFPOS_FLAGS * sizeof(uint32_t));
        uint64_t *d_off = ws->refpos.off.as<uint64_t>(), *d_mark = ws->refpos.mark.as<uint64_t>(), *d_slot = ws->refpos.jump.as<uint64_t>();
        uint32_t *d_jump = ws->refpos.jump.as<uint32_t>(), *d_next = d_jump + (P + 1), *d_flags = ws->refpos.flags.as<uint32_t>();
        const uint64_t *d_rows = ws->refpos.rows.as<uint64_t>();
        HIP_CHECK(hipMemcpyAsync(ws->refpos.rows.ptr, host_rows.data(), host_rows.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(ws->refpos.flags.ptr, 0, REFPOS_FLAGS * sizeof(uint32_t), s));
        HIP_CHECK(hipEventRecord(ws->refpos.ev[0], s));
        // 2. bases in front of every position
        launch_refpos_lengths(rows, labels_of(ix), d_mark, s);
        launch_scan(d_mark, d_off, P, ws->scratch.scan_temp.ptr, tb, s, piece);
        // 3. successors, 4. the greedy chain of every row by pointer doubling
        launch_refpos_succ(rows, d_off, interval, d_jump, s);
        HIP_CHECK(hipMemsetAsync(d_mark, 0, words, s));
        launch_refpos_first_marks(rows, d_mark, s);
        const uint32_t rounds = rounds_for(P);
        for (uint32_t t = 0; t < rounds; t++) { launch_refpos_round(d_mark, d_jump, d_next, P, d_flags, t, s); std::swap(d_jump, d_next); }
        // 5. slots (over the jump arrays, which nobody reads any more)
        launch_scan(d_mark, d_slot, P, ws->scratch.scan_temp.ptr, tb, s, piece);
        uint64_t total = 0;
        uint32_t flags[REFPOS_FLAGS] = {};
        HIP_CHECK(hipMemcpyAsync(&total, d_slot + P, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipEventRecord(ws->refpos.ev[1], s));
        HIP_CHECK(hipStreamSynchronize(s));          // the one wait in front of the results: the total sizes them
        HIP_CHECK(hipGetLastError());
        // lengths, two scans (one launch per piece of GBWT_HIP_SCAN_PIECE positions: ceil(P / piece) each), successors, first marks, the rounds, paths, walk
        ws->refpos.launches = static_cast<uint32_t>((P ? 1 : 0) + 2 * scan_launches(P, piece) + 2 + rounds + 2);
        for (uint32_t t = 0; t < rounds; t++) ws->refpos.rounds += flags[t] != 0 ? 1u : 0u;
        if (total > (~uint64_t(0)) / sizeof(gbwt_hip_reference_position)) return fail(GBWT_HIP_CAPACITY, "too many positions for device memory");
        const uint64_t result_bytes = std::max<uint64_t>(total, 1) * sizeof(gbwt_hip_reference_position);
        require_fits({{&ws->refpos.positions, result_bytes}}, "the positions of the request");
        ws->refpos.positions.reserve(result_bytes);
        // 6. the walk that carries the in-record offsets
        DeviceIndex d = ix->dev;
        d.sample_stride = 1; d.sample_part = 0; d.sample_parts = 0;
        RefposWalk w{};
        w.seq_ids = d_rows; w.seg_first = d_rows + 2 * n; w.walkers = seg_first[n]; w.segmented = segmented ? 1u : 0u;
        w.off = d_off; w.slot = d_slot; w.out = ws->refpos.positions.as<gbwt_hip_reference_position>(); w.flags = d_flags;
        launch_refpos_paths(rows, d_rows + n, d_off, d_slot, ws->refpos.paths.as<gbwt_hip_reference_path>(), s);
        launch_refpos_walk(d, rows, w, d.desc_raw != nullptr && d.blocks != nullptr, s);
        HIP_CHECK(hipEventRecord(ws->refpos.ev[2], s));
        HIP_CHECK(hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventElapsedTime(&ws->refpos.select_ms, ws->refpos.ev[0], ws->refpos.ev[1]));
        HIP_CHECK(hipEventElapsedTime(&ws->refpos.offsets_ms, ws->refpos.ev[1], ws->refpos.ev[2]));
        ws->refpos.timed = true;
        if (flags[REFPOS_FLAG_MISMATCH] != 0)
            return fail(GBWT_HIP_DEVICE_ERROR, "a walker of the positions met another node than the extracted row holds, or no successor inside a row (an inconsistent index)");
        ws->refpos.total = total;
        ws->refpos.memo.store({{path_ids, n * sizeof(uint64_t)}}, {static_cast<int64_t>(interval)});
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const OutOfMemory &e) {
        return fail(GBWT_HIP_CAPACITY, e.what);
    } catch (const HipError &e) {
        return status_of(e, "a request for positions");
    }
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_reference_sample_names(const gbwt_hip_index *ix, int also_generic, char *out, uint64_t capacity, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !total) return fail(GBWT_HIP_BAD_ARGUMENT, "null index / total");
    *total = 0;
    if (!ix->host.has_metadata) return GBWT_HIP_OK;
    std::string text;
    for (const auto &s : reference_samples(ix->host, also_generic != 0)) { text += s.first; text += '\n'; }
    *total = text.size();
    if (!out) return GBWT_HIP_OK;
    if (capacity < text.size()) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the reference sample names");
    std::memcpy(out, text.data(), text.size());
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_reference_paths(const gbwt_hip_index *ix, int also_generic, uint64_t *out_ids, uint64_t capacity, uint64_t *count) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !count) return fail(GBWT_HIP_BAD_ARGUMENT, "null index / count");
    *count = 0;
    try {
        const std::vector<uint64_t> paths = reference_paths(ix, also_generic != 0);
        *count = paths.size();
        if (!out_ids) return GBWT_HIP_OK;
        if (capacity < paths.size()) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the reference paths");
        std::copy(paths.begin(), paths.end(), out_ids);
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_path_positions_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, uint64_t interval,
                                               const gbwt_hip_reference_path **d_paths, const gbwt_hip_reference_position **d_positions, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (total) *total = 0;
    if (d_paths) *d_paths = nullptr;
    if (d_positions) *d_positions = nullptr;
    if (!d_paths || !d_positions || !total) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    const gbwt_hip_status st = positions_compute(ix, ws, path_ids, n, interval);
    if (st != GBWT_HIP_OK) return st;
    *d_paths = ws->refpos.paths.as<gbwt_hip_reference_path>();
    *d_positions = ws->refpos.positions.as<gbwt_hip_reference_position>();
    *total = ws->refpos.total;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_path_positions(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, uint64_t interval,
                                        gbwt_hip_reference_path *out_paths, gbwt_hip_reference_position *out_positions, uint64_t positions_capacity, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (total) *total = 0;
    if (!total) return fail(GBWT_HIP_BAD_ARGUMENT, "null total");
    const gbwt_hip_status st = positions_compute(ix, ws, path_ids, n, interval);
    if (st != GBWT_HIP_OK) return st;
    *total = ws->refpos.total;
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        if (out_paths && n) {
            HIP_CHECK(hipMemcpyAsync(out_paths, ws->refpos.paths.ptr, n * sizeof(gbwt_hip_reference_path), hipMemcpyDeviceToHost, ws->stream));
            HIP_CHECK(hipStreamSynchronize(ws->stream));
        }
        if (!out_positions) return GBWT_HIP_OK;
        if (positions_capacity < ws->refpos.total) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the positions");
        if (ws->refpos.total) copy_to_host(ws, out_positions, ws->refpos.positions.ptr, ws->refpos.total * sizeof(gbwt_hip_reference_position));
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_reference_positions(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, uint64_t interval, gbwt_hip_reference_path *out_paths, uint64_t paths_capacity,
                                             uint64_t *n_paths, gbwt_hip_reference_position *out_positions, uint64_t positions_capacity, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (n_paths) *n_paths = 0;
    if (total) *total = 0;
    if (!ix || !ws || ws->index != ix || !n_paths || !total) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace / counts");
    if (!ix->host.is_gbz) return fail(GBWT_HIP_UNSUPPORTED, "reference positions need a GBZ (node labels), this handle holds a bare GBWT");
    std::vector<uint64_t> ids;
    try {
        ids = reference_paths(ix, true);
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    }
    *n_paths = ids.size();
    if (out_paths && paths_capacity < ids.size()) {
        const gbwt_hip_status st = gbwt_hip_path_positions(ix, ws, ids.data(), ids.size(), interval, nullptr, nullptr, 0, total);
        return st != GBWT_HIP_OK ? st : fail(GBWT_HIP_CAPACITY, "output capacity too small for the reference paths");
    }
    return gbwt_hip_path_positions(ix, ws, ids.data(), ids.size(), interval, out_paths, out_positions, positions_capacity, total);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_positions_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *select_ms, float *offsets_ms) {
    GBWT_HIP_GUARD_BEGIN
    if (!ws || !ws->refpos.timed) return fail(GBWT_HIP_BAD_ARGUMENT, "no timed request for positions on this workspace");
    if (walk_ms) *walk_ms = ws->refpos.walk_ms;
    if (select_ms) *select_ms = ws->refpos.select_ms;
    if (offsets_ms) *offsets_ms = ws->refpos.offsets_ms;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_positions_rounds(const gbwt_hip_workspace *ws, uint32_t *rounds, uint32_t *launches) {
    GBWT_HIP_GUARD_BEGIN
    if (!ws || !ws->refpos.timed) return fail(GBWT_HIP_BAD_ARGUMENT, "no timed request for positions on this workspace");
    if (rounds) *rounds = ws->refpos.rounds;
    if (launches) *launches = ws->refpos.launches;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

}  // extern "C"
