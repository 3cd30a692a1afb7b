// capi_lines.hip -- the C ABI of gbunzip's GFA text (src/bin/gbunzip.rs:193-550) on top of the device extraction: gbwt_hip_path_lines*,
// gbwt_hip_segment_paths and the whole-file writer gbwt_hip_write_gfa*.
//
// P- and W-lines are where the LF-steps go, so they are produced on the device: the forward sequences of a batch of paths are extracted
// (k_walk_*), every line is sized -- from the line cache the open left in the handle, or by a pass over the rows -- with its header taken
// from the per-path tables built at open (open_lines.hip), and a formatting kernel writes headers, node tokens and trailers (lines.hip).
// The decisions of a request are arithmetic in lines_plan.hpp; nothing is launched from here but through the wrappers of lines.hpp.
// With a node-to-segment translation the tokens are segment names; a path that is not a concatenation of whole segments makes the
// reference's iterator stop at an input-dependent place: the device flags such paths and the host formats them with the reference's state
// machine (gfa_host.cpp: host_segment_path), from the node ids the device extracted.
// The H-, S- and L-lines of a whole file are written by the host (gfa_host.cpp: host_graph_lines) while the first batch of paths is walked;
// gbwt_hip_graph_lines (capi_topology.hip) makes the same text on the device.
#include <fcntl.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "batch_writer.hpp"
#include "capi_internal.hpp"
#include "gfa_host.hpp"
#include "lines.hpp"
#include "lines_plan.hpp"
#include "scan.hpp"

using namespace gbwt_hip;

namespace {

const char *const GENERIC_SAMPLE = "_gbwt_ref";  // src/lib.rs

void require_gfa_capable(const gbwt_hip_index *ix) {
    if (!(ix->caps & GBWT_HIP_OPEN_GFA)) throw InvalidData("the handle was not opened for GFA lines (GBWT_HIP_OPEN_GFA)");
    if (!ix->host.is_gbz) throw InvalidData("GFA lines need a GBZ (graph + metadata), this handle holds a bare GBWT");
    if (!ix->host.has_metadata) throw InvalidData("GFA lines need path metadata");
}

SegmentTables segment_tables(const gbwt_hip_index *ix) {
    return SegmentTables{ix->seg_of.as<uint32_t>(), ix->seg_start.as<uint32_t>(), ix->seg_name_off.as<uint64_t>(), ix->seg_names.as<uint8_t>(),
                         ix->seg_seq_len.as<uint64_t>(), ix->node_real.as<uint8_t>(), ix->host.mapping_len};
}

// Rows that are not concatenations of whole segments (valid[k] == 0): the reference's iterator stops somewhere inside them.  Their node
// ids come to the host (offs: the host's copy of the row offsets) and the iterator is replayed on them; row(k, tokens, seq_len) takes the result.
template <class Row>
void replay_broken_rows(const HostIndex &h, const gbwt_hip_paths &paths, const std::vector<uint64_t> &offs, const std::vector<uint8_t> &valid, Row row) {
    std::vector<uint32_t> nodes;
    std::vector<std::pair<uint64_t, bool>> tokens;
    for (uint64_t k = 0; k < valid.size(); k++) {
        if (valid[k]) continue;
        nodes.resize(offs[k + 1] - offs[k]);
        if (!nodes.empty()) HIP_CHECK(hipMemcpy(nodes.data(), paths.d_nodes + offs[k], nodes.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint64_t seq_len = 0;
        host_segment_path(h, nodes.data(), nodes.size(), tokens, seq_len);
        row(k, tokens, seq_len);
    }
}

// ---- the lines of a batch of paths ----------------------------------------------------------------------------------------------------
// Formatted ONCE into device memory (the text buffer of `slot`: ws->lines.text or text2; line k at [line_start[k], line_start[k + 1]),
// offsets also on the device in ws->lines.b).  The request is remembered in the workspace: the fill call that follows a size query, and the
// copy-out of gbwt_hip_path_lines after gbwt_hip_path_lines_device, find the text there.
//
// Everything between the walk and the text stays on the device (round 4): chunk counts, per-chunk sizes, their scans, the line lengths --
// headers included, from the per-path header tables built at open and the end coordinate the walk yields -- and the scan that places the
// lines.  The host waits ONCE, for the total that sizes the text buffer (and, with a node-to-segment translation, for the flags of the
// paths it has to replay).  Until round 3 it built every header itself, between two more synchronisations: 0.9 ms per request whatever its
// size -- config 4's 32 000 walks in rounds of 512 spent 58 ms there.
//
// What the steps of one request hand on to each other:
struct LinesRequest {
    const gbwt_hip_index *ix;
    gbwt_hip_workspace *ws;
    const uint64_t *path_ids;
    uint64_t n;
    int mode, slot;
    LinesRequest(const gbwt_hip_index *index, gbwt_hip_workspace *workspace, const uint64_t *ids, uint64_t count, int line_mode, int text_slot)
        : ix(index), ws(workspace), path_ids(ids), n(count), mode(line_mode), slot(text_slot) {}
    int p_lines = 0;
    bool translated = false;
    // extract
    gbwt_hip_paths paths{};
    hipStream_t s = nullptr;
    const uint64_t *d_seq_ids = nullptr;
    // size
    LineSizing sizing = LineSizing::Plain;
    size_t tb = 0;
    ChunkedRows rows{};
    LineHeaders hdr{};
    LineCache cache{};
    uint64_t *d_line_len = nullptr, *d_line_end = nullptr, *d_line_start = nullptr, *d_text_before = nullptr;
    uint8_t *d_valid = nullptr;
    // wait
    uint64_t total = 0;
    std::vector<uint8_t> valid;
    // replay: the lines the host made (empty: none) and where every line starts with their lengths put in
    std::vector<std::string> host_lines;
    std::vector<uint64_t> line_start;
};

void lines_remember(const LinesRequest &r) {
    LinesState &l = r.ws->lines;
    l.memo.store({{r.path_ids, r.n * sizeof(uint64_t)}}, {r.mode, r.slot});
    l.n = r.n; l.slot = r.slot;
}

// 0. arguments and memo.  `answered`: the status is the answer of the request -- refused, found in the workspace, or no paths asked for.
gbwt_hip_status lines_begin(LinesRequest &r, bool &answered) {
    answered = true;
    if (!r.ix || !r.ws || r.ws->index != r.ix) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    if (r.n && !r.path_ids) return fail(GBWT_HIP_BAD_ARGUMENT, "null path_ids");
    if (r.mode < 0 || r.mode > 2) return fail(GBWT_HIP_BAD_ARGUMENT, "mode must be 0 (P-lines), 1 (W-lines) or 2 (P-lines with PanSN names)");
    r.p_lines = r.mode != 1 ? 1 : 0;
    LinesState &l = r.ws->lines;
    if (l.memo.matches({{r.path_ids, r.n * sizeof(uint64_t)}}, {r.mode, r.slot})) return GBWT_HIP_OK;
    l.memo.drop();
    require_gfa_capable(r.ix);
    const HostIndex &h = r.ix->host;
    r.translated = h.has_translation && !h.segment_starts.empty();
    for (uint64_t k = 0; k < r.n; k++)
        if (r.path_ids[k] >= h.path_names.size()) return fail(GBWT_HIP_BAD_ARGUMENT, "path id out of range");
    l.total = 0;
    if (r.n == 0) {
        lines_remember(r);
        return GBWT_HIP_OK;
    }
    answered = false;
    return GBWT_HIP_OK;
}

// 1. forward sequences of the paths (GBZ::path(id, Forward), src/bin/gbunzip.rs:462, 532)
gbwt_hip_status lines_extract(LinesRequest &r) {
    std::vector<uint64_t> seq_ids(r.n);
    for (uint64_t k = 0; k < r.n; k++) seq_ids[k] = 2 * r.path_ids[k];
    const gbwt_hip_status st = gbwt_hip_extract_device(r.ix, r.ws, seq_ids.data(), r.n, &r.paths);
    if (st != GBWT_HIP_OK) return st;
    HIP_CHECK(hipSetDevice(r.ix->device));
    r.s = r.ws->stream;
    r.ws->lines.ev.ensure();
    HIP_CHECK(hipEventRecord(r.ws->lines.ev[0], r.s));
    r.d_seq_ids = r.ws->extract.seq_ids.as<uint64_t>();         // (the extraction has left the ids on the device)
    return GBWT_HIP_OK;
}

// 2. size of every line: chunks of LINE_CHUNK positions, a wave per chunk, scans over the chunks -- or, from the line cache of the index
// (filled at open), without reading a node id before the formatter does -- and the scan that places the lines
gbwt_hip_status lines_size(LinesRequest &r) {
    const gbwt_hip_index *ix = r.ix;
    gbwt_hip_workspace *ws = r.ws;
    const HostIndex &h = ix->host;
    const uint64_t n = r.n;
    const ChunksCap cap = chunks_cap(r.paths.total, n);
    if (cap.refused) return fail(GBWT_HIP_UNSUPPORTED, LINES_TOO_MANY_CHUNKS);
    const LinesLayout at = lines_layout(n, cap.chunks);
    const uint64_t piece = ws->knobs.scan_piece;
    r.tb = scan_temp_bytes(std::max(n, cap.chunks), piece);
    ws->scratch.a.reserve(at.a_bytes);
    ws->lines.b.reserve((n + 1) * sizeof(uint64_t));
    ws->scratch.chunk_first.reserve(at.chunk_first_bytes);
    ws->scratch.chunks.reserve(at.chunks_bytes);
    ws->scratch.scan_temp.reserve(r.tb);
    ws->lines.valid.reserve(std::max<uint64_t>(n, 16));
    void *const a = ws->scratch.a.ptr, *const first = ws->scratch.chunk_first.ptr, *const chunks = ws->scratch.chunks.ptr, *const temp = ws->scratch.scan_temp.ptr;
    r.d_line_len = scratch_at<uint64_t>(a, at.line_len); r.d_line_end = scratch_at<uint64_t>(a, at.line_end);
    r.d_line_start = ws->lines.b.as<uint64_t>();
    uint64_t *const d_chunk_first = scratch_at<uint64_t>(first, at.chunk_first), *const d_chunk_counts = scratch_at<uint64_t>(first, at.chunk_counts);
    uint64_t *const d_chunk_text = scratch_at<uint64_t>(chunks, at.chunk_text), *const d_chunk_seq = scratch_at<uint64_t>(chunks, at.chunk_seq);
    uint64_t *const d_chunk_bad = scratch_at<uint64_t>(chunks, at.chunk_bad), *const d_seq_before = scratch_at<uint64_t>(chunks, at.seq_before);
    uint64_t *const d_bad_before = scratch_at<uint64_t>(chunks, at.bad_before);
    uint32_t *const d_chunk_path = scratch_at<uint32_t>(chunks, at.chunk_path);
    r.d_text_before = scratch_at<uint64_t>(chunks, at.text_before);
    r.d_valid = r.translated ? ws->lines.valid.as<uint8_t>() : nullptr;
    r.hdr = LineHeaders{ix->line_prefix[r.mode].as<uint8_t>(), ix->line_prefix_off[r.mode].as<uint64_t>(), r.mode == 1 ? ix->line_fragment.as<uint32_t>() : nullptr};
    r.cache = LineCache{ix->lc_chunk_first.as<uint64_t>(), ix->lc_text.as<uint64_t>(), ix->lc_path.as<uint64_t>()};
    r.sizing = line_sizing(r.translated, ix->lc_state);
    r.rows = ChunkedRows{r.paths.d_offsets, r.paths.d_nodes, n, d_chunk_first, d_chunk_path, cap.chunks};
    hipStream_t s = r.s;
    launch_chunk_plan(r.paths.d_offsets, n, cap.chunks, d_chunk_counts, d_chunk_first, d_chunk_path, temp, r.tb, s, piece);
    if (r.sizing == LineSizing::Cached) {
        launch_line_sizes_cached(r.paths.d_offsets, r.d_seq_ids, n, r.cache, r.hdr, r.p_lines, r.d_line_len, r.d_line_end, s);
    } else {
        if (r.sizing == LineSizing::Translated) {
            launch_chunk_stats_segments(r.rows, segment_tables(ix), r.p_lines, d_chunk_text, d_chunk_seq, d_chunk_bad, s);
            launch_scan(d_chunk_bad, d_bad_before, cap.chunks, temp, r.tb, s, piece);
        } else {
            launch_chunk_stats(r.rows, ix->label_len.as<uint32_t>(), static_cast<uint64_t>(h.sequences_labels.size()), static_cast<uint32_t>(h.alphabet_offset + 1), r.p_lines,
                               d_chunk_text, d_chunk_seq, s);
        }
        launch_scan(d_chunk_text, r.d_text_before, cap.chunks, temp, r.tb, s, piece);
        launch_scan(d_chunk_seq, d_seq_before, cap.chunks, temp, r.tb, s, piece);
        launch_line_sizes(r.d_seq_ids, d_chunk_first, n, r.d_text_before, d_seq_before, r.translated ? d_bad_before : nullptr, r.hdr, r.p_lines, r.d_line_len, r.d_line_end,
                          r.d_valid, s);
    }
    launch_scan(r.d_line_len, r.d_line_start, n, temp, r.tb, s, piece);
    return GBWT_HIP_OK;
}

// 3. the one wait of a request: for the total that sizes the text, and with a translation for the flags of the paths
void lines_wait(LinesRequest &r) {
    HIP_CHECK(hipMemcpyAsync(&r.total, r.d_line_start + r.n, sizeof(uint64_t), hipMemcpyDeviceToHost, r.s));
    if (r.translated) { r.valid.resize(r.n); HIP_CHECK(hipMemcpyAsync(r.valid.data(), r.d_valid, r.n, hipMemcpyDeviceToHost, r.s)); }
    HIP_CHECK(hipStreamSynchronize(r.s));
    HIP_CHECK(hipGetLastError());
}

// 3b. paths that are not concatenations of whole segments: the host replays the reference's iterator on the extracted node ids, makes
// their lines, puts the lengths of those lines in and places the lines again
void lines_replay(LinesRequest &r) {
    if (std::find(r.valid.begin(), r.valid.end(), uint8_t(0)) == r.valid.end()) return;
    const HostIndex &h = r.ix->host;
    const uint64_t n = r.n;
    r.host_lines.resize(n);
    std::vector<uint64_t> offs(n + 1), lens(n);
    HIP_CHECK(hipMemcpy(offs.data(), r.paths.d_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(lens.data(), r.d_line_len, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    const std::vector<char> &prefix = r.ix->host_line_prefix[r.mode];
    const std::vector<uint64_t> &prefix_off = r.ix->host_line_prefix_off[r.mode];
    replay_broken_rows(h, r.paths, offs, r.valid, [&](uint64_t k, const std::vector<std::pair<uint64_t, bool>> &tokens, uint64_t seq_len) {
        const uint64_t path = r.path_ids[k];
        std::string &line = r.host_lines[k];
        line.assign(prefix.data() + prefix_off[path], prefix_off[path + 1] - prefix_off[path]);
        if (r.mode == 1) line += std::to_string(static_cast<uint64_t>(h.path_names[path].fragment) + seq_len) + "\t";
        for (size_t j = 0; j < tokens.size(); j++) {
            const std::string name = h.segment_names.str(tokens[j].first);
            if (r.p_lines) line += (j ? "," : "") + name + (tokens[j].second ? "-" : "+");
            else line += (tokens[j].second ? "<" : ">") + name;
        }
        line += r.p_lines ? "\t*\n" : "\n";
        lens[k] = line.size();
    });
    r.line_start.assign(n + 1, 0);
    for (uint64_t k = 0; k < n; k++) r.line_start[k + 1] = r.line_start[k] + lens[k];
    r.total = r.line_start[n];
    HIP_CHECK(hipMemcpyAsync(r.d_line_start, r.line_start.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, r.s));
}

// 4. format on the device; the lines the host had to replay are copied into their places
void lines_format(LinesRequest &r) {
    gbwt_hip_workspace *ws = r.ws;
    DeviceBuffer &text = r.slot == 0 ? ws->lines.text : ws->lines.text2;
    text.reserve(std::max<uint64_t>(r.total, 16));
    if (r.translated)
        launch_format_chunks_segments(r.rows, r.d_text_before, segment_tables(r.ix), r.p_lines, r.d_valid, r.d_line_start, r.d_seq_ids, r.hdr, r.d_line_end, text.as<uint8_t>(), r.s);
    else {
        ws->scratch.plan.reserve(r.rows.chunks_cap * sizeof(ChunkPlan));
        launch_plan_chunks(r.rows, r.d_text_before, r.p_lines, r.d_line_start, r.d_seq_ids, r.hdr, r.d_line_end,
                           r.sizing == LineSizing::Cached ? r.cache : LineCache{nullptr, nullptr, nullptr}, ws->scratch.plan.as<ChunkPlan>(), r.s);
        launch_format_chunks(r.rows, ws->scratch.plan.as<ChunkPlan>(), r.p_lines, r.d_seq_ids, r.hdr, r.d_line_end, text.as<uint8_t>(), r.s);
    }
    HIP_CHECK(hipGetLastError());
    for (uint64_t k = 0; k < r.host_lines.size(); k++)
        if (!r.valid[k] && !r.host_lines[k].empty())
            HIP_CHECK(hipMemcpyAsync(text.as<char>() + r.line_start[k], r.host_lines[k].data(), r.host_lines[k].size(), hipMemcpyHostToDevice, r.s));
}

// 5. the text is there when the call returns (and the host's lines may go); the workspace remembers the request
void lines_finish(LinesRequest &r) {
    LinesState &l = r.ws->lines;
    HIP_CHECK(hipEventRecord(l.ev[1], r.s));
    HIP_CHECK(hipStreamSynchronize(r.s));
    l.timed = true;
    l.total = r.total;
    lines_remember(r);
}

gbwt_hip_status path_lines_compute(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int mode, int slot = 0) {
    LinesRequest r(ix, ws, path_ids, n, mode, slot);
    try {
        bool answered = false;
        gbwt_hip_status st = lines_begin(r, answered);
        if (answered) return st;
        if ((st = lines_extract(r)) != GBWT_HIP_OK) return st;
        if ((st = lines_size(r)) != GBWT_HIP_OK) return st;
        lines_wait(r);
        if (r.translated) lines_replay(r);
        lines_format(r);
        lines_finish(r);
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const HipError &e) {
        return status_of(e);
    }
}

// gbwt_hip_path_lines: formats (or finds) the lines and copies them to the host buffer -- over several threads with pinned staging
// buffers (copy_to_host), as the CSR of gbwt_hip_extract is: one pageable hipMemcpy moved a gigabyte of W-lines at 2.4 GB/s.
gbwt_hip_status path_lines_impl(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int mode, char *out, uint64_t capacity,
                                uint64_t *total) {
    if (!total) return fail(GBWT_HIP_BAD_ARGUMENT, "null total");
    *total = 0;
    const gbwt_hip_status st = path_lines_compute(ix, ws, path_ids, n, mode);
    if (st != GBWT_HIP_OK) return st;
    *total = ws->lines.total;
    if (!out || *total == 0) return GBWT_HIP_OK;
    if (capacity < *total) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the lines");
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        copy_to_host(ws, out, ws->lines.text.ptr, *total);
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
}

// ---- GBZ::segment_path as data (src/gbz.rs:477-489) -----------------------------------------------------------------------------------
// Sizing of a segment tokens request: tokens and flag of every chunk, their scans, tokens and validity of every row.  Returns the rows
// and their chunks for the fill; `at` says where the arrays lie.
ChunkedRows segment_tokens_size(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const gbwt_hip_paths &paths, uint64_t n, uint64_t cap, const TokensLayout &at, hipStream_t s) {
    const uint64_t piece = ws->knobs.scan_piece;
    const size_t tb = scan_temp_bytes(std::max(n, cap), piece);
    ws->scratch.a.reserve(at.a_bytes);
    ws->scratch.chunk_first.reserve(at.chunk_first_bytes);
    ws->scratch.chunks.reserve(at.chunks_bytes);
    ws->scratch.scan_temp.reserve(tb);
    ws->lines.valid.reserve(std::max<uint64_t>(n, 16));
    void *const first = ws->scratch.chunk_first.ptr, *const chunks = ws->scratch.chunks.ptr, *const temp = ws->scratch.scan_temp.ptr;
    uint64_t *const d_chunk_first = scratch_at<uint64_t>(first, at.chunk_first), *const d_chunk_counts = scratch_at<uint64_t>(first, at.chunk_counts);
    uint64_t *const d_chunk_tokens = scratch_at<uint64_t>(chunks, at.chunk_tokens), *const d_chunk_bad = scratch_at<uint64_t>(chunks, at.chunk_bad);
    uint64_t *const d_tokens_before = scratch_at<uint64_t>(chunks, at.tokens_before), *const d_bad_before = scratch_at<uint64_t>(chunks, at.bad_before);
    uint32_t *const d_chunk_path = scratch_at<uint32_t>(chunks, at.chunk_path);
    const ChunkedRows rows{paths.d_offsets, paths.d_nodes, n, d_chunk_first, d_chunk_path, cap};
    launch_chunk_plan(paths.d_offsets, n, cap, d_chunk_counts, d_chunk_first, d_chunk_path, temp, tb, s, piece);
    launch_segment_chunk_tokens(rows, segment_tables(ix), d_chunk_tokens, d_chunk_bad, s);
    launch_scan(d_chunk_tokens, d_tokens_before, cap, temp, tb, s, piece);
    launch_scan(d_chunk_bad, d_bad_before, cap, temp, tb, s, piece);
    launch_segment_row_tokens(d_chunk_first, n, d_tokens_before, d_bad_before, scratch_at<uint64_t>(ws->scratch.a.ptr, at.row_tokens), ws->lines.valid.as<uint8_t>(), s);
    return rows;
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_path_lines(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int mode,
                                    char *out, uint64_t capacity, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    return path_lines_impl(ix, ws, path_ids, n, mode, out, capacity, total);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_path_lines_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int mode,
                                           gbwt_hip_lines *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_lines{nullptr, nullptr, 0, 0};
    const gbwt_hip_status st = path_lines_compute(ix, ws, path_ids, n, mode);
    if (st != GBWT_HIP_OK) return st;
    out->d_text = n ? ws->lines.text.as<char>() : nullptr;
    out->d_line_offsets = n ? ws->lines.b.as<uint64_t>() : nullptr;
    out->total = ws->lines.total;
    out->n = n;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_segment_paths(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *seq_ids, uint64_t n, uint64_t *out_offsets, uint64_t *out_tokens,
                                       uint64_t capacity, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !ws || ws->index != ix || !total) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace / total");
    if (n && (!seq_ids || !out_offsets)) return fail(GBWT_HIP_BAD_ARGUMENT, "null seq_ids / out_offsets");
    *total = 0;
    const HostIndex &h = ix->host;
    if (!(ix->caps & GBWT_HIP_OPEN_GFA)) return fail(GBWT_HIP_BAD_ARGUMENT, "the handle was not opened for GFA lines (GBWT_HIP_OPEN_GFA): the node-to-segment tables belong to that group");
    if (!h.is_gbz || !h.has_translation || h.segment_starts.empty())
        return fail(GBWT_HIP_BAD_ARGUMENT, "no node-to-segment translation (GBZ::segment_path returns None, src/gbz.rs:477-480)");
    if (out_offsets) out_offsets[0] = 0;
    if (n == 0) return GBWT_HIP_OK;
    try {
        gbwt_hip_paths paths{};
        const gbwt_hip_status st = gbwt_hip_extract_device(ix, ws, seq_ids, n, &paths);
        if (st != GBWT_HIP_OK) return st;
        ws->lines.memo.drop();                                           // (the line buffers of the workspace are used below)
        HIP_CHECK(hipSetDevice(ix->device));
        hipStream_t s = ws->stream;
        const ChunksCap cap = chunks_cap(paths.total, n);
        if (cap.refused) return fail(GBWT_HIP_UNSUPPORTED, TOKENS_TOO_MANY_CHUNKS);
        const TokensLayout at = tokens_layout(n, cap.chunks);
        const ChunkedRows rows = segment_tokens_size(ix, ws, paths, n, cap.chunks, at, s);
        uint64_t *const d_row_tokens = scratch_at<uint64_t>(ws->scratch.a.ptr, at.row_tokens), *const d_row_start = scratch_at<uint64_t>(ws->scratch.a.ptr, at.row_start);
        uint8_t *const d_valid = ws->lines.valid.as<uint8_t>();
        std::vector<uint64_t> counts(n), offs(n + 1);
        std::vector<uint8_t> valid(n);
        HIP_CHECK(hipMemcpyAsync(counts.data(), d_row_tokens, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(valid.data(), d_valid, n, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(offs.data(), paths.d_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        std::vector<std::vector<std::pair<uint64_t, bool>>> replayed(n);
        replay_broken_rows(h, paths, offs, valid, [&](uint64_t k, const std::vector<std::pair<uint64_t, bool>> &tokens, uint64_t) {
            replayed[k] = tokens;
            counts[k] = tokens.size();
        });
        out_offsets[0] = 0;
        for (uint64_t k = 0; k < n; k++) out_offsets[k + 1] = out_offsets[k] + counts[k];
        *total = out_offsets[n];
        if (!out_tokens || *total == 0) return GBWT_HIP_OK;               // the size query
        if (capacity < *total) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the segment tokens");
        ws->lines.text.reserve(std::max<uint64_t>(*total, 1) * sizeof(uint64_t));
        HIP_CHECK(hipMemcpyAsync(d_row_start, out_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        launch_segment_fill_tokens(rows, scratch_at<uint64_t>(ws->scratch.chunks.ptr, at.tokens_before), segment_tables(ix), d_valid, d_row_start, ws->lines.text.as<uint64_t>(), s);
        HIP_CHECK(hipMemcpyAsync(out_tokens, ws->lines.text.ptr, *total * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        for (uint64_t k = 0; k < n; k++)
            for (size_t j = 0; j < replayed[k].size(); j++) out_tokens[out_offsets[k] + j] = (replayed[k][j].first << 1) | (replayed[k][j].second ? 1u : 0u);
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_lines_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *format_ms) {
    GBWT_HIP_GUARD_BEGIN
    if (!ws || !ws->lines.timed || !ws->extract.timed) return fail(GBWT_HIP_BAD_ARGUMENT, "no timed GFA lines request on this workspace");
    float a = 0, b = 0;
    if (hipEventElapsedTime(&a, ws->extract.ev[0], ws->extract.ev[1]) != hipSuccess || hipEventElapsedTime(&b, ws->lines.ev[0], ws->lines.ev[1]) != hipSuccess)
        return fail(GBWT_HIP_DEVICE_ERROR, "hipEventElapsedTime failed");
    if (walk_ms) *walk_ms = a;
    if (format_ms) *format_ms = b;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_write_gfa(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const char *path) {
    return gbwt_hip_write_gfa_mode(ix, ws, path, GBWT_HIP_PATHS_DEFAULT);
}

// The reference builds the lines of the paths in parallel and hands them to a writer under a mutex, behind an 8 MiB BufWriter
// (src/bin/gbunzip.rs:96, 205-226, 421-434).  Here: batches bounded by BYTES of text (GBWT_HIP_GFA_BATCH_MIB, default 1 GiB: config 4's
// 32 000 walks are four batches, the headline's 5 000 paths of 4.5 MB each a few hundred), formatted on the device into two text
// buffers in turn, while a writer thread moves the previous batch to the file through pinned buffers (batch_writer.hpp) -- and
// writes the H-, S- and L-lines of the graph, host work, while the first batch is walked.
gbwt_hip_status gbwt_hip_write_gfa_mode(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const char *path, int path_mode) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !ws || ws->index != ix || !path) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    if (path_mode < GBWT_HIP_PATHS_DEFAULT || path_mode > GBWT_HIP_PATHS_REF_ONLY) return fail(GBWT_HIP_BAD_ARGUMENT, "unknown path mode");
    try {
        require_gfa_capable(ix);
        const HostIndex &h = ix->host;
        const bool translated = h.has_translation && !h.segment_starts.empty();
        PositionalFile file;
        file.fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (file.fd < 0) return fail(GBWT_HIP_IO_ERROR, std::string("cannot create ") + path);
        // the writer's thread first puts out the graph lines, which precede the paths in the file (host_graph_lines), then the batches
        BatchWriter writer;
        writer.file = &file; writer.device = ix->device;
        writer.preamble = [&h, translated, &file]() { return host_graph_lines(h, translated, file); };
        writer.start();
        // the passes over the paths (lines_plan.hpp: gfa_passes), each in ascending path id
        static_assert(GBWT_HIP_PATHS_DEFAULT == 0 && GBWT_HIP_PATHS_PAN_SN == 1 && GBWT_HIP_PATHS_REF_ONLY == 2, "the path modes gfa_passes knows");
        uint64_t ref_sample = 0;
        const bool have_ref = (h.metadata_flags & 2) && h.sample_names.find(GENERIC_SAMPLE, ref_sample);
        if (!have_ref) ref_sample = h.sample_count;
        uint64_t longest_name = 0;
        if (translated) for (size_t i = 0; i < h.segment_names.size(); i++) longest_name = std::max<uint64_t>(longest_name, h.segment_names.len(i));
        const uint64_t token = token_width_bound(h.alphabet_size / 2, translated, longest_name);
        uint64_t budget = uint64_t(1) << 30;
        if (const char *v = std::getenv("GBWT_HIP_GFA_BATCH_MIB")) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10)) << 20;
        const uint64_t fallback_batch = 4096;                // without sequence lengths: by count, as until round 3
        int slot = 0;
        gbwt_hip_status st = GBWT_HIP_OK;
        for (const LinePass &pass : gfa_passes(path_mode, have_ref)) {
            std::vector<uint64_t> ids;
            for (uint64_t p = 0; p < h.path_names.size(); p++)
                if (pass.which == 2 || (h.path_names[p].sample == ref_sample) == (pass.which == 0)) ids.push_back(p);
            for (uint64_t b0 = 0; b0 < ids.size() && st == GBWT_HIP_OK;) {
                const uint64_t nb = next_batch(ids.data(), ids.size(), b0, ix->host_seq_len.data(), ix->host_seq_len.size(), token, budget, fallback_batch);
                if (!writer.acquire(slot)) { st = GBWT_HIP_IO_ERROR; break; }
                st = path_lines_compute(ix, ws, ids.data() + b0, nb, pass.line_mode, slot);
                if (st != GBWT_HIP_OK) break;
                writer.submit((slot == 0 ? ws->lines.text : ws->lines.text2).as<char>(), ws->lines.total, slot);
                slot ^= 1;
                b0 += nb;
            }
            if (st != GBWT_HIP_OK) break;
        }
        const gbwt_hip_status wst = writer.finish();
        ws->lines.memo.drop();                               // (both text buffers have been reused)
        if (st == GBWT_HIP_OK && wst != GBWT_HIP_OK) return fail(wst, writer.message);
        if (st != GBWT_HIP_OK) return wst != GBWT_HIP_OK ? fail(wst, writer.message) : st;
        if (file.failed) return fail(GBWT_HIP_IO_ERROR, "short write");
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

}  // extern "C"
