// capi_sequences.hip -- the C ABI of the bases family (include/gbwt_hip.h): the bases of a batch of paths on a workspace, the label of a
// node from the host image, and gbz-extract's `sequences` mode into files.  The kernels and the label upload are sequences.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "batch_writer.hpp"
#include "capi_internal.hpp"
#include "extract_files.hpp"
#include "gfa_host.hpp"
#include "scan.hpp"
#include "sequences.hpp"

using namespace gbwt_hip;

namespace {

constexpr uint32_t SEQ_CHUNK = GFA_LINE_CHUNK;     // path positions per chunk (the chunks of the line formatter: launch_chunk_plan)

// The bases of a batch of paths, computed ONCE into device memory (text buffer of `slot`: ws->bases.text or text2; row k at
// [offsets[k], offsets[k + 1]) of ws->bases.offsets).  The request is remembered in the workspace: the fill call after a size query, and the
// copy-out of gbwt_hip_path_sequences after gbwt_hip_path_sequences_device, find the bases there.
gbwt_hip_status sequences_compute(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int reverse, int endmarker, int slot = 0) {
    if (!ix || !ws || ws->index != ix) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    if (n && !path_ids) return fail(GBWT_HIP_BAD_ARGUMENT, "null path_ids");
    if (!endmarker_valid(endmarker)) return fail(GBWT_HIP_BAD_ARGUMENT, ENDMARKER_RULE);
    reverse = reverse ? 1 : 0;
    if (ws->bases.memo.matches({{path_ids, n * sizeof(uint64_t)}}, {reverse, endmarker, slot})) return GBWT_HIP_OK;
    ws->bases.memo.drop();
    ws->bases.timed = false;
    try {
        require_bases_capable(ix);
        const HostIndex &h = ix->host;
        HIP_CHECK(hipSetDevice(ix->device));
        hipStream_t s = ws->stream;
        ws->bases.offsets.reserve((n + 1) * sizeof(uint64_t));
        ws->bases.total = 0;
        if (n == 0) {
            HIP_CHECK(hipMemsetAsync(ws->bases.offsets.ptr, 0, sizeof(uint64_t), s));
            HIP_CHECK(hipStreamSynchronize(s));
            ws->bases.memo.store({{nullptr, 0}}, {reverse, endmarker, slot});
            return GBWT_HIP_OK;
        }
        ensure_labels(ix);
        if (!labels_fit_a_batch(ix)) return fail(GBWT_HIP_UNSUPPORTED, LABELS_TOO_LONG);
        // 1. the rows: GBZ::path(id, orientation) = sequence 2 id + orientation (support::encode_path); an id whose sequence does not exist
        // walks nothing and gets an empty row (as in gbwt_hip_extract_paths)
        std::vector<uint64_t> seq_ids(n);
        bool cacheable = !reverse && ix->lc_state == 1;
        for (uint64_t k = 0; k < n; k++) {
            seq_ids[k] = path_ids[k] < (~uint64_t(0)) / 2 ? 2 * path_ids[k] + static_cast<uint64_t>(reverse) : ~uint64_t(0);
            if (seq_ids[k] < h.sequences && path_ids[k] >= h.path_names.size()) cacheable = false;   // (the line cache has the paths of the metadata)
        }
        gbwt_hip_paths paths{};
        const gbwt_hip_status st = gbwt_hip_extract_device(ix, ws, seq_ids.data(), n, &paths);
        if (st != GBWT_HIP_OK) return st;
        ws->bases.ev.ensure();
        ws->extract.pinned_words.ensure();
        HIP_CHECK(hipEventRecord(ws->bases.ev[0], s));
        const uint64_t *d_seq_ids = ws->extract.seq_ids.as<uint64_t>();         // (the extraction has left the ids on the device)
        // 2. sizes.  Chunks of SEQ_CHUNK positions (at least one per row, at most len / SEQ_CHUNK + 1): launches and scans run over that bound.
        const uint64_t chunks_cap = paths.total / SEQ_CHUNK + n;
        if (chunks_cap > 0x7FFFFFFFull) return fail(GBWT_HIP_UNSUPPORTED, "too many chunks in one batch: ask for fewer paths per call");
        const uint64_t piece = ws->knobs.scan_piece;
        const size_t tb = scan_temp_bytes(std::max(n, chunks_cap) + 1, piece);
        ws->scratch.a.reserve(n * sizeof(uint64_t));
        ws->scratch.chunk_first.reserve(2 * (n + 1) * sizeof(uint64_t));
        ws->scratch.chunks.reserve((2 * chunks_cap + 1) * sizeof(uint64_t) + (chunks_cap + 1) * sizeof(uint32_t));
        ws->scratch.plan.reserve(chunks_cap * sizeof(SeqPlan));
        ws->scratch.scan_temp.reserve(tb);
        uint64_t *d_row_len = ws->scratch.a.as<uint64_t>(), *d_row_start = ws->bases.offsets.as<uint64_t>();
        uint64_t *d_chunk_first = ws->scratch.chunk_first.as<uint64_t>(), *d_chunk_counts = d_chunk_first + (n + 1);
        uint64_t *d_chunk_bases = ws->scratch.chunks.as<uint64_t>(), *d_bases_before = d_chunk_bases + chunks_cap;
        uint32_t *d_chunk_path = reinterpret_cast<uint32_t *>(d_bases_before + (chunks_cap + 1));
        const Labels labels = labels_of(ix);
        const ChunkedRows rows{paths.d_offsets, paths.d_nodes, n, d_chunk_first, d_chunk_path, chunks_cap};
        launch_chunk_plan(paths.d_offsets, n, chunks_cap, d_chunk_counts, d_chunk_first, d_chunk_path, ws->scratch.scan_temp.ptr, tb, s, piece);
        const auto chunk_pass = [&]() {
            launch_chunk_bases(rows, labels, d_chunk_bases, s);
            launch_scan(d_chunk_bases, d_bases_before, chunks_cap, ws->scratch.scan_temp.ptr, tb, s, piece);
        };
        // The host waits once, for the total that sizes the text buffer.  With the line cache the rows are sized without a node read and the
        // total leaves before the pass that places the chunks inside their rows: the host's wait and allocation run under that pass.
        if (!cacheable) chunk_pass();
        launch_row_bytes(d_seq_ids, n, h.sequences, cacheable ? ix->lc_path.as<uint64_t>() : nullptr, d_chunk_first, d_bases_before, endmarker, d_row_len, s);
        launch_scan(d_row_len, d_row_start, n, ws->scratch.scan_temp.ptr, tb, s, piece);
        HIP_CHECK(hipMemcpyAsync(ws->extract.pinned_words.p, d_row_start + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipEventRecord(ws->bases.ev[1], s));
        if (cacheable) chunk_pass();
        HIP_CHECK(hipEventSynchronize(ws->bases.ev[1]));                      // the one wait of a request
        HIP_CHECK(hipGetLastError());
        const uint64_t total = ws->extract.pinned_words.p[0];
        // 3. the bases
        DeviceBuffer &text = slot == 0 ? ws->bases.text : ws->bases.text2;
        text.reserve(std::max<uint64_t>(total, 16));
        launch_plan_bases(rows, d_seq_ids, h.sequences, d_bases_before, d_row_start, endmarker, ws->scratch.plan.as<SeqPlan>(), s);
        HIP_CHECK(hipEventRecord(ws->bases.ev[1], s));
        launch_bases(rows, ws->scratch.plan.as<SeqPlan>(), labels, endmarker, text.as<uint8_t>(), s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ws->bases.ev[2], s));
        HIP_CHECK(hipStreamSynchronize(s));
        ws->bases.timed = true;
        ws->bases.total = total;
        ws->bases.memo.store({{path_ids, n * sizeof(uint64_t)}}, {reverse, endmarker, slot});
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const HipError &e) {
        return status_of(e);
    }
}

// Metadata::sample_name / contig_name fall back to the number (src/gbwt.rs:744-761, 792-809)
std::string name_or_number(const Strings &table, bool has, uint64_t id) {
    if (has && id < table.size()) return std::string(reinterpret_cast<const char *>(table.bytes.data()) + table.offsets[id], table.len(id));
    return std::to_string(id);
}

}  // namespace

extern "C" {

// gbz-extract's extract_sequence (src/bin/gbz-extract.rs:173-191) for a batch of paths, left in HBM
gbwt_hip_status gbwt_hip_path_sequences_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int reverse, int endmarker,
                                               gbwt_hip_lines *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_lines{nullptr, nullptr, 0, 0};
    const gbwt_hip_status st = sequences_compute(ix, ws, path_ids, n, reverse, endmarker);
    if (st != GBWT_HIP_OK) return st;
    out->d_text = ws->bases.text.as<char>();
    out->d_line_offsets = ws->bases.offsets.as<uint64_t>();
    out->total = ws->bases.total;
    out->n = n;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

// The same copied to host buffers: out_offsets[n + 1] (may be NULL), out[total] (NULL = size query)
gbwt_hip_status gbwt_hip_path_sequences(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int reverse, int endmarker, char *out,
                                        uint64_t *out_offsets, uint64_t capacity, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (!total) return fail(GBWT_HIP_BAD_ARGUMENT, "null total");
    *total = 0;
    const gbwt_hip_status st = sequences_compute(ix, ws, path_ids, n, reverse, endmarker);
    if (st != GBWT_HIP_OK) return st;
    *total = ws->bases.total;
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        if (out_offsets) HIP_CHECK(hipMemcpy(out_offsets, ws->bases.offsets.ptr, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (!out || *total == 0) return GBWT_HIP_OK;
        if (capacity < *total) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the bases");
        copy_to_host(ws, out, ws->bases.text.ptr, *total);
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

// GBZ::sequence / sequence_len (src/gbz.rs:292-305) from the host image
gbwt_hip_status gbwt_hip_node_sequence(const gbwt_hip_index *ix, uint64_t node_id, char *out, uint64_t capacity, uint64_t *len, uint8_t *found) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !len || !found) return fail(GBWT_HIP_BAD_ARGUMENT, "null index / len / found");
    *len = 0; *found = 0;
    const HostIndex &h = ix->host;
    if (!h.is_gbz) return fail(GBWT_HIP_BAD_ARGUMENT, "node labels need a GBZ, this handle holds a bare GBWT");
    if (!node_exists(h, node_id)) return GBWT_HIP_OK;
    const uint64_t s = (2 * node_id - (h.alphabet_offset + 1)) / 2;      // GBZ::graph_node_to_sequence (src/gbz.rs:246-255; has_node: 2 node_id > alphabet_offset)
    if (s >= h.sequences_labels.size()) return GBWT_HIP_OK;
    *found = 1;
    *len = h.sequences_labels.len(s);
    if (!out || *len == 0) return GBWT_HIP_OK;
    if (capacity < *len) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the label");
    std::memcpy(out, h.sequences_labels.bytes.data() + h.sequences_labels.offsets[s], *len);
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_sequences_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *sizes_ms, float *bases_ms) {
    GBWT_HIP_GUARD_BEGIN
    if (!ws || !ws->bases.timed || !ws->extract.timed) return fail(GBWT_HIP_BAD_ARGUMENT, "no timed request for bases on this workspace");
    float a = 0, b = 0, c = 0;
    if (hipEventElapsedTime(&a, ws->extract.ev[0], ws->extract.ev[1]) != hipSuccess || hipEventElapsedTime(&b, ws->bases.ev[0], ws->bases.ev[1]) != hipSuccess ||
        hipEventElapsedTime(&c, ws->bases.ev[1], ws->bases.ev[2]) != hipSuccess)
        return fail(GBWT_HIP_DEVICE_ERROR, "hipEventElapsedTime failed");
    if (walk_ms) *walk_ms = a;
    if (sizes_ms) *sizes_ms = b;
    if (bases_ms) *bases_ms = c;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

// gbz-extract -o path (extract_sequences, src/bin/gbz-extract.rs:266-294): the forward bases of the paths, each with its endmarker, into
// `path`, and one line per path into `path`.names (extract_files.hpp).  Batches bounded by BYTES (GBWT_HIP_SEQ_BATCH_MIB, read at
// call time, default 1 GiB) are made into two device buffers in turn while a writer thread moves the previous one to the file (batch_writer.hpp).
gbwt_hip_status gbwt_hip_write_sequences(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const char *path, const uint64_t *path_ids, uint64_t n, int endmarker) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !ws || ws->index != ix || !path) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace / path");
    if (!endmarker_valid(endmarker)) return fail(GBWT_HIP_BAD_ARGUMENT, ENDMARKER_RULE);
    try {
        require_bases_capable(ix);
        const HostIndex &h = ix->host;
        if (!h.has_metadata) return fail(GBWT_HIP_BAD_ARGUMENT, "sequence extraction requires GBWT metadata");
        if (!(h.metadata_flags & 1) || h.path_names.empty()) return fail(GBWT_HIP_BAD_ARGUMENT, "sequence extraction requires path names");
        std::vector<uint64_t> ids;
        if (path_ids) ids.assign(path_ids, path_ids + n);
        else for (uint64_t p = 0; p < h.path_names.size(); p++) ids.push_back(p);
        for (uint64_t p : ids)
            if (p >= h.path_names.size() || !path_exists(h.sequences, p)) return fail(GBWT_HIP_BAD_ARGUMENT, "path id out of range");
        ensure_labels(ix);                                   // refused before a file is created or emptied
        if (!ids.empty() && !labels_fit_a_batch(ix)) return fail(GBWT_HIP_UNSUPPORTED, LABELS_TOO_LONG);
        uint64_t budget = uint64_t(1) << 30;
        if (const char *v = std::getenv("GBWT_HIP_SEQ_BATCH_MIB")) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10)) << 20;
        // bytes of every path: exact from the line cache of the index (summed label lengths of the forward path); else nodes x the mean label
        // length, twice over; else (no lengths known) batches of a fixed number of paths
        std::vector<uint64_t> est(ids.size(), 0);
        if (ix->lc_state == 1) {
            std::vector<uint64_t> totals(2 * h.path_names.size());
            HIP_CHECK(hipSetDevice(ix->device));
            HIP_CHECK(hipMemcpy(totals.data(), ix->lc_path.ptr, totals.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
            for (size_t k = 0; k < ids.size(); k++) est[k] = totals[2 * ids[k] + 1] + 1;
        } else if (!ix->host_seq_len.empty()) {
            const uint64_t labels = std::max<uint64_t>(h.sequences_labels.size(), 1);
            const uint64_t mean = (h.sequences_labels.bytes.size() + labels - 1) / labels;
            for (size_t k = 0; k < ids.size(); k++) est[k] = 2 * mean * ix->host_seq_len[2 * ids[k]] + 1;
        }
        const uint64_t fallback_batch = 4096;
        PositionalFile file, names;
        file.fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (file.fd < 0) return fail(GBWT_HIP_IO_ERROR, std::string("cannot create ") + path);
        const std::string names_path = std::string(path) + ".names";
        names.fd = ::open(names_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (names.fd < 0) return fail(GBWT_HIP_IO_ERROR, std::string("cannot create ") + names_path);
        const bool sample_names = (h.metadata_flags & 2) != 0, contig_names = (h.metadata_flags & 4) != 0;
        std::string lines;
        uint64_t names_at = 0;
        BatchWriter writer;
        writer.file = &file; writer.device = ix->device; writer.what = "sequences";
        writer.start();
        int slot = 0;
        gbwt_hip_status st = GBWT_HIP_OK;
        std::vector<uint64_t> offs;
        for (uint64_t b0 = 0; b0 < ids.size();) {
            uint64_t nb = 0, bytes = 0;
            while (b0 + nb < ids.size()) {
                if (nb != 0 && (est[b0 + nb] == 0 ? nb >= fallback_batch : bytes + est[b0 + nb] > budget)) break;
                bytes += est[b0 + nb]; nb++;
            }
            if (!writer.acquire(slot)) { st = GBWT_HIP_IO_ERROR; break; }
            st = sequences_compute(ix, ws, ids.data() + b0, nb, 0, endmarker, slot);
            if (st != GBWT_HIP_OK) break;
            writer.submit((slot == 0 ? ws->bases.text : ws->bases.text2).as<char>(), ws->bases.total, slot);
            offs.resize(nb + 1);
            HIP_CHECK(hipMemcpy(offs.data(), ws->bases.offsets.ptr, (nb + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
            lines.clear();
            for (uint64_t k = 0; k < nb; k++) {
                const uint64_t p = ids[b0 + k];
                const PathName &pn = h.path_names[p];
                append_names_line(lines, p, name_or_number(h.sample_names, sample_names, pn.sample), name_or_number(h.contig_names, contig_names, pn.contig), pn.phase, pn.fragment,
                                  offs[k + 1] - offs[k] - (endmarker >= 0 ? 1 : 0));
            }
            if (!names.write_at(lines.data(), lines.size(), names_at)) { st = fail(GBWT_HIP_IO_ERROR, "short write"); break; }
            names_at += lines.size();
            slot ^= 1;
            b0 += nb;
        }
        const gbwt_hip_status wst = writer.finish();
        ws->bases.memo.drop();                               // (both text buffers have been reused)
        if (st == GBWT_HIP_OK && wst != GBWT_HIP_OK) return fail(wst, writer.message);
        if (st != GBWT_HIP_OK) return wst != GBWT_HIP_OK ? fail(wst, writer.message) : st;
        if (file.failed || names.failed) return fail(GBWT_HIP_IO_ERROR, "short write");
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

}  // extern "C"
