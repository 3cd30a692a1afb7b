// capi_tags.hip -- the C ABI of the tags family (include/gbwt_hip.h): the plan of a list of path ids on a workspace, the gather of a suffix
// array in device or host memory, and gbz-extract's `tag-array` mode over files (extract_tag_array, src/bin/gbz-extract.rs:408-482).  The
// kernels, and what a tag is, are tags.hip.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "batch_writer.hpp"
#include "capi_internal.hpp"
#include "extract_files.hpp"
#include "scan.hpp"
#include "tags.hpp"

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
        throw OutOfMemory{std::string(what) + " needs " + std::to_string(total) + " bytes of device memory, " + std::to_string(more - back) + " more than the workspace holds for it; " +
                          std::to_string(free_bytes) + " are free"};
}

void drop_plan(gbwt_hip_workspace *ws) { ws->tags.plan_key.drop(); ws->tags.timed = false; ws->tags.rows.clear(); ws->tags.positions = 0; ws->tags.text_len = 0; }

// The plan of a list of path ids (see the top of tags.hip), made unless the workspace holds it.  No gather has run on it yet: gather_ms = 0.
gbwt_hip_status tags_plan(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n) {
    if (!ix || !ws || ws->index != ix) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    if (n && !path_ids) return fail(GBWT_HIP_BAD_ARGUMENT, "null path_ids");
    if (ws->tags.plan_key.matches({{path_ids, n * sizeof(uint64_t)}}, {})) {
        ws->tags.gather_ms = 0;
        return GBWT_HIP_OK;
    }
    drop_plan(ws);
    try {
        require_bases_capable(ix);
        const HostIndex &h = ix->host;
        std::vector<uint64_t> seq_ids(n);
        for (uint64_t k = 0; k < n; k++) {
            if (!path_exists(h.sequences, path_ids[k])) return fail(GBWT_HIP_BAD_ARGUMENT, "path id out of range: " + std::to_string(path_ids[k]));
            seq_ids[k] = 2 * path_ids[k];            // GBZ::path(id, Forward) = sequence 2 id (support::encode_path)
        }
        HIP_CHECK(hipSetDevice(ix->device));
        hipStream_t s = ws->stream;
        ws->tags.ev.ensure();
        ws->tags.state.reserve(sizeof(TagState));
        ws->tags.walk_ms = ws->tags.plan_ms = ws->tags.gather_ms = 0;
        if (n == 0) {                                // an empty text: nothing to look anything up in
            ws->tags.rows.assign(1, 0);
            ws->tags.plan_key.store({{nullptr, 0}}, {});
            ws->tags.timed = true;
            return GBWT_HIP_OK;
        }
        ensure_labels(ix);
        gbwt_hip_paths paths{};
        const gbwt_hip_status st = gbwt_hip_extract_device(ix, ws, seq_ids.data(), n, &paths);
        if (st != GBWT_HIP_OK) return st;
        HIP_CHECK(hipEventElapsedTime(&ws->tags.walk_ms, ws->extract.ev[0], ws->extract.ev[1]));
        const uint64_t positions = paths.total + n;
        // GBWT_HIP_TAG_WIDE (64-bit hints whatever the size) lets tests reach what only plans of 2^32 positions reach otherwise; read when a plan is made
        const char *force_wide = std::getenv("GBWT_HIP_TAG_WIDE");
        const bool wide = positions > 0xFFFFFFFFull || (force_wide && std::atoi(force_wide) != 0);
        DeviceBuffer lengths;                        // the label lengths in front of the scan: scratch of the plan
        require_fits({{&ws->tags.node, positions * sizeof(uint32_t)}, {&ws->tags.off, (positions + 1) * sizeof(uint64_t)}, {&lengths, positions * sizeof(uint64_t)}}, "the tag plan");
        ws->tags.node.reserve(positions * sizeof(uint32_t));
        ws->tags.off.reserve((positions + 1) * sizeof(uint64_t));
        lengths.reserve(positions * sizeof(uint64_t));
        const size_t tb = scan_temp_bytes(positions, ws->knobs.scan_piece);
        ws->scratch.scan_temp.reserve(tb);
        ws->scratch.a.reserve((n + 1) * sizeof(uint64_t));
        uint64_t *d_len = lengths.as<uint64_t>(), *d_off = ws->tags.off.as<uint64_t>(), *d_rows = ws->scratch.a.as<uint64_t>();
        HIP_CHECK(hipEventRecord(ws->tags.ev[0], s));
        launch_tag_positions(paths.d_offsets, paths.d_nodes, n, positions, labels_of(ix), ws->tags.node.as<uint32_t>(), d_len, s);
        launch_scan(d_len, d_off, positions, ws->scratch.scan_temp.ptr, tb, s, ws->knobs.scan_piece);
        launch_tag_rows(paths.d_offsets, n, d_off, positions, d_rows, s);
        ws->tags.rows.resize(n + 1);
        HIP_CHECK(hipMemcpyAsync(ws->tags.rows.data(), d_rows, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));          // the one wait of a plan: the text length sizes the top level
        HIP_CHECK(hipGetLastError());
        lengths.release();
        const uint64_t text_len = ws->tags.rows[n], hints = ((text_len - 1) >> TAG_SHIFT) + 2;
        const uint64_t top_bytes = hints * (wide ? sizeof(uint64_t) : sizeof(uint32_t));
        require_fits({{&ws->tags.top, top_bytes}}, "the top level of the tag plan");
        ws->tags.top.reserve(top_bytes);
        launch_tag_top(d_off, positions, hints, ws->tags.top.ptr, wide, s);
        HIP_CHECK(hipEventRecord(ws->tags.ev[1], s));
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventElapsedTime(&ws->tags.plan_ms, ws->tags.ev[0], ws->tags.ev[1]));
        ws->tags.positions = positions;
        ws->tags.text_len = text_len;
        ws->tags.wide = wide;
        ws->tags.plan_key.store({{path_ids, n * sizeof(uint64_t)}}, {});
        ws->tags.timed = true;
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const OutOfMemory &e) {
        return fail(GBWT_HIP_CAPACITY, e.what);
    } catch (const HipError &e) {
        return status_of(e, "the tag plan");
    }
}

// One batch of the gather on the workspace's stream, waited for: tags[i] = tag(sa[i]) for i < count, runs and last tag into `state` (the
// device's copy is cleared by whoever starts a request), the kernel's time added to gather_ms; INVALID_DATA for a value out of range.
// has_prev, parity: see launch_tags.
gbwt_hip_status gather_batch(gbwt_hip_workspace *ws, const uint64_t *d_sa, uint64_t count, uint64_t *d_tags, bool has_prev, uint32_t parity, TagState &state) {
    hipStream_t s = ws->stream;
    TagsState &t = ws->tags;
    HIP_CHECK(hipEventRecord(t.ev[0], s));
    launch_tags(ws->index->device, TagTables{t.top.ptr, t.wide, t.off.as<uint64_t>(), t.node.as<uint32_t>(), t.text_len}, d_sa, count, d_tags, t.state.as<TagState>(), has_prev, parity, s);
    HIP_CHECK(hipEventRecord(t.ev[1], s));
    HIP_CHECK(hipMemcpyAsync(&state, t.state.ptr, sizeof(TagState), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, t.ev[0], t.ev[1]));
    t.gather_ms += ms;
    if (state.bad) return fail(GBWT_HIP_INVALID_DATA, "suffix array value out of range: the text has " + std::to_string(t.text_len) + " positions");
    return GBWT_HIP_OK;
}

// A whole request for `count` values in HBM: one batch behind a cleared state
gbwt_hip_status gather_once(gbwt_hip_workspace *ws, const uint64_t *d_sa, uint64_t count, uint64_t *d_tags, uint64_t *runs) {
    if (runs) *runs = 0;
    if (count == 0) return GBWT_HIP_OK;
    if (ws->tags.text_len == 0) return fail(GBWT_HIP_INVALID_DATA, "suffix array value out of range: the text of no paths is empty");
    TagState state{};
    HIP_CHECK(hipMemsetAsync(ws->tags.state.ptr, 0, sizeof(TagState), ws->stream));
    const gbwt_hip_status st = gather_batch(ws, d_sa, count, d_tags, false, 0, state);
    if (st == GBWT_HIP_OK && runs) *runs = state.runs;
    return st;
}

// The .tags file of a call from the moment it exists: however the call leaves, the writer has finished, and a file that is not whole is gone
struct TagsFile {
    const std::string &path;
    PositionalFile out;
    BatchWriter writer;
    bool whole = false;
    TagsFile(const std::string &tags_path, int fd, int device) : path(tags_path) {
        out.fd = fd;
        writer.file = &out; writer.device = device; writer.what = "tags";
        writer.start();
    }
    ~TagsFile() {
        (void)writer.finish();
        if (!whole) (void)::unlink(path.c_str());
    }
};

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_tags_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, const uint64_t *d_sa, uint64_t count,
                                     uint64_t *d_tags, uint64_t *runs) {
    GBWT_HIP_GUARD_BEGIN
    if (runs) *runs = 0;
    const gbwt_hip_status st = tags_plan(ix, ws, path_ids, n);
    if (st != GBWT_HIP_OK) return st;
    if (count && (!d_sa || !d_tags)) return fail(GBWT_HIP_BAD_ARGUMENT, "null suffix array / tags");
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        return gather_once(ws, d_sa, count, d_tags, runs);
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_tags(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, const uint64_t *sa, uint64_t count, uint64_t *tags,
                              uint64_t *expected_len, uint64_t *runs) {
    GBWT_HIP_GUARD_BEGIN
    if (expected_len) *expected_len = 0;
    if (runs) *runs = 0;
    const gbwt_hip_status st = tags_plan(ix, ws, path_ids, n);
    if (st != GBWT_HIP_OK) return st;
    if (expected_len) *expected_len = ws->tags.text_len;
    if (!sa && !tags) return GBWT_HIP_OK;            // the size query
    if (count && (!sa || !tags)) return fail(GBWT_HIP_BAD_ARGUMENT, "null suffix array / tags");
    if (count == 0) return GBWT_HIP_OK;
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        if (count > (~uint64_t(0)) / 16) return fail(GBWT_HIP_CAPACITY, "suffix array too large for device memory");
        require_fits({{&ws->tags.sa, count * sizeof(uint64_t)}, {&ws->tags.out, count * sizeof(uint64_t)}}, "the suffix array and its tags");
        ws->tags.sa.reserve(count * sizeof(uint64_t));
        ws->tags.out.reserve(count * sizeof(uint64_t));
        HIP_CHECK(hipMemcpyAsync(ws->tags.sa.ptr, sa, count * sizeof(uint64_t), hipMemcpyHostToDevice, ws->stream));
        const gbwt_hip_status gst = gather_once(ws, ws->tags.sa.as<uint64_t>(), count, ws->tags.out.as<uint64_t>(), runs);
        if (gst != GBWT_HIP_OK) return gst;          // (the caller's tags are untouched)
        copy_to_host(ws, tags, ws->tags.out.ptr, count * sizeof(uint64_t));
        return GBWT_HIP_OK;
    } catch (const OutOfMemory &e) {
        return fail(GBWT_HIP_CAPACITY, e.what);
    } catch (const HipError &e) {
        return status_of(e, "the suffix array");
    }
    GBWT_HIP_GUARD_END
}

// gbz-extract -m tag-array -o base (extract_tag_array, src/bin/gbz-extract.rs:408-482)
gbwt_hip_status gbwt_hip_write_tag_array(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const char *base_path, uint64_t sa_skip, uint64_t *runs) {
    GBWT_HIP_GUARD_BEGIN
    if (runs) *runs = 0;
    if (!ix || !ws || ws->index != ix || !base_path) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace / path");
    const std::string base(base_path), sa_path = base + ".sa", tags_path = base + ".tags";
    try {
        require_bases_capable(ix);
        // 1. the names: path id, bases
        std::vector<uint64_t> ids, lens;
        FileCheck names = read_names(base + ".names", ids, lens);
        if (names.ok()) names = check_paths_exist(ix->host.sequences, ids, lens);
        if (!names.ok()) return fail(names.status, names.message);
        // 2. the plan, and the walked bases of every path against its line
        const gbwt_hip_status st = tags_plan(ix, ws, ids.data(), ids.size());
        if (st != GBWT_HIP_OK) return st;
        const FileCheck walked = check_walked_lengths(ids, lens, ws->tags.rows.data());
        if (!walked.ok()) return fail(walked.status, walked.message);
        const uint64_t expected_len = ws->tags.text_len;
        // 3. the suffix array: sa_skip values skipped, expected_len read
        PositionalFile sa_file;
        sa_file.fd = ::open(sa_path.c_str(), O_RDONLY);
        if (sa_file.fd < 0) return fail(GBWT_HIP_IO_ERROR, "cannot open " + sa_path);
        struct stat info {};
        if (::fstat(sa_file.fd, &info) != 0) return fail(GBWT_HIP_IO_ERROR, "cannot stat " + sa_path);
        if (sa_skip > (~uint64_t(0)) / 16 || static_cast<uint64_t>(info.st_size) / sizeof(uint64_t) < sa_skip + expected_len)
            return fail(GBWT_HIP_IO_ERROR, sa_path + " is too short: " + std::to_string(sa_skip + expected_len) + " values expected, " + std::to_string(info.st_size) + " bytes found");
        uint64_t budget = uint64_t(256) << 20;
        if (const char *v = std::getenv("GBWT_HIP_TAG_BATCH_MIB")) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10)) << 20;
        const uint64_t batch = std::min<uint64_t>(std::max<uint64_t>(budget / sizeof(uint64_t), 1), expected_len);
        HIP_CHECK(hipSetDevice(ix->device));
        require_fits({{&ws->tags.sa, batch * sizeof(uint64_t)}, {&ws->tags.sa2, batch * sizeof(uint64_t)}, {&ws->tags.out, batch * sizeof(uint64_t)}, {&ws->tags.out2, batch * sizeof(uint64_t)}},
                     "the batches of the tag array");
        for (DeviceBuffer *b : {&ws->tags.sa, &ws->tags.sa2, &ws->tags.out, &ws->tags.out2}) b->reserve(batch * sizeof(uint64_t));
        std::vector<uint64_t> values(batch);
        HIP_CHECK(hipMemsetAsync(ws->tags.state.ptr, 0, sizeof(TagState), ws->stream));
        const int fd = ::open(tags_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd < 0) return fail(GBWT_HIP_IO_ERROR, "cannot create " + tags_path);
        // 4. the batches: read, gathered, handed to the writer; any return or throw from here on goes through ~TagsFile
        TagsFile file(tags_path, fd, ix->device);
        TagState state{};
        int slot = 0;
        uint32_t batches = 0;
        for (uint64_t done = 0; done < expected_len; done += batch, batches++, slot ^= 1) {
            const uint64_t cnt = std::min(batch, expected_len - done);
            uint64_t got = 0;
            while (got < cnt * sizeof(uint64_t)) {
                const ssize_t r = ::pread(sa_file.fd, reinterpret_cast<char *>(values.data()) + got, cnt * sizeof(uint64_t) - got, static_cast<off_t>((sa_skip + done) * sizeof(uint64_t) + got));
                if (r <= 0) break;
                got += static_cast<uint64_t>(r);
            }
            if (got < cnt * sizeof(uint64_t)) return fail(GBWT_HIP_IO_ERROR, "short read from " + sa_path);
            if (!file.writer.acquire(slot)) break;                                 // (the writer has failed: its status and message, below)
            uint64_t *d_sa = (slot == 0 ? ws->tags.sa : ws->tags.sa2).as<uint64_t>(), *d_tags = (slot == 0 ? ws->tags.out : ws->tags.out2).as<uint64_t>();
            HIP_CHECK(hipMemcpyAsync(d_sa, values.data(), cnt * sizeof(uint64_t), hipMemcpyHostToDevice, ws->stream));
            const gbwt_hip_status gst = gather_batch(ws, d_sa, cnt, d_tags, batches != 0, batches & 1u, state);
            if (gst != GBWT_HIP_OK) return gst;
            file.writer.submit(reinterpret_cast<const char *>(d_tags), cnt * sizeof(uint64_t), slot);
        }
        const gbwt_hip_status wst = file.writer.finish();
        if (wst != GBWT_HIP_OK) return fail(wst, file.writer.message);
        if (file.out.failed) return fail(GBWT_HIP_IO_ERROR, "short write to " + tags_path);
        file.whole = true;
        if (runs) *runs = state.runs;
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const OutOfMemory &e) {
        return fail(GBWT_HIP_CAPACITY, e.what);
    } catch (const HipError &e) {
        return status_of(e, "the batches of the tag array");
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_tags_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *plan_ms, float *gather_ms) {
    GBWT_HIP_GUARD_BEGIN
    if (!ws || !ws->tags.timed) return fail(GBWT_HIP_BAD_ARGUMENT, "no timed request for tags on this workspace");
    if (walk_ms) *walk_ms = ws->tags.walk_ms;
    if (plan_ms) *plan_ms = ws->tags.plan_ms;
    if (gather_ms) *gather_ms = ws->tags.gather_ms;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

}  // extern "C"
