// capi_suffix_array.hip -- the C ABI of the suffix array family (include/gbwt_hip.h, "suffix array and BWT of a text"): a text in host or
// device memory without an index, the text of paths on a workspace, and the files between gbz-extract's two modes.  The builder is
// suffix_array.hip; the text of paths is the bases family's (capi_sequences.hip); what the files hold is extract_files.hpp.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <mutex>
#include <string>
#include <vector>

#include "batch_writer.hpp"
#include "capi_internal.hpp"
#include "extract_files.hpp"
#include "sa_plan.hpp"
#include "suffix_array.hpp"

using namespace gbwt_hip;

namespace {

constexpr uint64_t SA_LEAD = 16;      // bytes in front of the results on a workspace (workspace.hpp: SuffixState)

// The last gbwt_hip_suffix_array_text* call of the process (gbwt_hip_last_suffix_array_info without a workspace)
std::mutex text_info_mutex;
gbwt_hip_suffix_array_info text_info{};
bool text_info_valid = false;

void keep_text_info(const gbwt_hip_suffix_array_info &info) {
    std::lock_guard<std::mutex> lock(text_info_mutex);
    text_info = info;
    text_info_valid = true;
}

gbwt_hip_status check_text_call(const void *text, uint64_t n, int sentinel, const uint64_t *out_sa) {
    if (sentinel < 0 || sentinel > 255) return fail(GBWT_HIP_BAD_ARGUMENT, "sentinel must be a byte value 0..255");
    if (n && (!text || !out_sa)) return fail(GBWT_HIP_BAD_ARGUMENT, "null text / suffix array");
    if (n > SA_MAX_TEXT) return fail(GBWT_HIP_UNSUPPORTED, sa_plan(n, 0, 0).message);
    return GBWT_HIP_OK;
}

// The suffix array of the text of these paths on the workspace, made unless the workspace holds it
gbwt_hip_status suffix_compute(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int endmarker) {
    if (!ix || !ws || ws->index != ix) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    if (n && !path_ids) return fail(GBWT_HIP_BAD_ARGUMENT, "null path_ids");
    if (!endmarker_valid(endmarker)) return fail(GBWT_HIP_BAD_ARGUMENT, ENDMARKER_RULE);
    SuffixState &f = ws->suffix;
    if (f.memo.matches({{path_ids, n * sizeof(uint64_t)}}, {endmarker})) return GBWT_HIP_OK;
    f.memo.drop();
    f.built = false;
    gbwt_hip_lines text{};
    const gbwt_hip_status st = gbwt_hip_path_sequences_device(ix, ws, path_ids, n, 0, endmarker, &text);
    if (st != GBWT_HIP_OK) return st;
    const uint64_t total = text.total;
    if (total > SA_MAX_TEXT) return fail(GBWT_HIP_UNSUPPORTED, sa_plan(total, 0, 0).message);
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        hipStream_t s = ws->stream;
        f.ctx.ensure();
        f.sa.reserve(SA_LEAD + total * sizeof(uint64_t));
        f.bwt.reserve(SA_LEAD + total);
        const uint64_t lead[2] = {0, total};                 // what a .sa and a .bwt file start with
        HIP_CHECK(hipMemcpyAsync(f.sa.ptr, lead, sizeof(lead), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(f.bwt.ptr, 0, SA_LEAD, s));
        if (total) HIP_CHECK(hipMemcpyAsync(f.bwt.as<uint8_t>() + SA_LEAD - 1, text.d_text + total - 1, 1, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));                  // (`lead` leaves the stack)
        const uint8_t sentinel = endmarker >= 0 ? static_cast<uint8_t>(endmarker) : 0;
        const gbwt_hip_status built = build_suffix_array(reinterpret_cast<const uint8_t *>(text.d_text), total, sentinel, reinterpret_cast<uint64_t *>(f.sa.as<uint8_t>() + SA_LEAD),
                                                         f.bwt.as<uint8_t>() + SA_LEAD, f.ctx, s, f.info);
        if (built != GBWT_HIP_OK) return built;
        float walk = 0, sizes = 0, bases = 0;
        if (total && gbwt_hip_last_sequences_ms(ws, &walk, &sizes, &bases) == GBWT_HIP_OK) f.info.text_ms = walk + sizes + bases;
        f.total = total;
        f.built = true;
        f.memo.store({{path_ids, n * sizeof(uint64_t)}}, {endmarker});
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e, "the suffix array");
    }
}

// One stretch of device memory into a new file through the whole-file writer
gbwt_hip_status write_stretch(const std::string &path, const char *d_bytes, uint64_t bytes, int device, const char *what) {
    PositionalFile file;
    file.fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (file.fd < 0) return fail(GBWT_HIP_IO_ERROR, "cannot create " + path);
    BatchWriter writer;
    writer.file = &file; writer.device = device; writer.what = what;
    writer.start();
    if (writer.acquire(0)) writer.submit(d_bytes, bytes, 0);
    const gbwt_hip_status st = writer.finish();
    if (st != GBWT_HIP_OK) return fail(st, writer.message);
    if (file.failed) return fail(GBWT_HIP_IO_ERROR, "short write to " + path);
    return GBWT_HIP_OK;
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_suffix_array_text_device(int device, const void *d_text, uint64_t n, int sentinel, uint64_t *d_sa, uint8_t *d_bwt, void *stream, uint64_t *bwt_runs) {
    GBWT_HIP_GUARD_BEGIN
    if (bwt_runs) *bwt_runs = 0;
    gbwt_hip_status st = check_text_call(d_text, n, sentinel, d_sa);
    if (st != GBWT_HIP_OK) return st;
    if (n == 0) { keep_text_info(gbwt_hip_suffix_array_info{}); return GBWT_HIP_OK; }
    st = require_device();
    if (st != GBWT_HIP_OK) return st;
    try {
        HIP_CHECK(hipSetDevice(device));
        SaContext ctx;
        ctx.ensure();
        gbwt_hip_suffix_array_info info{};
        st = build_suffix_array(static_cast<const uint8_t *>(d_text), n, static_cast<uint8_t>(sentinel), d_sa, d_bwt, ctx, static_cast<hipStream_t>(stream), info);
        if (st != GBWT_HIP_OK) return st;
        keep_text_info(info);
        if (bwt_runs) *bwt_runs = info.bwt_runs;
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e, "the suffix array");
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_suffix_array_text(int device, const void *text, uint64_t n, int sentinel, uint64_t *out_sa, uint8_t *out_bwt, uint64_t *bwt_runs) {
    GBWT_HIP_GUARD_BEGIN
    if (bwt_runs) *bwt_runs = 0;
    gbwt_hip_status st = check_text_call(text, n, sentinel, out_sa);
    if (st != GBWT_HIP_OK) return st;
    if (n == 0) { keep_text_info(gbwt_hip_suffix_array_info{}); return GBWT_HIP_OK; }
    st = require_device();
    if (st != GBWT_HIP_OK) return st;
    try {
        HIP_CHECK(hipSetDevice(device));
        Stream stream;
        SaContext ctx;
        ctx.ensure();
        DeviceBuffer d_text, d_sa, d_bwt;
        d_text.reserve(n);
        d_sa.reserve(n * sizeof(uint64_t));
        if (out_bwt) d_bwt.reserve(n);
        HIP_CHECK(hipEventRecord(ctx.ev[0], stream));
        HIP_CHECK(hipMemcpyAsync(d_text.ptr, text, n, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipEventRecord(ctx.ev[7], stream));
        gbwt_hip_suffix_array_info info{};
        st = build_suffix_array(d_text.as<uint8_t>(), n, static_cast<uint8_t>(sentinel), d_sa.as<uint64_t>(), out_bwt ? d_bwt.as<uint8_t>() : nullptr, ctx, stream, info);
        if (st != GBWT_HIP_OK) return st;
        HIP_CHECK(hipEventElapsedTime(&info.text_ms, ctx.ev[0], ctx.ev[7]));
        HIP_CHECK(hipMemcpy(out_sa, d_sa.ptr, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (out_bwt) HIP_CHECK(hipMemcpy(out_bwt, d_bwt.ptr, n, hipMemcpyDeviceToHost));
        keep_text_info(info);
        if (bwt_runs) *bwt_runs = info.bwt_runs;
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e, "the suffix array");
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_path_suffix_array_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int endmarker, gbwt_hip_suffix_array *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    *out = gbwt_hip_suffix_array{nullptr, nullptr, 0, 0};
    const gbwt_hip_status st = suffix_compute(ix, ws, path_ids, n, endmarker);
    if (st != GBWT_HIP_OK) return st;
    out->d_sa = reinterpret_cast<uint64_t *>(ws->suffix.sa.as<uint8_t>() + SA_LEAD);
    out->d_bwt = ws->suffix.bwt.as<uint8_t>() + SA_LEAD;
    out->total = ws->suffix.total;
    out->bwt_runs = ws->suffix.info.bwt_runs;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_path_suffix_array(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n, int endmarker, uint64_t *out_sa, uint8_t *out_bwt,
                                           uint64_t capacity, uint64_t *total, uint64_t *bwt_runs) {
    GBWT_HIP_GUARD_BEGIN
    if (!total) return fail(GBWT_HIP_BAD_ARGUMENT, "null total");
    *total = 0;
    if (bwt_runs) *bwt_runs = 0;
    const gbwt_hip_status st = suffix_compute(ix, ws, path_ids, n, endmarker);
    if (st != GBWT_HIP_OK) return st;
    *total = ws->suffix.total;
    if (bwt_runs) *bwt_runs = ws->suffix.info.bwt_runs;
    if ((!out_sa && !out_bwt) || *total == 0) return GBWT_HIP_OK;
    if (capacity < *total) return fail(GBWT_HIP_CAPACITY, "output capacity too small for the suffix array");
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        if (out_sa) copy_to_host(ws, out_sa, ws->suffix.sa.as<uint8_t>() + SA_LEAD, *total * sizeof(uint64_t));
        if (out_bwt) copy_to_host(ws, out_bwt, ws->suffix.bwt.as<uint8_t>() + SA_LEAD, *total);
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_write_suffix_array(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const char *base_path, uint64_t *bwt_runs) {
    GBWT_HIP_GUARD_BEGIN
    if (bwt_runs) *bwt_runs = 0;
    if (!ix || !ws || ws->index != ix || !base_path) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace / path");
    const std::string base(base_path), sa_path = base + ".sa", bwt_path = base + ".bwt";
    try {
        require_bases_capable(ix);
        (void)::unlink(sa_path.c_str());                     // what an earlier call left would stand beside names it no longer matches if this one fails
        (void)::unlink(bwt_path.c_str());
        // 1. the names: path id, bases; the text file, where there is one: its size, and the endmarker at its end
        std::vector<uint64_t> ids, lens;
        FileCheck names = read_names(base + ".names", ids, lens);
        if (names.ok()) names = check_paths_exist(ix->host.sequences, ids, lens);
        if (!names.ok()) return fail(names.status, names.message);
        uint64_t expected_len = 0;
        for (uint64_t len : lens) expected_len += len + 1;
        int endmarker = 0;
        {
            PositionalFile text_file;
            text_file.fd = ::open(base.c_str(), O_RDONLY);
            if (text_file.fd >= 0) {
                struct stat info {};
                if (::fstat(text_file.fd, &info) != 0) return fail(GBWT_HIP_IO_ERROR, "cannot stat " + base);
                if (static_cast<uint64_t>(info.st_size) != expected_len)
                    return fail(GBWT_HIP_INVALID_DATA, base + " has " + std::to_string(info.st_size) + " bytes, the paths of " + base + ".names have " + std::to_string(expected_len));
                uint8_t last = 0;
                if (::pread(text_file.fd, &last, 1, static_cast<off_t>(expected_len - 1)) != 1) return fail(GBWT_HIP_IO_ERROR, "cannot read " + base);
                endmarker = last;
            }
        }
        // 2. the text, and the walked bases of every path against its line
        gbwt_hip_lines text{};
        gbwt_hip_status st = gbwt_hip_path_sequences_device(ix, ws, ids.data(), ids.size(), 0, endmarker, &text);
        if (st != GBWT_HIP_OK) return st;
        std::vector<uint64_t> rows(ids.size() + 1);
        HIP_CHECK(hipSetDevice(ix->device));
        HIP_CHECK(hipMemcpy(rows.data(), text.d_line_offsets, rows.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
        const FileCheck walked = check_walked_lengths(ids, lens, rows.data());
        if (!walked.ok()) return fail(walked.status, walked.message);
        // 3. the suffix array (the text of step 2 is still the bases family's), and the two files
        st = suffix_compute(ix, ws, ids.data(), ids.size(), endmarker);
        if (st != GBWT_HIP_OK) return st;
        const uint64_t total = ws->suffix.total;
        st = write_stretch(sa_path, ws->suffix.sa.as<char>() + SA_LEAD - sizeof(uint64_t), (total + 1) * sizeof(uint64_t), ix->device, "suffix array");
        if (st == GBWT_HIP_OK) st = write_stretch(bwt_path, ws->suffix.bwt.as<char>() + SA_LEAD - 1, total + 1, ix->device, "bwt");
        if (st != GBWT_HIP_OK) {
            const std::string message = last_error_slot();
            (void)::unlink(sa_path.c_str());                 // nothing half written stays behind
            (void)::unlink(bwt_path.c_str());
            return fail(st, message);
        }
        if (bwt_runs) *bwt_runs = ws->suffix.info.bwt_runs;
        return GBWT_HIP_OK;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_BAD_ARGUMENT, e.what());
    } catch (const HipError &e) {
        return status_of(e, "the suffix array");
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_suffix_array_info(const gbwt_hip_workspace *ws, gbwt_hip_suffix_array_info *out) {
    GBWT_HIP_GUARD_BEGIN
    if (!out) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    if (ws) {
        if (!ws->suffix.built) return fail(GBWT_HIP_BAD_ARGUMENT, "no suffix array has been built on this workspace");
        *out = ws->suffix.info;
        return GBWT_HIP_OK;
    }
    std::lock_guard<std::mutex> lock(text_info_mutex);
    if (!text_info_valid) return fail(GBWT_HIP_BAD_ARGUMENT, "no suffix array of a text has been built in this process");
    *out = text_info;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

}  // extern "C"
