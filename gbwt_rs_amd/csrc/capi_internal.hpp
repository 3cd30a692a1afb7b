// capi_internal.hpp -- handle / workspace structures, statuses and the checks of a call that makes a handle, shared by the C-ABI translation units (capi_open.hip, capi_extract.hip, capi_query.hip, capi_graph.hip, capi_topology.hip, capi_refpos.hip, capi_locate.hip, capi_build.hip, capi_gfa_build.hip, capi_merge.hip, capi_remove.hip, gfa.hip, sequences.hip, tags.hip, comm.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/gbwt_hip.h"
#include "device_index.hpp"
#include "host_index.hpp"
#include "kernels.hpp"
#include "lazy_build.hpp"

namespace gbwt_hip {

std::string &last_error_slot();   // thread-local message of the last failing call

inline gbwt_hip_status fail(gbwt_hip_status st, const std::string &msg) {
    last_error_slot() = msg;
    return st;
}

struct HipError { hipError_t err; const char *what; };

#define HIP_CHECK(expr)                                            \
    do {                                                           \
        hipError_t e_ = (expr);                                    \
        if (e_ != hipSuccess) throw gbwt_hip::HipError{e_, #expr}; \
    } while (0)

// Grow-only device buffer.
// Where a pass's 13 GB of rows land physically is worth up to 10 % of its time: on a fresh box one hipMalloc of that size takes one
// contiguous stretch of VRAM, and a pass over it takes 4.95 ms where the same buffer put together from chunks that lie SPREAD over the
// VRAM takes 4.45 (profiles/r02_walk_bounds.txt #25; the fast and slow "states" of a box in round 1 were this).  So the rows buffer of
// a workspace (may_spread), from 4 GiB, is built with the virtual-memory API: `spread` times as many physical chunks as needed are created, every spread-th is
// kept and mapped into one virtual range, the others are given back.  Chunks of 2 GiB: with 256 MB chunks the rows of ragged batches
// (walks out of lock step) were written 5 % slower than into one hipMalloc -- smaller mappings, less TLB reach -- with 2 GiB 1 %.  The
// price is paid when a workspace is sized: the driver clears what it hands out, about 15 ms per GB created (1.7 s for a 13 GB buffer at
// spread 8; spread 4 keeps half of the gain, 2 nothing).  hipMalloc whenever any of that fails.
// GBWT_HIP_VMM="0": always hipMalloc;  "<chunk MiB>:<spread, 0 = as much as half of the free memory allows, at most 8>:<min MiB>:<after>"
// (after = requests served as one hipMalloc before the buffer is rebuilt from spread chunks; 0 = spread at once).
struct VmmPolicy { size_t chunk = size_t(2048) << 20, min = size_t(4) << 30; unsigned spread = 0, after = 2; };
// GBWT_HIP_VMM, read when a workspace is created (the policy travels with its rows buffer)
inline VmmPolicy vmm_policy_from_env() {
    VmmPolicy p;
    if (const char *v = std::getenv("GBWT_HIP_VMM")) {
        unsigned long chunk = 0, spread = 0, min = 4096, after = 2;
        const int got = std::sscanf(v, "%lu:%lu:%lu:%lu", &chunk, &spread, &min, &after);
        if (got >= 1) { p.chunk = chunk << 20; p.spread = static_cast<unsigned>(spread); p.min = min << 20; }
        if (got >= 4) p.after = static_cast<unsigned>(after);
    }
    return p;
}

struct DeviceBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;
    std::vector<hipMemGenericAllocationHandle_t> chunks;   // empty: ptr comes from hipMalloc
    size_t reserved = 0;                                     // bytes of virtual range reserved at ptr (0: hipMalloc)
    size_t chunk_bytes = 0, mapped_chunks = 0;               // the first mapped_chunks chunks are mapped at ptr + i * chunk_bytes
    bool may_spread = false;                                 // the extracted rows of a workspace only: spreading the index arrays gains nothing (#25)
    VmmPolicy policy;                                        // how (set by the workspace from GBWT_HIP_VMM)
    unsigned uses = 0;                                       // requests the buffer has served at its present size
    ~DeviceBuffer() { release(); }
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    // hipFree waits for the work that may still use the memory; unmapping does not.  The rows of a workspace are handed out as raw
    // device pointers (gbwt_hip_paths, dist.device_view) that a consumer may still be reading on ANOTHER stream -- a torch kernel,
    // an RCCL send -- so a mapped buffer waits for the whole device before it goes.
    void release() noexcept {
        if (reserved) {
            (void)hipDeviceSynchronize();
            // one hipMemUnmap per hipMemMap: a single call over the whole range is not documented to undo several mappings, and
            // a chunk that stays mapped keeps its 2 GiB of VRAM for good
            for (size_t i = 0; i < mapped_chunks; i++) (void)hipMemUnmap(static_cast<char *>(ptr) + i * chunk_bytes, chunk_bytes);
            (void)hipMemAddressFree(ptr, reserved);
        } else if (ptr) (void)hipFree(ptr);
        for (auto h : chunks) (void)hipMemRelease(h);
        (void)hipGetLastError();
        chunks.clear();
        ptr = nullptr; bytes = 0; reserved = 0; chunk_bytes = 0; mapped_chunks = 0;
    }
    // Spreading costs seconds (the driver clears every chunk it hands out, and gives the unused ones back lazily: the NEXT large
    // allocation of the process waits for that), so a buffer starts as one hipMalloc -- what a one-shot extraction sees -- and is
    // rebuilt from spread chunks once it has served `policy.after` requests: a workspace that is used again and again (a server, the
    // timed passes of bench.py) pays once and gains on every pass after that.  The contents do not survive; callers reserve before
    // they write.
    void reserve(size_t need) {
        if (need <= bytes) {
            if (may_spread && reserved == 0 && policy.chunk != 0 && bytes >= policy.min && ++uses == policy.after) {
                const size_t want = bytes;
                release();
                if (!spread_chunks(want)) HIP_CHECK(hipMalloc(&ptr, want));
                bytes = want;
            }
            return;
        }
        release();
        uses = 0;
        const size_t want = std::max<size_t>(need, 256);
        if (may_spread && policy.chunk != 0 && want >= policy.min && policy.after == 0 && spread_chunks(want)) { bytes = want; return; }
        HIP_CHECK(hipMalloc(&ptr, want));
        bytes = want;
    }
    template <class T> T *as() const { return static_cast<T *>(ptr); }

private:
    // false (and nothing held) when the virtual-memory API does not cooperate
    bool spread_chunks(size_t want) noexcept {
        int device = 0;
        if (hipGetDevice(&device) != hipSuccess) return false;
        hipMemAllocationProp prop{};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = device;
        size_t granule = 0, free_bytes = 0, total_bytes = 0;
        if (hipMemGetAllocationGranularity(&granule, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || granule == 0) return false;
        if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess || want > free_bytes) return false;   // sizes out of a corrupt file: let hipMalloc say no
        const size_t chunk = (policy.chunk + granule - 1) / granule * granule, n = want / chunk + (want % chunk != 0 ? 1 : 0);
        // spread 0 = automatic: at most 8, and never more than HALF of the free memory in flight while the chunks are chosen -- other
        // contexts on the device (a second rank sharing the GPU, a torch allocator) must not see a spurious out-of-memory
        size_t spread = policy.spread;
        if (spread == 0) spread = std::min<size_t>(8, std::max<size_t>(1, free_bytes / 2 / (n * chunk)));
        // more chunks than needed, every spread-th kept: the kept ones lie `spread` chunks apart in whatever order the driver hands them out
        std::vector<hipMemGenericAllocationHandle_t> all;
        all.reserve(n * spread);
        for (size_t i = 0; i < n * spread; i++) {
            hipMemGenericAllocationHandle_t h;
            if (hipMemCreate(&h, chunk, &prop, 0) != hipSuccess) break;
            all.push_back(h);
        }
        (void)hipGetLastError();
        const size_t step = all.size() / n;     // >= 1 unless not even n chunks could be had
        for (size_t i = 0; i < all.size(); i++) {
            if (step != 0 && i % step == 0 && chunks.size() < n) chunks.push_back(all[i]);
            else (void)hipMemRelease(all[i]);
        }
        bool ok = chunks.size() == n && hipMemAddressReserve(&ptr, n * chunk, 0, nullptr, 0) == hipSuccess;
        if (ok) {
            reserved = n * chunk; chunk_bytes = chunk;
            for (size_t i = 0; i < n && ok; i++) {
                ok = hipMemMap(static_cast<char *>(ptr) + i * chunk, chunk, 0, chunks[i], 0) == hipSuccess;
                if (ok) mapped_chunks = i + 1;                 // a failure half-way unwinds exactly what was mapped
            }
            hipMemAccessDesc access{};
            access.location = prop.location;
            access.flags = hipMemAccessFlagsProtReadWrite;
            ok = ok && hipMemSetAccess(ptr, reserved, &access, 1) == hipSuccess;
        }
        if (!ok) { (void)hipGetLastError(); release(); }
        return ok;
    }
};

inline gbwt_hip_status status_of(const HipError &e) {
    std::string msg = std::string(e.what) + ": " + hipGetErrorString(e.err);
    if (e.err == hipErrorNoDevice || e.err == hipErrorInvalidDevice) return fail(GBWT_HIP_NO_DEVICE, msg);
    return fail(GBWT_HIP_DEVICE_ERROR, msg);
}

// The catch of an entry point that allocates by the size of a request: out of device memory is the caller's to act on (`what`: "the
// merge", "a locate request", ...), and the error state is cleared so that the next call starts clean
inline gbwt_hip_status status_of(const HipError &e, const char *what) {
    if (e.err != hipErrorOutOfMemory) return status_of(e);
    (void)hipGetLastError();
    return fail(GBWT_HIP_CAPACITY, std::string(what) + " does not fit in device memory: " + e.what);
}

// The checks every call that makes a handle starts with: its flags, and -- once its arguments are through -- a device to make it on
inline gbwt_hip_status check_open_flags(uint32_t flags) {
    if (flags == 0 || (flags & ~uint32_t(GBWT_HIP_OPEN_ALL)) != 0) return fail(GBWT_HIP_BAD_ARGUMENT, "flags: a non-empty set of GBWT_HIP_OPEN_EXTRACT | _SEARCH | _GFA");
    return GBWT_HIP_OK;
}
inline uint32_t normalised_caps(uint32_t flags) { return (flags & GBWT_HIP_OPEN_GFA) ? (flags | GBWT_HIP_OPEN_EXTRACT) : flags; }   // the lines are formatted from extracted rows
inline gbwt_hip_status require_device() {
    int count = 0;
    if (hipGetDeviceCount(&count) == hipSuccess && count != 0) return GBWT_HIP_OK;
    (void)hipGetLastError();
    return fail(GBWT_HIP_NO_DEVICE, "no HIP device available (libgbwt_hip has no CPU fallback)");
}

// Lippincott function: the status of the exception in flight.  No exception may cross the C ABI (the caller is Rust / C /
// ctypes: it would be std::terminate), so every extern "C" entry point that can throw wraps its body in
// GBWT_HIP_GUARD_BEGIN / GBWT_HIP_GUARD_END, whatever it already catches inside.
inline gbwt_hip_status status_of_current_exception() noexcept {
    try {
        throw;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_INVALID_DATA, e.what());
    } catch (const IoError &e) {
        return fail(GBWT_HIP_IO_ERROR, e.what());
    } catch (const Unsupported &e) {
        return fail(GBWT_HIP_UNSUPPORTED, e.what());
    } catch (const HipError &e) {
        return status_of(e);
    } catch (const std::bad_alloc &) {
        return fail(GBWT_HIP_DEVICE_ERROR, "out of host memory");
    } catch (const std::length_error &e) {   // a size taken from a file that no container can hold
        return fail(GBWT_HIP_INVALID_DATA, std::string("length error: ") + e.what());
    } catch (const std::exception &e) {
        return fail(GBWT_HIP_DEVICE_ERROR, std::string("unexpected exception: ") + e.what());
    } catch (...) {
        return fail(GBWT_HIP_DEVICE_ERROR, "unexpected exception");
    }
}
// The pinned staging buffers and streams of a workspace's device-to-host copies (capi_extract.hip: copy_to_host), made on first use.
struct HostCopier {
    static constexpr size_t CHUNK = size_t(16) << 20;
    struct Lane { void *pinned[2] = {nullptr, nullptr}; hipEvent_t landed[2] = {nullptr, nullptr}; hipStream_t stream = nullptr; };
    std::vector<Lane> lanes;
    std::mutex busy;
    HostCopier() = default;
    HostCopier(const HostCopier &) = delete;
    HostCopier &operator=(const HostCopier &) = delete;
    ~HostCopier();
    bool ensure(int device, unsigned threads);
};

#define GBWT_HIP_GUARD_BEGIN try {
#define GBWT_HIP_GUARD_END } catch (...) { return gbwt_hip::status_of_current_exception(); }

// gfa.hip: the chunk plan of the line formatter (chunks of GFA_LINE_CHUNK positions per row) for other passes over a batch of rows, and
// GBZ::has_node (src/gbz.rs:286-289) on the host image (makes the host's records on first use: HostIndex::ensure_records)
void launch_chunk_plan(const uint64_t *d_offsets, uint64_t n, uint64_t chunks_cap, uint64_t *d_chunk_counts, uint64_t *d_chunk_first, uint32_t *d_chunk_path, void *d_temp,
                       size_t temp_bytes, hipStream_t s);
bool node_exists(const HostIndex &h, uint64_t node_id);

// The full-width two-step blocks of a handle, built on first need, and a copy of its DeviceIndex with them put in (capi_open.hip)
const uint4 *ensure_cblocks(const gbwt_hip_index *index);
DeviceIndex with_cblocks(const gbwt_hip_index *ix);

}  // namespace gbwt_hip

// The GBWT_HIP_* settings of an open, read ONCE by gbwt_hip_open_file_flags / gbwt_hip_open_records_flags before the loader or any thread
// of the open starts, and kept on the handle: nothing else of an open looks at the environment (getenv is not safe against a concurrent
// setenv, and the early copy, the tail thread and the loader's jobs run next to the caller).  Unset = std::nullopt where it matters whether
// a setting is there at all, or where its default depends on the index.
struct OpenKnobs {
    bool seq_len = true;                               // GBWT_HIP_SEQ_LEN (0: no lengths, no samples)
    std::optional<uint32_t> sample_interval;           // GBWT_HIP_SAMPLE_INTERVAL (0: no samples; unset: by the size of the index, and coarse samples may be kept)
    std::optional<uint32_t> sample_coarse;             // GBWT_HIP_SAMPLE_COARSE (unset: nominal interval / 512)
    bool serial_samples = false;                       // GBWT_HIP_SERIAL_SAMPLES: a walk of every sequence instead of checkpoints
    bool two_pass = false;                             // GBWT_HIP_TWO_PASS_OPEN: lengths, then samples, by two walks of every sequence
    bool orientation_check = false;                    // GBWT_HIP_ORIENTATION_CHECK: fingerprints even where samples make them unnecessary
    std::optional<double> checkpoint_gap;              // GBWT_HIP_CHECKPOINT_GAP (unset: by the interval and the chains)
    std::optional<uint32_t> checkpoint_cap;            // GBWT_HIP_CHECKPOINT_CAP (unset: the interval)
    std::optional<uint32_t> chains;                    // GBWT_HIP_CHAINS (unset: CHAIN_MAX, and a handful of chained records are linked again without)
    uint32_t gather_limit = 1u << 21;                  // GBWT_HIP_GATHER_LIMIT: the counts of the packed blocks (0: none; tests lower it)
    uint32_t lookahead_hops = 15;                      // GBWT_HIP_LOOKAHEAD_HOPS
    bool walk_tables = true, deep_tables = true, compact_tables = true;   // GBWT_HIP_WALK_TABLES / _DEEP_TABLES / _COMPACT_TABLES (0 switches off)
    std::optional<uint64_t> table_bytes;               // GBWT_HIP_TABLE_BYTES (unset: by the device's memory)
    bool line_cache = true;                            // GBWT_HIP_LINE_CACHE (0: requests size their lines themselves)
    uint32_t locate_interval = 64;                     // GBWT_HIP_LOCATE_INTERVAL: expected records between two sampled ones of the locate index (1: every record, 0: none)
    bool trace = false;                                // GBWT_HIP_TRACE_OPEN set (any value): phase timings on stderr
    static OpenKnobs from_env() {
        OpenKnobs k;
        const auto on = [](const char *name) { const char *v = std::getenv(name); return !(v && std::atoi(v) == 0); };     // "0" switches off
        const auto forced = [](const char *name) { const char *v = std::getenv(name); return v && std::atoi(v) != 0; };  // anything but "0" switches on
        k.seq_len = on("GBWT_HIP_SEQ_LEN");
        if (const char *v = std::getenv("GBWT_HIP_SAMPLE_INTERVAL")) k.sample_interval = static_cast<uint32_t>(std::max(0, std::atoi(v)));
        if (const char *v = std::getenv("GBWT_HIP_SAMPLE_COARSE")) k.sample_coarse = static_cast<uint32_t>(std::max(1, std::atoi(v)));
        k.serial_samples = forced("GBWT_HIP_SERIAL_SAMPLES");
        k.two_pass = forced("GBWT_HIP_TWO_PASS_OPEN");
        k.orientation_check = forced("GBWT_HIP_ORIENTATION_CHECK");
        if (const char *v = std::getenv("GBWT_HIP_CHECKPOINT_GAP")) k.checkpoint_gap = std::max(2.0, std::atof(v));
        if (const char *v = std::getenv("GBWT_HIP_CHECKPOINT_CAP")) k.checkpoint_cap = static_cast<uint32_t>(std::max(1, std::atoi(v)));
        if (const char *v = std::getenv("GBWT_HIP_CHAINS")) k.chains = static_cast<uint32_t>(std::min<long>(gbwt_hip::CHAIN_MAX, std::max<long>(0, std::atol(v))));
        if (const char *v = std::getenv("GBWT_HIP_GATHER_LIMIT")) k.gather_limit = static_cast<uint32_t>(std::min<long>(1l << 21, std::max<long>(0, std::atol(v))));
        if (const char *v = std::getenv("GBWT_HIP_LOOKAHEAD_HOPS")) k.lookahead_hops = static_cast<uint32_t>(std::max(0, std::atoi(v)));
        k.walk_tables = on("GBWT_HIP_WALK_TABLES"); k.deep_tables = on("GBWT_HIP_DEEP_TABLES"); k.compact_tables = on("GBWT_HIP_COMPACT_TABLES");
        if (const char *v = std::getenv("GBWT_HIP_TABLE_BYTES")) k.table_bytes = std::strtoull(v, nullptr, 10);
        k.line_cache = on("GBWT_HIP_LINE_CACHE");
        if (const char *v = std::getenv("GBWT_HIP_LOCATE_INTERVAL")) k.locate_interval = static_cast<uint32_t>(std::min<long>(1l << 30, std::max<long>(0, std::atol(v))));
        k.trace = std::getenv("GBWT_HIP_TRACE_OPEN") != nullptr;
        return k;
    }
    // GBWT_HIP_LAZY_HOST_RECORDS, once per process: 0 = an open from a file makes the host's copy of the records in the loader's background
    static bool lazy_host_records() {
        static const bool lazy = [] { const char *e = std::getenv("GBWT_HIP_LAZY_HOST_RECORDS"); return !(e && e[0] == '0'); }();
        return lazy;
    }
};

// The GBWT_HIP_* tuning / measurement switches of an extraction, read ONCE when the workspace is created: gbwt_hip_extract_device
// itself never looks at the environment (getenv is not safe against a concurrent setenv, and several host threads extract from one
// index at the same time, each with its own workspace -- include/gbwt_hip.h).  -1 = not set: the library's default for the batch.
struct ExtractKnobs {
    int direct = 1, segments = 1, both_ends = 1;             // GBWT_HIP_DIRECT / _SEGMENTS / _BOTH_ENDS (0 switches the feature off)
    int all4 = 1;                                             // GBWT_HIP_ALL4: 0 = the uniform loop counts every node it stages (rounds 1-3)
    int sample_stride = -1;                                   // GBWT_HIP_SAMPLE_STRIDE: a walker per this many samples of a row; -1 = by the size of the batch (gbwt_hip_extract_device)
    int defer_total = 1;                                      // GBWT_HIP_DEFER_TOTAL: 0 = every request waits for the total of its row lengths before it launches the walk (rounds 1-3)
    int fused_offsets = 1;                                    // GBWT_HIP_FUSED_OFFSETS: 0 = the offsets of a batch of equally long rows come from k_row_offsets in front of the walk, as every batch's did until round 6 (WalkArgs::uniform_len)
    int ring_slots = -1, helper_naps = -1, xcd_map = -1, uniform_loop = -1, packed_blocks = -1, row_piece = -1, catch_up = -1, headroom = 0;
    int gather_reach = -1;                                    // GBWT_HIP_GATHER_REACH: look-ahead of mixed waves (WalkArgs::gather_reach); -1 = by the index (rows per record), 0 = none
    bool wide_addresses = false;                              // GBWT_HIP_WIDE_ADDRESSES set (any value)
    uint32_t debug = 0;                                       // GBWT_HIP_DEBUG_DRY_ROWS (measurement switches, WalkArgs::debug)
    unsigned copy_threads = 8;                                // GBWT_HIP_COPY_THREADS
    uint64_t locate_sort_piece = 0x7FFFFFFFull;               // GBWT_HIP_LOCATE_SORT_PIECE: items of one radix sort of a unique locate request (hipcub counts in int; tests lower it)
    static ExtractKnobs from_env() {
        ExtractKnobs k;
        const auto num = [](const char *name, int unset) { const char *v = std::getenv(name); return v ? std::atoi(v) : unset; };
        k.direct = num("GBWT_HIP_DIRECT", 1); k.segments = num("GBWT_HIP_SEGMENTS", 1); k.both_ends = num("GBWT_HIP_BOTH_ENDS", 1);
        k.ring_slots = num("GBWT_HIP_RING_SLOTS", -1); if (k.ring_slots != 32 && k.ring_slots != 64 && k.ring_slots != 128) k.ring_slots = -1;
        k.helper_naps = std::max(-1, num("GBWT_HIP_HELPER_NAPS", -1));
        k.xcd_map = num("GBWT_HIP_XCD_MAP", -1); k.uniform_loop = num("GBWT_HIP_UNIFORM_LOOP", -1); k.packed_blocks = num("GBWT_HIP_PACKED_BLOCKS", -1);
        k.catch_up = num("GBWT_HIP_CATCH_UP", -1);
        k.gather_reach = std::min(64, std::max(-1, num("GBWT_HIP_GATHER_REACH", -1)));
        k.sample_stride = num("GBWT_HIP_SAMPLE_STRIDE", -1);
        k.defer_total = num("GBWT_HIP_DEFER_TOTAL", 1);
        k.fused_offsets = num("GBWT_HIP_FUSED_OFFSETS", 1);
        k.all4 = num("GBWT_HIP_ALL4", 1);
        k.headroom = std::min(32, std::max(0, num("GBWT_HIP_HEADROOM", 0)));
        k.row_piece = num("GBWT_HIP_ROW_PIECE", -1); if (k.row_piece != 0 && k.row_piece != 16 && k.row_piece != 32) k.row_piece = -1;
        k.wide_addresses = std::getenv("GBWT_HIP_WIDE_ADDRESSES") != nullptr;
        k.debug = static_cast<uint32_t>(num("GBWT_HIP_DEBUG_DRY_ROWS", 0));
        k.copy_threads = static_cast<unsigned>(std::min(64, std::max(1, num("GBWT_HIP_COPY_THREADS", 8))));
        k.locate_sort_piece = static_cast<uint64_t>(std::max(1, num("GBWT_HIP_LOCATE_SORT_PIECE", 0x7FFFFFFF)));
        return k;
    }
};

struct gbwt_hip_index {
    gbwt_hip::HostIndex host;
    int device = 0;
    OpenKnobs knobs;                      // the open's settings (gbwt_hip_open_*_flags)
    bool lean_extract = false;           // opened without SEARCH and no record needs the generic decoder: desc_raw was given back after the open (capi_open.hip: open_common)
    uint64_t slow_records = ~uint64_t(0); // non-empty records whose walk descriptor says "generic decoder" (k_link_desc2's count; ~0 = not counted)
    uint32_t caps = GBWT_HIP_OPEN_ALL;   // what the handle was opened for (gbwt_hip_open_*_flags): which arrays exist, which entry points answer
    uint64_t table_positions = 0;     // BWT positions in records with LF tables (outdegree > 2)
    gbwt_hip::DeviceBuffer data, starts, endmarker, desc, desc_raw, block_base, blocks, desc2, cblocks, gblocks, tables, wtables, wtables_deep, seq_len, samples, sample_base;
    gbwt_hip::DeviceBuffer label_len;   // GBZ only: label length per potential node (0 for nodes that do not exist)
    // GBZ with a node-to-segment translation (src/graph.rs:186-218), flattened for the line formatter:
    gbwt_hip::DeviceBuffer seg_of;        // u32 per node id < mapping_len: segment holding the node (~0 before the first segment)
    gbwt_hip::DeviceBuffer seg_start;     // u32 per segment + 1: first node id of the segment, last = mapping_len
    gbwt_hip::DeviceBuffer seg_name_off;  // u64 per segment + 1: offsets into seg_names
    gbwt_hip::DeviceBuffer seg_names;     // segment names, concatenated
    gbwt_hip::DeviceBuffer seg_seq_len;   // u64 per segment: length of the segment's sequence
    gbwt_hip::DeviceBuffer node_real;     // u8 per node id < mapping_len: GBZ::has_node
    // GFA line headers, one table per line mode (0 = P-line named by the contig, 1 = W-line, 2 = P-line with the PanSN name): for every path of
    // the metadata the bytes of its line up to the node tokens -- for a W-line up to and including "<fragment>\t"; the end coordinate
    // (fragment + summed label lengths, path_to_w_line, src/bin/gbunzip.rs:532-540) is only known once the path has been walked and is
    // appended by the device.  Built once at open (gfa.hip: upload_label_lengths), so that a request formats its lines without the host.
    gbwt_hip::DeviceBuffer line_prefix[3], line_prefix_off[3], line_fragment;
    std::vector<char> host_line_prefix[3];
    std::vector<uint64_t> host_line_prefix_off[3];
    // LINE CACHE (gfa.hip): what the GFA line of a path is made of -- the text bytes of its node tokens, chunk by chunk, and its summed label
    // lengths (the W-line's end coordinate) -- is a property of the index, not of the request.  Round 5 let the first request that formats a
    // path leave them here; since round 6 ONE walk at open fills them for every path (fill_line_cache_at_open; kernels.hpp: LineCacheFill), so
    // that no request sizes a line: the node ids cross HBM twice (written by the walk, read by the formatter), never three times.
    // 8 bytes per 4 096 path positions + 16 per path.  Absent (-1) without sequence samples, for graphs with a node-to-segment translation
    // and with GBWT_HIP_LINE_CACHE=0: requests then size their lines themselves (k_chunk_stats).
    gbwt_hip::DeviceBuffer lc_chunk_first, lc_text, lc_path;    // u64[paths + 1]: first chunk of every path; u64 per chunk: W-token bytes of the path in front of it; u64[2] per path: {W-token bytes, summed label lengths}
    int lc_state = 0;                                             // 1 = filled at open, -1 = not for this index (written before the handle is handed out)
    std::vector<uint32_t> host_seq_len;   // host copy of seq_len (empty when the lengths are not known): sizes byte-bounded batches of a whole-file write
    // NODE LABELS IN HBM, made by the first request for bases (sequences.hip: ensure_labels), never by an open: the bytes of every potential
    // node's label (+ 64 zero bytes, so that the aligned dword loads of the bases kernel may read past the last one) and u64 offsets[nodes + 1].
    // One upload per handle whichever thread asks first (gbwt_hip_memory_usage counts them once labels_built.made()).
    mutable gbwt_hip::LazyBuild labels_built;
    mutable gbwt_hip::DeviceBuffer label_bytes, label_off;
    mutable uint64_t max_label_len = 0;
    // WEAKLY CONNECTED COMPONENTS IN HBM (capi_graph.hip: ensure_components), made by the first call that asks for them, never by an open:
    // the component of every node slot, the CSR of the components (u64 offsets, u32 node ids) and the component of every path; the path
    // components on the host as well (what select_paths reads).  Once per handle whichever thread asks first.
    mutable gbwt_hip::LazyBuild components_built;
    mutable gbwt_hip::DeviceBuffer comp_of, comp_offsets, comp_nodes, comp_paths;
    mutable gbwt_hip::ComponentGeometry comp_geometry{0, 0};
    mutable uint64_t comp_count = 0, comp_node_count = 0;
    mutable std::vector<uint32_t> host_path_component;
    mutable gbwt_hip_components_times comp_times{};
    // THE LOCATE INDEX IN HBM (locate.hip, capi_locate.hip: ensure_locate), made by the first locate call, never by an open: the table base of
    // every record (u64, LOCATE_NONE where the record is not sampled), the sequence id of every position of a sampled record (u32) and the
    // sorted end entries of the sequences.  Once per handle whichever thread and workspace asks first; a build that fails keeps nothing.
    mutable gbwt_hip::LazyBuild locate_built;
    mutable gbwt_hip::DeviceBuffer loc_base, loc_table, loc_end_keys, loc_end_ids;
    mutable gbwt_hip::LocateIndex loc{nullptr, nullptr, nullptr, nullptr, 0, 0};
    mutable uint64_t loc_sampled_records = 0;
    mutable float loc_build_ms = 0;
    mutable uint32_t loc_build_launches = 0;
    gbwt_hip::DeviceIndex dev{};
    // The full-width two-step blocks (cblocks, as large as gblocks: 1.7 GB on the headline index) are only read by the loops for records
    // whose counts do not fit the packed half-blocks, by the pool-output kernel and by the serial walks at open: built at open when one of
    // those is certain to run, else on the first request that needs them (ensure_cblocks; once, whichever thread comes first).
    mutable gbwt_hip::LazyBuild cblocks_built;
    bool packed_blocks = false;       // gblocks holds the packed half-blocks (set by the open's walk layout, capi_open.hip: layout_walks; false: a handle
                                      // not opened for extraction, an index too large for 32-bit half-block indices, or GBWT_HIP_GATHER_LIMIT=0)
    uint32_t max_samples = 0;         // the largest number of samples of a sequence
    uint32_t sample_coarse = 1;       // the samples are this many times finer than a batch of the whole index wants: extractions stride over them (capi_extract.hip)
    std::vector<uint32_t> sample_counts;   // samples of every sequence (host copy: an extraction looks whether its rows all have the same number)
    uint32_t uniform_samples = 0;     // every sequence has this many samples (0: they differ): the walkers of an extraction are then w = segment * n + row
    bool starts_uploaded = false;         // ... and the record starts
    bool record_bytes_uploaded = false;   // gbwt_hip_open_file has copied the record bytes to `data` while the loader was still decoding
    gbwt_hip_open_times times{};      // where the time of the open went (gbwt_hip_get_open_times)
    gbwt_hip_build_info build_info{}; // the construction behind the handle (capi_build.hip); zeros for a handle that was opened from a file or from records
    gbwt_hip_gfa_info gfa_info{};     // the parse behind a handle made from GFA (capi_gfa_build.hip); zeros for every other handle
    gbwt_hip_gfa_translation_info gfa_translation_info{};   // its translation, if it made one
    gbwt_hip_merge_info merge_info{};   // the merge behind the handle (capi_merge.hip); zeros for every other handle
    gbwt_hip_remove_info remove_info{}; // the removal behind the handle (capi_remove.hip); zeros for every other handle
    uint32_t uniform_len = 0;         // every sequence has this many nodes (0: lengths differ, or unknown): an extraction then knows its offsets without asking the device
    bool orientation_pairs = false;   // verified at open: sequence 2k + 1 is sequence 2k reversed (rows can be filled from both ends)
    gbwt_hip_stats stats{};
};

struct gbwt_hip_workspace {
    const gbwt_hip_index *index = nullptr;
    ExtractKnobs knobs;
    hipStream_t stream = nullptr;
    uint64_t *pinned_words = nullptr;         // four words of pinned host memory: the total and extremes of a request whose rows are sized after its launch (capi_extract.hip)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t qev[2] = {nullptr, nullptr};   // around the kernel(s) of the last navigation / search call
    hipEvent_t gev[2] = {nullptr, nullptr};   // around the formatting of the last GFA lines request (behind its walk)
    bool timed = false, query_timed = false, lines_timed = false;
    uint64_t last_n = 0, last_total = 0;   // shape of the last device-resident extraction
    uint32_t walk_mode = gbwt_hip::WALK_TWO_STEP, paths_per_wave = 0, small_record = 16;   // paths_per_wave 0 = automatic
    gbwt_hip::DeviceBuffer seq_ids, lengths, offsets, head, pool, next, counters, nodes, scan_temp;
    gbwt_hip::DeviceBuffer order_keys, order_rows, order_counts, order_level, order_temp;   // walker order of a segmented extraction
    gbwt_hip::DeviceBuffer in_a, in_b, out_a, out_valid, follow_off;  // search staging
    gbwt_hip::DeviceBuffer gfa_a, gfa_b, gfa_c, gfa_text, gfa_text2, gfa_valid, gfa_chunk_first, gfa_chunks, gfa_plan;  // GFA line formatting (gfa_text2: the second text buffer of a pipelined whole-file write)
    // What the device-resident results answer.  The C idiom "size query, then the same call with a buffer" (gbwt_hip_extract,
    // _follow, _path_lines) must not compute twice: a call that repeats the request of the results still in the workspace
    // copies them out.  Keys are host copies of the ids / states of the request.
    bool extract_cached = false, follow_cached = false, lines_cached = false;
    std::vector<uint64_t> extract_key, lines_key;
    std::vector<uint8_t> follow_key;
    int follow_backward = 0, lines_mode = 0, lines_slot = 0;
    // Bases of paths (sequences.hip): text and row offsets of the last gbwt_hip_path_sequences* request (seq_text2: the second text buffer of a
    // pipelined whole-file write), the request they answer, and events around its sizing (sev[0] .. sev[1]) and its bases kernel (sev[1] .. sev[2]).
    gbwt_hip::DeviceBuffer seq_text, seq_text2, seq_offsets;
    bool seq_cached = false, seq_timed = false;
    std::vector<uint64_t> seq_key;
    int seq_reverse = 0, seq_endmarker = -1, seq_slot = 0;
    uint64_t seq_total = 0;
    hipEvent_t sev[3] = {nullptr, nullptr, nullptr};
    // Tags of a suffix array (tags.hip).  The PLAN of the last list of path ids: for every position of the text's walk -- the nodes of the rows and
    // one endmarker position behind each -- its node (tag_node, u32) and its text offset (tag_off, u64, one more entry = the text length), and
    // the sampled top level (tag_top: the position that holds text offset h << TAG_SHIFT; u32, u64 from 2^32 positions).  tag_rows: the text
    // offset of every row (+ the text length) on the host.  tag_state: run count, last tags and the out-of-range flag of a request;
    // tag_sa* / tag_out*: the staging of the host and file forms.  Times of the last request: the plan's are kept with the plan.
    gbwt_hip::DeviceBuffer tag_node, tag_off, tag_top, tag_state, tag_sa, tag_sa2, tag_out, tag_out2;
    bool tag_planned = false, tag_timed = false, tag_wide = false;
    std::vector<uint64_t> tag_key, tag_rows;
    uint64_t tag_positions = 0, tag_text_len = 0;
    float tag_walk_ms = 0, tag_plan_ms = 0, tag_gather_ms = 0;
    hipEvent_t tev[2] = {nullptr, nullptr};
    // Reference positions (refpos.hip, capi_refpos.hip).  Scratch of the last request, per position (node of its rows): rp_off (u64 bases in
    // front of it), rp_mark (u64: its label length, then whether it is kept), rp_jump (two u32 jump arrays, then its u64 slot); rp_rows: the
    // sequence ids, path ids and segment counts of the rows; rp_flags: a word per pointer-doubling round, one for the walk.  Results:
    // rp_paths[n], rp_positions[rp_total], and the request they answer (rp_key, rp_interval).  Events around the selection (rev[0] ..
    // rev[1]) and the walk that writes the positions (rev[1] .. rev[2]).
    gbwt_hip::DeviceBuffer rp_off, rp_mark, rp_jump, rp_rows, rp_flags, rp_paths, rp_positions;
    bool rp_cached = false, rp_timed = false;
    std::vector<uint64_t> rp_key;
    uint64_t rp_interval = 0, rp_total = 0;
    uint32_t rp_rounds = 0, rp_launches = 0;
    float rp_walk_ms = 0, rp_select_ms = 0, rp_offsets_ms = 0;
    hipEvent_t rev[3] = {nullptr, nullptr, nullptr};
    // The graph API (topology.hip, capi_topology.hip).  Edge / link rows of the last request: its queries (tp_ids u64, tp_orient u8; tp_seg: the
    // segment ids of a links request), counts, offsets, edges, the query of every edge (tp_rows, links only), valid bytes and the list of long
    // rows (tp_big); for links the cuts, the link offsets and the links.  tp_key: the request they answer (the fill call after a size query).
    gbwt_hip::DeviceBuffer tp_ids, tp_orient, tp_seg, tp_counts, tp_off, tp_edges, tp_rows, tp_valid, tp_big, tp_cut, tp_loff, tp_links;
    bool tp_cached = false;
    std::vector<uint8_t> tp_key;
    int tp_links_request = 0, tp_predecessors = 0;
    uint64_t tp_n = 0, tp_total = 0;
    // Graph lines: the items of the S-lines (node or segment ids) and their line offsets, the edge rows of all (node | segment, orientation)
    // pairs with the query of every edge and the offsets of their L-lines -- kept from the first request (gt_sized), so that a later one only
    // formats -- and the text.  Events: gt_ev[0] .. [1] sizing, [1] .. [2] S-lines, [2] .. [3] L-lines.
    gbwt_hip::DeviceBuffer gt_items, gt_soff, gt_edges, gt_rows, gt_loff, gt_text;
    bool gt_sized = false, gt_text_valid = false, gt_timed = false, gt_translated = false, gt_sized_now = false;   // gt_sized_now: the last request sized
    uint64_t gt_item_count = 0, gt_edge_count = 0, gt_sbytes = 0, gt_lbytes = 0, gt_links = 0;
    std::string gt_header;
    hipEvent_t gt_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // Locate (locate.hip, capi_locate.hip).  The rows of the last request -- lo_off / lo_ids / lo_valid, for a unique request lo_uoff and the
    // compacted ids -- live in buffers of their own: an edges / links request leaves them alone.  lo_states: the states of a request given on the
    // host; lo_counts, lo_keys, lo_sorted, lo_flag, lo_rank, lo_temp: scratch; lo_words: the flag word, a scan carry and the step counter;
    // lo_pos / lo_pos_ids / lo_pos_valid: a positions request.  lo_key: the request the rows answer (the fill call after a size query).
    // Events: lev[0] .. lev[1] the locate kernel, lev[1] .. lev[2] sort and compaction of a unique request.
    gbwt_hip::DeviceBuffer lo_states, lo_counts, lo_off, lo_ids, lo_valid, lo_keys, lo_sorted, lo_flag, lo_rank, lo_uoff, lo_temp, lo_words, lo_pos, lo_pos_ids, lo_pos_valid;
    bool lo_cached = false, lo_timed = false, lo_compacted = false;   // lo_compacted: lo_uoff holds the offsets of the rows (a unique request with ids)
    std::vector<uint8_t> lo_key;
    int lo_unique = 0;
    uint64_t lo_n = 0, lo_total = 0, lo_steps = 0;
    float lo_walk_ms = 0, lo_sort_ms = 0;
    hipEvent_t lev[3] = {nullptr, nullptr, nullptr};
    gbwt_hip::HostCopier copier;     // pinned staging of the large device-to-host copies
    uint64_t follow_total = 0, lines_total = 0;
    ~gbwt_hip_workspace() {
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
        for (auto &e : qev) if (e) (void)hipEventDestroy(e);
        for (auto &e : gev) if (e) (void)hipEventDestroy(e);
        for (auto &e : sev) if (e) (void)hipEventDestroy(e);
        for (auto &e : tev) if (e) (void)hipEventDestroy(e);
        for (auto &e : rev) if (e) (void)hipEventDestroy(e);
        for (auto &e : lev) if (e) (void)hipEventDestroy(e);
        for (auto &e : gt_ev) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
        if (pinned_words) (void)hipHostFree(pinned_words);
    }
};

namespace gbwt_hip {
// A handle with its settings and nothing else: the device, what it is opened for (caps decide which arrays the open makes) and the
// GBWT_HIP_* settings of the open, read here and nowhere else
inline std::unique_ptr<gbwt_hip_index> new_handle(int device, uint32_t flags) {
    std::unique_ptr<gbwt_hip_index> ix(new gbwt_hip_index);
    ix->device = device;
    ix->caps = normalised_caps(flags);
    ix->knobs = OpenKnobs::from_env();
    return ix;
}

// gbwt_hip_last_*_info, gbwt_hip_get_stats, gbwt_hip_get_open_times: a struct the open or a maker left on the handle
// (static, like fill_build_counters and extract_rows: a helper over the ABI's types adds no symbol to what the library exports)
template <class Info>
static gbwt_hip_status last_info(const gbwt_hip_index *ix, Info *out, Info gbwt_hip_index::*member) {
    if (!ix || !out) return fail(GBWT_HIP_BAD_ARGUMENT, "null argument");
    *out = ix->*member;
    return GBWT_HIP_OK;
}

// capi_open.hip: the open behind every handle -- device passes, GFA tables, line cache -- for a host image that is already filled (takes
// ownership; t_open: when the caller started, for the handle's open times).  Settings come with the handle (new_handle).
gbwt_hip_status open_host_index(std::unique_ptr<gbwt_hip_index> ix, gbwt_hip_index **out, std::chrono::steady_clock::time_point t_open);

// The labels of a handle as the kernels see them (sequences.hip, tags.hip): node v (GBWT-encoded, 2 id + o) has label bytes[off[s] .. off[s + 1])
// with s = (v & ~1 - first_node) / 2 (GBZ::graph_node_to_sequence, src/gbz.rs:246-255); a node outside [first_node, first_node + 2 n) has none.
struct Labels { const uint8_t *bytes; const uint64_t *off; uint64_t n; uint32_t first_node; };

__device__ __forceinline__ void label_of(const Labels &L, uint32_t node, uint64_t &lo, uint64_t &hi) {
    const uint32_t fwd = node & ~1u;
    const uint64_t s = (static_cast<uint64_t>(fwd) - L.first_node) / 2;
    if (fwd < L.first_node || s >= L.n) { lo = 0; hi = 0; return; }
    lo = L.off[s]; hi = L.off[s + 1];
}

// sequences.hip: the labels of a handle in HBM (made by the first request that needs them), and the test every entry point for bases and
// tags starts with (InvalidData for a bare GBWT or a handle without GBWT_HIP_OPEN_EXTRACT)
Labels labels_of(const gbwt_hip_index *ix);
void ensure_labels(const gbwt_hip_index *ix);
void require_bases_capable(const gbwt_hip_index *ix);

// Device -> pageable host memory over the workspace's copy threads (GBWT_HIP_COPY_THREADS, default 8), each with two pinned staging
// buffers and a stream of its own (capi_extract.hip)
void copy_to_host(gbwt_hip_workspace *ws, void *dst, const void *src, size_t bytes, size_t piece = HostCopier::CHUNK);
}
