// capi_extract.hip -- the C ABI of libgbwt_hip.so (include/gbwt_hip.h), part 2 of 3: workspaces and batched path extraction
// (gbwt_hip_extract*: SequenceIter / GBZ::path, src/gbwt.rs:253-261, 557-568, src/gbz.rs:461-466), the copies of results to the host, and
// the per-row checksums.  No CPU implementation of any compute entry point.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "capi_internal.hpp"
#include "extract_plan.hpp"
#include "scan.hpp"

using namespace gbwt_hip;

namespace {

// One request of gbwt_hip_extract_part_device, as its steps pass it on
struct Request {
    const gbwt_hip_index *ix;
    gbwt_hip_workspace *ws;
    const uint64_t *seq_ids;
    uint64_t n;
    uint32_t part, parts;
    size_t temp_bytes;         // of scratch.scan_temp, for a scan over n lengths
    gbwt_hip_paths *out;
};

// THE finish of every request that succeeds: what copy_result / path_sums / copy_path trust, the memo of whole rows (gbwt_hip_extract's
// fill call asks for whole rows: a part of them is never stored), and the caller's view of the rows
gbwt_hip_status finish(const Request &r, uint64_t total, bool store_memo) {
    ExtractState &e = r.ws->extract;
    e.timed = true; e.last_n = r.n; e.last_total = total;
    if (store_memo) e.memo.store({{r.seq_ids, r.n * sizeof(uint64_t)}}, {});
    r.out->d_offsets = e.offsets.as<uint64_t>(); r.out->d_nodes = e.nodes.as<uint32_t>(); r.out->total = total; r.out->n = r.n;
    return GBWT_HIP_OK;
}

// n empty rows: an empty CSR with all its events, so that the times of the request can be asked for like any other's
gbwt_hip_status empty_rows(const Request &r, bool store_memo) {
    ExtractState &e = r.ws->extract;
    hipStream_t s = r.ws->stream;
    HIP_CHECK(hipMemsetAsync(e.offsets.ptr, 0, (r.n + 1) * sizeof(uint64_t), s));
    e.nodes.reserve(sizeof(uint32_t));
    HIP_CHECK(hipEventRecord(e.ev[0], s)); HIP_CHECK(hipEventRecord(e.ev[1], s)); HIP_CHECK(hipEventRecord(e.ev[2], s));
    HIP_CHECK(hipStreamSynchronize(s));
    return finish(r, 0, store_memo);
}

// The walk of a direct request between ev[0] and ev[1], the end of the request (ev[2]) and the host's wait for it
void walk_and_wait(ExtractState &e, const DeviceIndex &dev, const WalkArgs &a, bool walk, hipStream_t s) {
    HIP_CHECK(hipEventRecord(e.ev[0], s));
    if (walk) launch_walk(dev, a, s);
    HIP_CHECK(hipEventRecord(e.ev[1], s));
    HIP_CHECK(hipEventRecord(e.ev[2], s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
}

PlanIndex plan_index(const gbwt_hip_index *ix) {
    PlanIndex p;
    p.sequences = ix->host.sequences; p.size = ix->host.size; p.records = ix->stats.records;
    p.has_samples = ix->dev.samples != nullptr;
    p.max_samples = ix->max_samples; p.sample_coarse = ix->sample_coarse; p.uniform_samples = ix->uniform_samples; p.uniform_len = ix->uniform_len;
    p.sample_counts = ix->sample_counts.data(); p.n_sample_counts = ix->sample_counts.size();
    p.orientation_pairs = ix->orientation_pairs; p.lean = ix->lean_extract; p.packed_blocks = ix->packed_blocks;
    return p;
}

// Lengths known: offsets first, then every lane writes into its row; in a bidirectional index two walkers per sequence, one from each
// end.  Every decision is extract_plan.hpp's; here are the launches, the copies and the waits.
gbwt_hip_status direct_rows(const Request &r) {
    const gbwt_hip_index *ix = r.ix;
    ExtractState &e = r.ws->extract;
    const ExtractKnobs &knobs = r.ws->knobs;
    hipStream_t s = r.ws->stream;
    const uint64_t n = r.n;
    const PlanIndex pi = plan_index(ix);
    const IdSummary ids = summarize_ids(r.seq_ids, n, pi);
    const uint64_t capacity = e.nodes.bytes / sizeof(uint32_t);
    const RowsPlan rows = plan_rows(knobs, pi, ids, n, r.part, r.parts, capacity);
    if (rows.empty_part) return empty_rows(r, false);
    DeviceIndex strided = ix->dev; strided.sample_stride = rows.stride;
    if (rows.parted) { strided.sample_part = r.part; strided.sample_parts = r.parts; }
    // lengths, offsets and extremes: one launch for the batch sizes there are, else a memset and three
    if (!rows.fused_offsets && !launch_row_offsets(strided, e.seq_ids.as<uint64_t>(), n, e.lengths.as<uint64_t>(), e.offsets.as<uint64_t>(), e.counters.as<uint32_t>(), s)) {
        HIP_CHECK(hipMemsetAsync(e.counters.ptr, 0, 4 * sizeof(uint32_t), s));
        if (rows.parted) launch_part_lengths(strided, e.seq_ids.as<uint64_t>(), n, e.lengths.as<uint64_t>(), e.counters.as<uint32_t>(), s);
        else launch_gather_lengths(ix->dev.seq_len, ix->dev.n_sequences, e.seq_ids.as<uint64_t>(), n, e.lengths.as<uint64_t>(), e.counters.as<uint32_t>(), s);
        launch_scan(e.lengths.as<uint64_t>(), e.offsets.as<uint64_t>(), n, r.ws->scratch.scan_temp.ptr, r.temp_bytes, s, knobs.scan_piece);
    }
    uint64_t total = rows.total;
    uint32_t max_len = rows.max_len;
    if (rows.defer) {
        e.pinned_words.ensure();
        HIP_CHECK(hipMemcpyAsync(e.pinned_words.p, e.offsets.as<uint64_t>() + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    } else if (!rows.all_valid) {
        uint32_t extremes[2] = {0, 0};   // the longest row, ~(the shortest)
        HIP_CHECK(hipMemcpyAsync(&total, e.offsets.as<uint64_t>() + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(extremes, e.counters.ptr, sizeof(extremes), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        max_len = extremes[0];
    }
    e.nodes.reserve(std::max<uint64_t>(total, 1) * sizeof(uint32_t));
    const WalkPlan p = plan_walk(knobs, pi, rows, ids.ids_valid, n, r.part, r.parts, max_len, capacity);
    if (p.refused)
        return fail(GBWT_HIP_UNSUPPORTED, "this handle was opened for extraction only and has given its raw descriptors back: walks that do not start from sequence samples (GBWT_HIP_SEGMENTS=0, more than 2^31 - 1 rows) need GBWT_HIP_OPEN_ALL");
    WalkArgs a{};
    a.seq_ids = e.seq_ids.as<uint64_t>(); a.n = n;
    a.mode = knobs.walk_mode;
    a.segments = p.segments;
    uint64_t walkers = p.walkers;
    if (p.same_segments) a.walkers = walkers;
    if (p.needs_order) {
        const size_t ob = walker_order_temp_bytes(n), sb = scan_temp_bytes(a.segments, knobs.scan_piece);
        e.order_keys.reserve(2 * n * sizeof(uint32_t)); e.order_rows.reserve(2 * n * sizeof(uint32_t));
        e.order_counts.reserve(a.segments * sizeof(uint64_t)); e.order_level.reserve((a.segments + 1ull) * sizeof(uint64_t));
        e.order_temp.reserve(std::max(ob, sb));
        const uint32_t *sorted_rows = nullptr;
        launch_walker_order(strided, e.seq_ids.as<uint64_t>(), n, a.segments, e.order_keys.as<uint32_t>(), e.order_rows.as<uint32_t>(),
                            e.order_counts.as<uint64_t>(), e.order_level.as<uint64_t>(), e.order_temp.ptr, ob, &sorted_rows, s);
        launch_scan(e.order_counts.as<uint64_t>(), e.order_level.as<uint64_t>(), a.segments, e.order_temp.ptr, sb, s, knobs.scan_piece);
        HIP_CHECK(hipMemcpyAsync(&walkers, e.order_level.as<uint64_t>() + a.segments, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        a.sorted_rows = sorted_rows; a.level = e.order_level.as<uint64_t>(); a.walkers = walkers;
    }
    a.paths_per_wave = p.paths_per_wave;
    a.helper_lanes = 64u;
    a.wide_addresses = p.wide_addresses;
    a.ring_slots = p.ring_slots;
    a.helper_naps = p.helper_naps;
    a.out_nodes = e.nodes.as<uint32_t>(); a.out_offsets = e.offsets.as<uint64_t>();
    a.xcd_map = p.xcd_map;
    a.uniform_loop = p.uniform_loop;
    a.catch_up = p.catch_up;
    a.gather_reach = p.gather_reach;
    a.all4 = p.all4;
    a.headroom = p.headroom;
    a.packed_blocks = p.packed_blocks;
    a.row_piece = p.row_piece;
    a.debug = p.debug;
    a.both_ends = p.both_ends;
    a.capacity = p.capacity;
    if (p.uniform_len) { a.uniform_len = p.uniform_len; a.fill_offsets = e.offsets.as<uint64_t>(); }
    DeviceIndex dev = a.packed_blocks ? ix->dev : with_cblocks(ix);
    dev.sample_stride = strided.sample_stride; dev.sample_part = strided.sample_part; dev.sample_parts = strided.sample_parts;
    walk_and_wait(e, dev, a, !rows.parted || (total != 0 && walkers != 0), s);   // (a part of nothing but empty stretches: no walkers)
    if (rows.defer) {
        total = e.pinned_words.p[0];
        if (total > capacity) {                              // the rows were too small and nobody walked: make them, walk
            e.nodes.reserve(total * sizeof(uint32_t));
            a.out_nodes = e.nodes.as<uint32_t>(); a.capacity = 0;
            walk_and_wait(e, dev, a, walkers != 0, s);
        }
    }
    return finish(r, total, !rows.parted);
}

// No sequence lengths, GBWT_HIP_DIRECT=0 or a tuned walk mode: whole rows into a pool of blocks, then compacted into the CSR
gbwt_hip_status pool_rows(const Request &r) {
    const gbwt_hip_index *ix = r.ix;
    ExtractState &e = r.ws->extract;
    const ExtractKnobs &knobs = r.ws->knobs;
    hipStream_t s = r.ws->stream;
    const uint64_t n = r.n;
    if (ix->lean_extract) return fail(GBWT_HIP_UNSUPPORTED, "this handle was opened for extraction only and has given its raw descriptors back: the pool-output walk modes need GBWT_HIP_OPEN_ALL");
    // The pool-output kernels walk whole rows and cannot cut them: as the header says for rows that cannot be cut, the LAST part is the
    // whole row and every earlier part is n empty rows -- never the whole row from every part (a gather of parts would then hold every
    // row `parts` times).
    if (r.parts > 1 && r.part + 1 < r.parts) return empty_rows(r, false);
    uint64_t pool_blocks = plan_pool_blocks(plan_index(ix), n, POOL_BLOCK_NODES);
    uint32_t flags = 0;
    WalkArgs a{};
    const DeviceIndex dev = knobs.walk_mode == WALK_TWO_STEP ? with_cblocks(ix) : ix->dev;   // the pool-output kernel walks on the full-width two-step blocks
    for (int attempt = 0; attempt < 8; attempt++) {
        if (pool_blocks >= POOL_NONE) return fail(GBWT_HIP_UNSUPPORTED, "path pool would exceed 2^32 blocks");
        e.pool.reserve(pool_blocks * POOL_BLOCK_NODES * sizeof(uint32_t));
        e.next.reserve(pool_blocks * sizeof(uint32_t));
        a.seq_ids = e.seq_ids.as<uint64_t>(); a.n = n;
        a.pool = e.pool.as<uint32_t>(); a.next = e.next.as<uint32_t>(); a.pool_blocks = static_cast<uint32_t>(pool_blocks);
        a.counter = e.counters.as<uint32_t>(); a.flags = e.counters.as<uint32_t>() + 1;
        a.head = e.head.as<uint32_t>(); a.lengths = e.lengths.as<uint64_t>();
        a.mode = knobs.walk_mode; a.small_record = knobs.small_record;
        a.paths_per_wave = plan_pool_paths_per_wave(knobs, n);
        a.pack16 = ix->stats.max_record_len < 65536 ? 1u : 0u;
        a.helper_lanes = 64u;
        a.wide_addresses = knobs.wide_addresses;
        HIP_CHECK(hipMemsetAsync(e.counters.ptr, 0, 4 * sizeof(uint32_t), s));
        HIP_CHECK(hipEventRecord(e.ev[0], s));
        launch_walk(dev, a, s);
        HIP_CHECK(hipEventRecord(e.ev[1], s));
        HIP_CHECK(hipMemcpyAsync(&flags, a.flags, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        launch_scan(a.lengths, e.offsets.as<uint64_t>(), n, r.ws->scratch.scan_temp.ptr, r.temp_bytes, s, knobs.scan_piece);
        HIP_CHECK(hipStreamSynchronize(s));
        HIP_CHECK(hipGetLastError());
        if (!(flags & FLAG_POOL_OVERFLOW)) break;
        pool_blocks *= 2;  // duplicate ids can exceed the distinct-id bound: grow and walk again
    }
    if (flags & FLAG_POOL_OVERFLOW) return fail(GBWT_HIP_DEVICE_ERROR, "path pool overflow");
    uint64_t total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, e.offsets.as<uint64_t>() + n, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    e.nodes.reserve(std::max<uint64_t>(total, 1) * sizeof(uint32_t));
    launch_compact(a, e.offsets.as<uint64_t>(), e.nodes.as<uint32_t>(), s);
    HIP_CHECK(hipEventRecord(e.ev[2], s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    return finish(r, total, true);
}

}  // namespace

extern "C" {

gbwt_hip_status gbwt_hip_workspace_create(const gbwt_hip_index *index, gbwt_hip_workspace **out) {
    GBWT_HIP_GUARD_BEGIN
    if (!index || !out) return fail(GBWT_HIP_BAD_ARGUMENT, "null argument");
    *out = nullptr;
    std::unique_ptr<gbwt_hip_workspace> ws(new gbwt_hip_workspace);
    ws->extract.nodes.may_spread = true;
    ws->extract.nodes.policy = vmm_policy_from_env();
    ws->knobs = ExtractKnobs::from_env();
    ws->index = index;
    HIP_CHECK(hipSetDevice(index->device));
    ws->stream.create(hipStreamNonBlocking);
    ws->extract.ev.ensure();
    ws->extract.counters.reserve(4 * sizeof(uint32_t));
    *out = ws.release();
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

void gbwt_hip_workspace_destroy(gbwt_hip_workspace *ws) { delete ws; }

gbwt_hip_status gbwt_hip_workspace_tune(gbwt_hip_workspace *ws, uint32_t walk_mode, uint32_t paths_per_wave, uint32_t small_record) {
    GBWT_HIP_GUARD_BEGIN
    if (!ws || walk_mode > WALK_ONE_STEP || paths_per_wave > 64) return fail(GBWT_HIP_BAD_ARGUMENT, "bad tuning values");
    ws->knobs.walk_mode = walk_mode; ws->knobs.paths_per_wave = paths_per_wave; ws->knobs.small_record = small_record;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

void *gbwt_hip_workspace_stream(gbwt_hip_workspace *ws) { return ws ? static_cast<void *>(ws->stream.s) : nullptr; }

gbwt_hip_status gbwt_hip_extract_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *seq_ids, uint64_t n,
                                        gbwt_hip_paths *out) {
    return gbwt_hip_extract_part_device(ix, ws, seq_ids, n, 0, 1, out);
}

gbwt_hip_status gbwt_hip_extract_part_device(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *seq_ids, uint64_t n,
                                             uint32_t part, uint32_t parts, gbwt_hip_paths *out) {
    GBWT_HIP_GUARD_BEGIN
    // 1. the workspace of this handle -- 2. and what copy_result / path_sums / copy_path trust of it: gone whatever becomes of this request,
    // one that is refused for its other arguments included, and set again only by finish()
    if (!ix || !ws || ws->index != ix || !out) return fail(GBWT_HIP_BAD_ARGUMENT, "null or mismatched index / workspace");
    ExtractState &e = ws->extract;
    e.memo.drop();
    e.timed = false; e.last_n = 0; e.last_total = 0;
    if (n && !seq_ids) return fail(GBWT_HIP_BAD_ARGUMENT, "null seq_ids");
    if (parts == 0 || part >= parts) return fail(GBWT_HIP_BAD_ARGUMENT, "part must be < parts");
    if (!(ix->caps & GBWT_HIP_OPEN_EXTRACT)) return fail(GBWT_HIP_BAD_ARGUMENT, "the handle was not opened for extraction (GBWT_HIP_OPEN_EXTRACT)");
    // GBWT::sequence: id >= sequences -> no iterator (src/gbwt.rs:254-256).  "Not found" is a value here as well: such an id
    // gets an empty row (the kernels test the id), the rest of the batch is extracted; callers tell None from an empty
    // sequence by id < sequences.
    try {
        // 3. the ids on the device, room for what every body needs
        HIP_CHECK(hipSetDevice(ix->device));
        hipStream_t s = ws->stream;
        e.seq_ids.reserve(std::max<uint64_t>(n, 1) * sizeof(uint64_t));
        e.lengths.reserve(std::max<uint64_t>(n, 1) * sizeof(uint64_t));
        e.offsets.reserve((n + 1) * sizeof(uint64_t));
        e.head.reserve(std::max<uint64_t>(n, 1) * sizeof(uint32_t));
        const Request r{ix, ws, seq_ids, n, part, parts, scan_temp_bytes(n, ws->knobs.scan_piece), out};
        ws->scratch.scan_temp.reserve(r.temp_bytes);
        HIP_CHECK(hipEventRecord(e.ev[3], s));   // everything the extraction puts on the stream lies between ev[3] and ev[2]
        if (n) HIP_CHECK(hipMemcpyAsync(e.seq_ids.ptr, seq_ids, n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        // 4. one of three bodies, 5. each of which ends in finish()
        if (n == 0) return empty_rows(r, true);              // nothing asked for: an empty CSR, whatever the handle holds
        if (ix->dev.seq_len && ws->knobs.walk_mode == WALK_TWO_STEP && ws->knobs.direct != 0) return direct_rows(r);
        return pool_rows(r);
    } catch (const HipError &err) {
        return status_of(err);
    }
    GBWT_HIP_GUARD_END
}

}  // extern "C"

namespace gbwt_hip {

// Device -> pageable host memory for the large results (13 GB of node ids on the headline index, gigabytes of GFA lines).  A plain
// hipMemcpy stages through one pinned buffer on one thread and also pays the first-touch page faults of a fresh destination on that
// thread (0.5 - 1.1 s for 13.3 GB; 2.4 GB/s for a gigabyte of W-lines).  Here a few threads take alternate 16 MiB chunks, each with two
// pinned buffers and a stream of its own: the copy of a thread's next chunk over PCIe runs under its memcpy of the present one out of
// the pinned buffer, and the threads' page faults run side by side.  Buffers and streams belong to the workspace (HostCopier) and are
// made once: allocating pinned memory per call cost as much as copying a gigabyte.
HostCopier::~HostCopier() {
    for (Lane &l : lanes) {
        for (void *p : l.pinned) if (p) (void)hipHostFree(p);
        for (hipEvent_t e : l.landed) if (e) (void)hipEventDestroy(e);
        if (l.stream) (void)hipStreamDestroy(l.stream);
    }
}

bool HostCopier::ensure(int device, unsigned threads) {
    if (hipSetDevice(device) != hipSuccess) return false;
    while (lanes.size() < threads) {
        Lane l;
        bool ok = hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking) == hipSuccess;
        for (int b = 0; b < 2 && ok; b++) ok = hipHostMalloc(&l.pinned[b], CHUNK, hipHostMallocDefault) == hipSuccess && hipEventCreateWithFlags(&l.landed[b], hipEventDisableTiming) == hipSuccess;
        lanes.push_back(l);            // (its destructor frees whatever a failed lane got)
        if (!ok) { (void)hipGetLastError(); return false; }
    }
    return true;
}

void copy_to_host(gbwt_hip_workspace *ws, void *dst, const void *src, size_t bytes, size_t piece) {
    const size_t CHUNK = std::min(std::max<size_t>(piece, 4096), HostCopier::CHUNK);
    const int device = ws->index->device;
    const unsigned threads = ws->knobs.copy_threads;
    if (bytes < 4 * CHUNK || threads < 2) { HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return; }
    std::lock_guard<std::mutex> guard(ws->copier.busy);
    if (!ws->copier.ensure(device, threads)) { HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return; }
    const size_t chunks = (bytes + CHUNK - 1) / CHUNK;
    std::atomic<size_t> next{0};
    std::atomic<int> failed{0};
    auto work = [&](unsigned t) {
        HostCopier::Lane &l = ws->copier.lanes[t];
        if (hipSetDevice(device) != hipSuccess) { failed = 1; return; }
        auto issue = [&](size_t c, int b) {
            const size_t at = c * CHUNK, len = std::min(CHUNK, bytes - at);
            return hipMemcpyAsync(l.pinned[b], static_cast<const char *>(src) + at, len, hipMemcpyDeviceToHost, l.stream) == hipSuccess &&
                   hipEventRecord(l.landed[b], l.stream) == hipSuccess;
        };
        size_t cur = next++;
        int b = 0;
        if (cur >= chunks) return;
        if (!issue(cur, b)) { failed = 1; return; }
        while (!failed) {
            const size_t nxt = next++;
            if (nxt < chunks && !issue(nxt, b ^ 1)) { failed = 1; break; }
            if (hipEventSynchronize(l.landed[b]) != hipSuccess) { failed = 1; break; }
            std::memcpy(static_cast<char *>(dst) + cur * CHUNK, l.pinned[b], std::min(CHUNK, bytes - cur * CHUNK));
            if (nxt >= chunks) break;
            cur = nxt; b ^= 1;
        }
        (void)hipStreamSynchronize(l.stream);
    };
    const unsigned used = static_cast<unsigned>(std::min<size_t>(threads, chunks));
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < used; t++) pool.emplace_back(work, t);
    work(0);
    for (auto &t : pool) t.join();
    if (failed) { (void)hipGetLastError(); HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); }   // whatever went wrong: the plain way, which reports it
}


}  // namespace gbwt_hip

extern "C" {

gbwt_hip_status gbwt_hip_extract(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *seq_ids, uint64_t n,
                                 uint64_t *out_offsets, uint32_t *out_nodes, uint64_t capacity, uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (!out_offsets || !total) return fail(GBWT_HIP_BAD_ARGUMENT, "null output");
    gbwt_hip_paths p{};
    // the fill call after a size query (or after gbwt_hip_extract_device) with the same ids: the rows are still in the workspace
    if (ix && ws && ws->index == ix && ws->extract.memo.matches({{seq_ids, n * sizeof(uint64_t)}}, {})) {
        p.d_offsets = ws->extract.offsets.as<uint64_t>(); p.d_nodes = ws->extract.nodes.as<uint32_t>(); p.total = ws->extract.last_total; p.n = n;
    } else {
        gbwt_hip_status st = gbwt_hip_extract_device(ix, ws, seq_ids, n, &p);
        if (st != GBWT_HIP_OK) return st;
    }
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        HIP_CHECK(hipMemcpy(out_offsets, p.d_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        *total = p.total;
        if (!out_nodes) return GBWT_HIP_OK;
        if (capacity < p.total) return fail(GBWT_HIP_CAPACITY, "output capacity " + std::to_string(capacity) + " < " + std::to_string(p.total));
        if (p.total) copy_to_host(ws, out_nodes, p.d_nodes, p.total * sizeof(uint32_t));
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_extract_paths(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, const uint64_t *path_ids, uint64_t n,
                                       int reverse, uint64_t *out_offsets, uint32_t *out_nodes, uint64_t capacity,
                                       uint64_t *total) {
    GBWT_HIP_GUARD_BEGIN
    if (n && !path_ids) return fail(GBWT_HIP_BAD_ARGUMENT, "null path_ids");
    std::vector<uint64_t> ids(n);
    for (uint64_t k = 0; k < n; k++) ids[k] = 2 * path_ids[k] + (reverse ? 1 : 0);  // support::encode_path
    return gbwt_hip_extract(ix, ws, ids.data(), n, out_offsets, out_nodes, capacity, total);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_copy_result(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, uint64_t *out_offsets, uint32_t *out_nodes, uint64_t capacity) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !ws || ws->index != ix || !ws->extract.timed) return fail(GBWT_HIP_BAD_ARGUMENT, "no device-resident extraction on this workspace");
    if (!out_offsets && !out_nodes) return fail(GBWT_HIP_BAD_ARGUMENT, "null outputs");
    HIP_CHECK(hipSetDevice(ix->device));
    if (out_offsets) HIP_CHECK(hipMemcpy(out_offsets, ws->extract.offsets.ptr, (ws->extract.last_n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (out_nodes) {
        if (capacity < ws->extract.last_total) return fail(GBWT_HIP_CAPACITY, "output capacity " + std::to_string(capacity) + " < " + std::to_string(ws->extract.last_total));
        if (ws->extract.last_total) copy_to_host(ws, out_nodes, ws->extract.nodes.ptr, ws->extract.last_total * sizeof(uint32_t));
    }
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

static gbwt_hip_status path_sums(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, uint64_t *out_sums, uint64_t n, bool hashed) {
    if (!ix || !ws || ws->index != ix || !ws->extract.timed) return fail(GBWT_HIP_BAD_ARGUMENT, "no device-resident extraction on this workspace");
    if (n != ws->extract.last_n || (n && !out_sums)) return fail(GBWT_HIP_BAD_ARGUMENT, "n does not match the last extraction");
    if (n == 0) return GBWT_HIP_OK;
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        ws->query.out_a.reserve(n * sizeof(uint64_t));
        launch_path_sums(ws->extract.offsets.as<uint64_t>(), ws->extract.nodes.as<uint32_t>(), n, ws->query.out_a.as<uint64_t>(), hashed, ws->stream);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out_sums, ws->query.out_a.ptr, n * sizeof(uint64_t), hipMemcpyDeviceToHost, ws->stream));
        HIP_CHECK(hipStreamSynchronize(ws->stream));
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
}

gbwt_hip_status gbwt_hip_path_sums(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, uint64_t *out_sums, uint64_t n) {
    GBWT_HIP_GUARD_BEGIN
    return path_sums(ix, ws, out_sums, n, false);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_path_hashes(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, uint64_t *out_hashes, uint64_t n) {
    GBWT_HIP_GUARD_BEGIN
    return path_sums(ix, ws, out_hashes, n, true);
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_copy_path(const gbwt_hip_index *ix, gbwt_hip_workspace *ws, uint64_t k, uint32_t *out_nodes,
                                   uint64_t capacity, uint64_t *len) {
    GBWT_HIP_GUARD_BEGIN
    if (!ix || !ws || ws->index != ix || !ws->extract.timed || !len) return fail(GBWT_HIP_BAD_ARGUMENT, "no device-resident extraction on this workspace");
    if (k >= ws->extract.last_n) return fail(GBWT_HIP_BAD_ARGUMENT, "row out of range");
    try {
        HIP_CHECK(hipSetDevice(ix->device));
        uint64_t range[2];
        HIP_CHECK(hipMemcpy(range, ws->extract.offsets.as<uint64_t>() + k, sizeof(range), hipMemcpyDeviceToHost));
        *len = range[1] - range[0];
        uint64_t count = std::min(*len, capacity);
        if (count && out_nodes) HIP_CHECK(hipMemcpy(out_nodes, ws->extract.nodes.as<uint32_t>() + range[0], count * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return GBWT_HIP_OK;
    } catch (const HipError &e) {
        return status_of(e);
    }
    GBWT_HIP_GUARD_END
}

gbwt_hip_status gbwt_hip_last_kernel_ms(const gbwt_hip_workspace *ws, float *walk_ms, float *total_ms) {
    GBWT_HIP_GUARD_BEGIN
    if (!ws || !ws->extract.timed) return fail(GBWT_HIP_BAD_ARGUMENT, "no timed extraction on this workspace");
    float a = 0, b = 0;
    if (hipEventElapsedTime(&a, ws->extract.ev[0], ws->extract.ev[1]) != hipSuccess || hipEventElapsedTime(&b, ws->extract.ev[3], ws->extract.ev[2]) != hipSuccess)
        return fail(GBWT_HIP_DEVICE_ERROR, "hipEventElapsedTime failed");
    if (walk_ms) *walk_ms = a;
    if (total_ms) *total_ms = b;
    return GBWT_HIP_OK;
    GBWT_HIP_GUARD_END
}

}  // extern "C"
