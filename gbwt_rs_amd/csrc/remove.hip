// remove.hip -- path removal on the device: the index of the sequences that stay, without ranking anything.
//
// All positions of all records form one array: record r owns [first[r], first[r + 1]), the endmarker's record comes first.  Taking
// sequences out does not change the order of the visits that stay, so the new bodies are the old ones with the positions of the removed
// sequences left out.  A lane per removed sequence follows it with the plain LF step and marks its positions, one byte each; M is the
// exclusive sum of the marks, a kept position i moves to i - M[i], and the compacted bodies are what build.hip has after its ranking: its
// edge, size and fill phases make the bytes (encode_sorted_bodies).  The visits of w are sorted by predecessor first, so the first P
// positions of w's old record -- P the old stored offset of v -> w -- are the visits whose predecessor is below v, and the new offset is
// what is left of them:  P' = P - (M[first[w] + P] - M[first[w]]).
// Positions are u32 (build.hpp); every kernel indexes with 64 bits and checks what it writes against the size of the array.  No
// atomics: every position belongs to one sequence, so distinct lanes mark distinct bytes, and the same input gives the same bytes.
// A lane that meets what a sound index cannot hold -- a walk that leaves the records or does not end, an edge of the result that the old
// record lacks, an offset beyond the record -- stores 1 in one error word (a plain store: every such lane writes the same value); the host
// reads it behind the marks and behind the offsets and refuses the index (InvalidData) where the result would be plausible wrong bytes.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>

#include "build.hpp"
#include "capi_internal.hpp"
#include "device_common.hpp"
#include "hip_raii.hpp"
#include "lf_device.hpp"
#include "merge.hpp"
#include "remove.hpp"

namespace gbwt_hip {

namespace {

using namespace record_access;

constexpr uint32_t THREADS = 256;

using Scratch = CountedScratch;
using Buf = CountedBuf;

__device__ __forceinline__ uint64_t global_thread() { return static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x; }

// ---- marks -----------------------------------------------------------------------------------------------------------------------------
// One lane per removed sequence: its place in the endmarker's record, then every position on its way.  At most `positions` steps: a
// sequence cannot be longer, and a corrupt index cannot spin.
__global__ __launch_bounds__(THREADS) void k_remove_mark(DeviceIndex ix, const uint32_t *__restrict__ first, const uint64_t *__restrict__ removed, uint64_t n, uint64_t sequences,
                                                        uint64_t positions, uint8_t *__restrict__ mark, uint32_t *__restrict__ error) {
    const uint64_t x = global_thread();
    if (x >= n) return;
    const uint64_t id = removed[x];
    if (id >= sequences || id >= positions) { *error = 1; return; }
    mark[id] = 1;
    if (id >= ix.n_endmarker) return;                        // (a sequence without an entry is empty, as k_merge_decode_starts reads it)
    const uint2 start = ix.endmarker[id];
    uint64_t v = start.x, i = start.y;
    for (uint64_t step = 0; step < positions; step++) {
        if (v == 0) return;
        const uint64_t r = record_of_node(ix, v);
        if (r == NO_RECORD) { *error = 1; return; }
        const uint64_t at = static_cast<uint64_t>(first[r]) + i;
        if (at >= first[r + 1] || at >= positions) { *error = 1; return; }
        mark[at] = 1;
        uint64_t w, j;
        if (!gbwt_forward(ix, v, i, w, j)) return;           // the successor is the endmarker: the sequence ends
        v = w; i = j;
    }
    *error = 1;                                              // more steps than the index has positions
}

// ---- compaction ----------------------------------------------------------------------------------------------------------------------------
// A kept position i moves to i - M[i], with the node of its record and its successor.  Every slot of rec and succ is written exactly once:
// the arrays need no memset.
__global__ __launch_bounds__(THREADS) void k_remove_compact(DeviceIndex ix, const uint32_t *__restrict__ first, const uint32_t *__restrict__ body, const uint8_t *__restrict__ mark,
                                                           const uint32_t *__restrict__ M, uint64_t positions, uint64_t kept, uint32_t *__restrict__ rec, uint32_t *__restrict__ succ) {
    const uint64_t i = global_thread();
    if (i >= positions || mark[i]) return;
    const uint64_t out = i - M[i];                           // one to one on the kept positions, and kept = positions - M[positions] of them
    if (out >= kept) return;                                 // (cannot happen: M counts the marks in front of i)
    const uint64_t r = merge_upper_bound(first, ix.n_records + 1, i) - 1;   // the last record that starts at or before i: the one that is not empty
    rec[out] = static_cast<uint32_t>(node_of_record(ix, r));
    succ[out] = body[i];
}

// ---- edge offsets ------------------------------------------------------------------------------------------------------------------------
// One lane per edge v -> w of the result: the old offset, less the removed visits among the first P of w's old record
__global__ __launch_bounds__(THREADS) void k_remove_edge_offsets(DeviceIndex ix, const uint32_t *__restrict__ first, const uint32_t *__restrict__ M, uint64_t positions,
                                                                const uint64_t *__restrict__ edge, uint64_t edges, uint32_t *__restrict__ edge_offset, uint32_t *__restrict__ error) {
    const uint64_t e = global_thread();
    if (e >= edges) return;
    const uint64_t v = edge[e] >> 32, w = edge[e] & 0xFFFFFFFFull;
    if (v == 0 || w == 0) return;                            // (the 0 of the memset)
    uint64_t P;
    if (!edge_offset_of(ix, v, w, P)) { *error = 1; return; }      // a kept visit took the edge: the old record of v has it
    const uint64_t rw = record_of_node(ix, w);
    if (rw == NO_RECORD) { *error = 1; return; }
    const uint64_t base = first[rw], upto = base + P;
    if (upto > first[rw + 1] || upto > positions) { *error = 1; return; }   // (M has positions + 1 entries)
    edge_offset[e] = static_cast<uint32_t>(P - (M[upto] - M[base]));
}

struct Widen {
    __host__ __device__ __forceinline__ uint32_t operator()(uint8_t x) const { return x; }
};

}  // namespace

void remove_records_on_device(const MergeInput &in, const uint64_t *removed, uint64_t n, BuildOutput &out, RemoveWalk &walk, hipStream_t s) {
    const uint64_t positions = in.sequences + in.visits;
    Scratch sc;
    EventSet<4> ev;
    Buf temp;
    HIP_CHECK(hipEventRecord(ev.e[0], s));

    // 1. lengths and bodies (merge.hip)
    MergeDecoded d;
    merge_decode_bodies(in, d, sc, temp, s);
    HIP_CHECK(hipEventRecord(ev.e[1], s));
    const uint32_t *first = d.first.as<uint32_t>();

    // 2. marks, with one entry past the last position for the scan
    Buf mark(sc, positions + 1), M(sc, (positions + 1) * sizeof(uint32_t)), error(sc, sizeof(uint32_t));
    HIP_CHECK(hipMemsetAsync(mark.ptr, 0, mark.bytes, s));
    HIP_CHECK(hipMemsetAsync(error.ptr, 0, sizeof(uint32_t), s));
    const auto check_error = [&](const char *where) {         // (behind a synchronize of s)
        uint32_t flag = 0;
        HIP_CHECK(hipMemcpyAsync(&flag, error.ptr, sizeof(flag), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (flag) throw InvalidData(std::string("remove: the records of the index are not consistent (") + where + ")");
    };
    if (n) {
        Buf ids(sc, n * sizeof(uint64_t));
        HIP_CHECK(hipMemcpyAsync(ids.ptr, removed, n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        k_remove_mark<<<blocks_for(n), THREADS, 0, s>>>(in.ix, first, ids.as<uint64_t>(), n, in.sequences, positions, mark.as<uint8_t>(), error.as<uint32_t>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));                 // (ids goes out of scope)
    }
    HIP_CHECK(hipEventRecord(ev.e[2], s));

    // 3. M, the sizes of the result, the compacted bodies and their alphabet
    {
        hipcub::TransformInputIterator<uint32_t, Widen, const uint8_t *> marks(mark.as<uint8_t>(), Widen());
        size_t bytes = 0;
        HIP_CHECK(hipcub::DeviceScan::ExclusiveScan(nullptr, bytes, marks, M.as<uint32_t>(), hipcub::Sum(), uint32_t(0), positions + 1, s));
        if (bytes > temp.bytes) temp.alloc(sc, bytes);
        HIP_CHECK(hipcub::DeviceScan::ExclusiveScan(temp.ptr, bytes, marks, M.as<uint32_t>(), hipcub::Sum(), uint32_t(0), positions + 1, s));
    }
    uint32_t marked = 0;
    HIP_CHECK(hipMemcpyAsync(&marked, M.as<uint32_t>() + positions, sizeof(marked), hipMemcpyDeviceToHost, s));
    check_error("a removed sequence leaves the records or does not end");
    if (marked < n || marked > positions || n > in.sequences)
        throw InvalidData("remove: " + std::to_string(n) + " sequences marked " + std::to_string(marked) + " of " + std::to_string(positions) + " positions");
    walk.removed_sequences = n; walk.removed_steps = marked - n;
    const uint64_t sequences = in.sequences - n, visits = in.visits - walk.removed_steps, kept = sequences + visits;
    if (visits == 0) {
        build_without_visits(sequences, out);
        HIP_CHECK(hipEventRecord(ev.e[3], s));
        HIP_CHECK(hipStreamSynchronize(s));
    } else {
        Buf rec(sc, kept * sizeof(uint32_t)), succ(sc, kept * sizeof(uint32_t));
        k_remove_compact<<<blocks_for(positions), THREADS, 0, s>>>(in.ix, first, d.body.as<uint32_t>(), mark.as<uint8_t>(), M.as<uint32_t>(), positions, kept, rec.as<uint32_t>(),
                                                                   succ.as<uint32_t>());
        HIP_CHECK(hipGetLastError());
        uint32_t lo = 0, hi = 0;
        build_node_range(rec.as<uint32_t>() + sequences, visits, lo, hi, s);     // (synchronizes)
        d.body.release(); mark.release();
        if (lo < 2 || hi < lo) throw InvalidData("remove: the kept visits lie in the records of nodes " + std::to_string(lo) + " .. " + std::to_string(hi));
        out.sequences = sequences; out.visits = visits;
        out.alphabet_offset = lo - 1; out.alphabet_size = static_cast<uint64_t>(hi) + 1; out.records = out.alphabet_size - out.alphabet_offset;
        HIP_CHECK(hipEventRecord(ev.e[3], s));

        // 4. edges, offsets, bytes: the construction's
        BodyOffsets offsets;
        offsets.launch = [&](const BodyEdges &e) {
            if (e.edges) k_remove_edge_offsets<<<blocks_for(e.edges), THREADS, 0, s>>>(in.ix, first, M.as<uint32_t>(), positions, e.edge, e.edges, e.edge_offset, error.as<uint32_t>());
        };
        offsets.release = [&] {                              // (encode_sorted_bodies has synchronized behind the launch)
            M.release(); d.first.release();
            check_error("a kept edge is not in the old record, or its offset lies beyond the record");
        };
        encode_sorted_bodies(rec, succ, kept, out.records, out.alphabet_offset, offsets, sc, temp, out, ev.e[3], s);
    }
    HIP_CHECK(hipEventElapsedTime(&walk.decode_ms, ev.e[0], ev.e[1]));
    HIP_CHECK(hipEventElapsedTime(&walk.walk_ms, ev.e[1], ev.e[2]));
    HIP_CHECK(hipEventElapsedTime(&walk.compact_ms, ev.e[2], ev.e[3]));
    out.peak_scratch = sc.peak;
}

}  // namespace gbwt_hip
