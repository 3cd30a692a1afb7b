// build.hip -- GBWT construction on the device: from a set of paths in HBM to the record stream of their index.
//
// The TEXT is one slot per visit and one per sequence: sequence s owns the slots [first(s), first(s) + 1 + len(s)), the first of them its
// START (the virtual position -1), the others its visits in path order.  A record lists the visits of its node ordered by REVERSE PREFIX --
// the nodes before the visit read backwards, the start of a sequence below every node, two starts by sequence id -- so the slots are
// ranked by (own symbol, symbol before, ...) with prefix doubling: a start's symbol is its sequence id, a visit's its node above all
// of those, and every string ends in a start, so all ranks become distinct.  The sorted slots ARE the bodies of the records one after
// the other: the starts (record 0, the endmarker's: the successor of a start is the first node of its sequence), then the visits node by
// node.  From there: successors and run heads (gather), the distinct (record, successor) pairs of the run heads (edge lists), the first
// visit of every (predecessor, node) block (edge offsets), then byte sizes, three scans and a fill pass with one lane per item.
// Slots, ranks and offsets are u32 (build.hpp); every kernel indexes with 64 bits.  No atomics, stable sorts: the same input gives the
// same bytes.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "build.hpp"
#include "build_codec.hpp"
#include "capi_internal.hpp"
#include "device_common.hpp"
#include "hip_raii.hpp"

namespace gbwt_hip {

namespace {

constexpr uint32_t THREADS = 256;

__device__ __forceinline__ uint64_t global_thread() { return static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x; }

using Scratch = CountedScratch;
using Buf = CountedBuf;

// ---- 1. expand ---------------------------------------------------------------------------------------------------------------------
// Slot t: the path that owns it by bisection over first(p) = (off[p] + p) << bidir (a path owns one start and its visits, twice with
// its reverse), then node[t] (0 for a start), first_slot[t] = the start of its sequence, and the key of the first sort: the sequence id
// for a start, 2^32 + node for a visit.
__global__ __launch_bounds__(THREADS) void k_build_expand(const uint64_t *__restrict__ off, const uint32_t *__restrict__ nodes, uint64_t n_paths, uint32_t bidir, uint64_t slots,
                                                          uint32_t *__restrict__ node, uint32_t *__restrict__ first_slot, uint64_t *__restrict__ key, uint32_t *__restrict__ val) {
    const uint64_t t = global_thread();
    if (t >= slots) return;
    uint64_t lo = 0, hi = n_paths;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (((off[mid] + mid) << bidir) <= t) lo = mid; else hi = mid;
    }
    const uint64_t p = lo, begin = off[p], len = off[p + 1] - begin, local = t - ((begin + p) << bidir);
    const bool reverse = bidir != 0 && local > len;
    const uint64_t seq = bidir ? 2 * p + (reverse ? 1 : 0) : p, start = t - local + (reverse ? len + 1 : 0), j = t - start;
    uint32_t v = 0;
    if (j > 0) v = reverse ? (nodes[begin + len - j] ^ 1u) : nodes[begin + j - 1];
    node[t] = v;
    first_slot[t] = static_cast<uint32_t>(start);
    key[t] = j == 0 ? seq : ((uint64_t(1) << 32) | v);
    val[t] = static_cast<uint32_t>(t);
}

// ---- 2. ranking ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_build_rank_flags(const uint64_t *__restrict__ key, uint64_t n, uint32_t *__restrict__ flag) {
    const uint64_t i = global_thread();
    if (i >= n) return;
    flag[i] = (i > 0 && key[i] != key[i - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(THREADS) void k_build_rank_scatter(const uint32_t *__restrict__ val, const uint32_t *__restrict__ dense, uint64_t n, uint32_t *__restrict__ rank) {
    const uint64_t i = global_thread();
    if (i >= n) return;
    rank[val[i]] = dense[i];
}

// the keys of a doubling round over `h` symbols: (rank of the slot, rank of the slot h before it); a slot whose string ends within h
// symbols holds a distinct rank already, its second half is 0
__global__ __launch_bounds__(THREADS) void k_build_round_keys(const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ first_slot,
                                                              uint64_t n, uint64_t h, uint32_t bits, uint64_t *__restrict__ key, uint32_t *__restrict__ val) {
    const uint64_t i = global_thread();
    if (i >= n) return;
    const uint32_t t = sorted[i];
    const uint64_t before = (static_cast<uint64_t>(t) - first_slot[t] >= h) ? rank[t - h] : 0;
    key[i] = (static_cast<uint64_t>(rank[t]) << bits) | before;
    val[i] = t;
}

// ---- 3. successors and runs ---------------------------------------------------------------------------------------------------------------
// Position i of the sorted slots: its record's node (0: the endmarker's), its successor (0 at the end of the sequence), its predecessor
// (0: none -- a start, or the first visit of a sequence) and whether a run starts here.
__global__ __launch_bounds__(THREADS) void k_build_gather(const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ node, const uint32_t *__restrict__ first_slot, uint64_t n,
                                                          uint32_t *__restrict__ rec, uint32_t *__restrict__ succ, uint32_t *__restrict__ pred) {
    const uint64_t i = global_thread();
    if (i >= n) return;
    const uint64_t t = sorted[i];
    const uint32_t first = first_slot[t];
    rec[i] = node[t];
    succ[i] = (t + 1 < n && first_slot[t + 1] == first) ? node[t + 1] : 0u;
    pred[i] = (t >= static_cast<uint64_t>(first) + 2) ? node[t - 1] : 0u;
}

__global__ __launch_bounds__(THREADS) void k_build_run_flags(const uint32_t *__restrict__ rec, const uint32_t *__restrict__ succ, uint64_t n, uint8_t *__restrict__ flag) {
    const uint64_t i = global_thread();
    if (i >= n) return;
    flag[i] = (i == 0 || rec[i] != rec[i - 1] || succ[i] != succ[i - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(THREADS) void k_build_run_keys(const uint32_t *__restrict__ head, uint64_t runs, const uint32_t *__restrict__ rec, const uint32_t *__restrict__ succ,
                                                            uint64_t *__restrict__ key) {
    const uint64_t j = global_thread();
    if (j >= runs) return;
    const uint32_t i = head[j];
    key[j] = (static_cast<uint64_t>(rec[i]) << 32) | succ[i];
}

// ---- 4. / 5. edge lists and offsets -------------------------------------------------------------------------------------------------------
// Record r (r == records: the end): its first edge, its first run and its first position in the sorted slots
__global__ __launch_bounds__(THREADS) void k_build_record_bounds(const uint64_t *__restrict__ edge, uint64_t edges, const uint64_t *__restrict__ run_key, uint64_t runs,
                                                                 const uint32_t *__restrict__ rec, uint64_t slots, uint64_t records, uint64_t alphabet_offset,
                                                                 uint32_t *__restrict__ edge_first, uint32_t *__restrict__ run_first, uint32_t *__restrict__ visit_first) {
    const uint64_t r = global_thread();
    if (r > records) return;
    if (r == records) {
        edge_first[r] = static_cast<uint32_t>(edges); run_first[r] = static_cast<uint32_t>(runs); visit_first[r] = static_cast<uint32_t>(slots);
        return;
    }
    const uint64_t v = r == 0 ? 0 : r + alphabet_offset;       // < 2^32
    edge_first[r] = static_cast<uint32_t>(lower_bound<uint64_t>(edge, 0, edges, v << 32));
    run_first[r] = static_cast<uint32_t>(lower_bound<uint64_t>(run_key, 0, runs, v << 32));   // (the runs are in record order; inside a record no key is below v << 32)
    visit_first[r] = static_cast<uint32_t>(lower_bound<uint32_t>(rec, 0, slots, static_cast<uint32_t>(v)));
}

// The visits of node w that came from v are one block of w's record; the offset of edge v -> w is where the block starts.  Lanes at the
// head of a block look the edge up in v's list.  Edges to the endmarker and the edges of the endmarker keep the 0 of the memset.
__global__ __launch_bounds__(THREADS) void k_build_edge_offsets(const uint32_t *__restrict__ rec, const uint32_t *__restrict__ pred, uint64_t sequences, uint64_t slots,
                                                                const uint64_t *__restrict__ edge, const uint32_t *__restrict__ edge_first, const uint32_t *__restrict__ visit_first,
                                                                uint64_t alphabet_offset, uint32_t *__restrict__ edge_offset) {
    const uint64_t i = sequences + global_thread();
    if (i >= slots) return;
    const uint32_t w = rec[i], v = pred[i];
    if (v == 0) return;
    if (i > sequences && rec[i - 1] == w && pred[i - 1] == v) return;
    const uint64_t rv = v - alphabet_offset, lo = edge_first[rv], hi = edge_first[rv + 1];
    const uint64_t e = lo + lower_bound<uint64_t>(edge + lo, 0, hi - lo, (static_cast<uint64_t>(v) << 32) | w);
    if (e < hi) edge_offset[e] = static_cast<uint32_t>(i - visit_first[w - alphabet_offset]);
}

// ---- 6. sizes and bytes ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t record_of(uint64_t key, uint64_t alphabet_offset) {
    const uint64_t v = key >> 32;
    return v == 0 ? 0 : v - alphabet_offset;
}

// sizes[e] for the edges, 0 at e == edges (the scan's last entry is then the total)
__global__ __launch_bounds__(THREADS) void k_build_edge_sizes(const uint64_t *__restrict__ edge, uint64_t edges, const uint32_t *__restrict__ edge_first,
                                                              const uint32_t *__restrict__ edge_offset, uint64_t alphabet_offset, uint64_t *__restrict__ sizes) {
    const uint64_t e = global_thread();
    if (e > edges) return;
    if (e == edges) { sizes[e] = 0; return; }
    const uint64_t key = edge[e], r = record_of(key, alphabet_offset);
    const uint64_t prev = e > edge_first[r] ? (edge[e - 1] & 0xFFFFFFFFull) : 0;
    sizes[e] = build_codec::edge_size((key & 0xFFFFFFFFull) - prev, edge_offset[e]);
}

// the edge rank of every run and its size (0 at j == runs)
__global__ __launch_bounds__(THREADS) void k_build_run_sizes(const uint64_t *__restrict__ run_key, const uint32_t *__restrict__ head, uint64_t runs, uint64_t slots,
                                                             const uint64_t *__restrict__ edge, const uint32_t *__restrict__ edge_first, uint64_t alphabet_offset,
                                                             uint32_t *__restrict__ run_rank, uint64_t *__restrict__ sizes) {
    const uint64_t j = global_thread();
    if (j > runs) return;
    if (j == runs) { sizes[j] = 0; return; }
    const uint64_t key = run_key[j], r = record_of(key, alphabet_offset), lo = edge_first[r], sigma = edge_first[r + 1] - lo;
    const uint64_t rank = lower_bound<uint64_t>(edge + lo, 0, sigma, key);
    const uint64_t len = (j + 1 < runs ? static_cast<uint64_t>(head[j + 1]) : slots) - head[j];
    run_rank[j] = static_cast<uint32_t>(rank);
    sizes[j] = build_codec::run_size(sigma, rank, len);
}

__global__ __launch_bounds__(THREADS) void k_build_header_sizes(const uint32_t *__restrict__ edge_first, uint64_t records, uint64_t *__restrict__ sizes) {
    const uint64_t r = global_thread();
    if (r > records) return;
    sizes[r] = r == records ? 0 : build_codec::header_size(edge_first[r + 1] - edge_first[r]);
}

// The stream is record by record: head, edges, runs.  So with H, EC, RC the exclusive scans of the three kinds of sizes, record r starts at
// H[r] + EC[its first edge] + RC[its first run], its edge e at H[r + 1] + EC[e] + RC[its first run], its run j at H[r + 1] + EC[the end of
// its edges] + RC[j].
__global__ __launch_bounds__(THREADS) void k_build_starts(const uint64_t *__restrict__ hdr_at, const uint64_t *__restrict__ edge_at, const uint64_t *__restrict__ run_at,
                                                          const uint32_t *__restrict__ edge_first, const uint32_t *__restrict__ run_first, uint64_t records,
                                                          uint64_t *__restrict__ starts) {
    const uint64_t r = global_thread();
    if (r > records) return;
    starts[r] = hdr_at[r] + edge_at[edge_first[r]] + run_at[run_first[r]];
}

__global__ __launch_bounds__(THREADS) void k_build_fill_headers(const uint64_t *__restrict__ starts, const uint32_t *__restrict__ edge_first, uint64_t records, uint8_t *__restrict__ data) {
    const uint64_t r = global_thread();
    if (r >= records) return;
    build_codec::write_header(data + starts[r], edge_first[r + 1] - edge_first[r]);
}

__global__ __launch_bounds__(THREADS) void k_build_fill_edges(const uint64_t *__restrict__ edge, uint64_t edges, const uint32_t *__restrict__ edge_first, const uint32_t *__restrict__ run_first,
                                                              const uint32_t *__restrict__ edge_offset, const uint64_t *__restrict__ hdr_at, const uint64_t *__restrict__ edge_at,
                                                              const uint64_t *__restrict__ run_at, uint64_t alphabet_offset, uint8_t *__restrict__ data) {
    const uint64_t e = global_thread();
    if (e >= edges) return;
    const uint64_t key = edge[e], r = record_of(key, alphabet_offset);
    const uint64_t prev = e > edge_first[r] ? (edge[e - 1] & 0xFFFFFFFFull) : 0;
    build_codec::write_edge(data + hdr_at[r + 1] + edge_at[e] + run_at[run_first[r]], (key & 0xFFFFFFFFull) - prev, edge_offset[e]);
}

__global__ __launch_bounds__(THREADS) void k_build_fill_runs(const uint64_t *__restrict__ run_key, const uint32_t *__restrict__ head, const uint32_t *__restrict__ run_rank, uint64_t runs,
                                                             uint64_t slots, const uint32_t *__restrict__ edge_first, const uint64_t *__restrict__ hdr_at,
                                                             const uint64_t *__restrict__ edge_at, const uint64_t *__restrict__ run_at, uint64_t alphabet_offset,
                                                             uint8_t *__restrict__ data) {
    const uint64_t j = global_thread();
    if (j >= runs) return;
    const uint64_t r = record_of(run_key[j], alphabet_offset), hi = edge_first[r + 1], sigma = hi - edge_first[r];
    const uint64_t len = (j + 1 < runs ? static_cast<uint64_t>(head[j + 1]) : slots) - head[j];
    build_codec::write_run(data + hdr_at[r + 1] + edge_at[hi] + run_at[j], sigma, run_rank[j], len);
}

}  // namespace

void build_node_range(const uint32_t *d_nodes, uint64_t n, uint32_t &min_node, uint32_t &max_node, hipStream_t s) {
    Scratch sc;
    Buf out(sc, 2 * sizeof(uint32_t)), temp;
    size_t a = 0, b = 0;
    HIP_CHECK(hipcub::DeviceReduce::Min(nullptr, a, d_nodes, out.as<uint32_t>(), n, s));
    HIP_CHECK(hipcub::DeviceReduce::Max(nullptr, b, d_nodes, out.as<uint32_t>() + 1, n, s));
    temp.alloc(sc, std::max(a, b));
    HIP_CHECK(hipcub::DeviceReduce::Min(temp.ptr, a, d_nodes, out.as<uint32_t>(), n, s));
    HIP_CHECK(hipcub::DeviceReduce::Max(temp.ptr, b, d_nodes, out.as<uint32_t>() + 1, n, s));
    uint32_t both[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(both, out.ptr, sizeof(both), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    min_node = both[0]; max_node = both[1];
}

// From the sorted slots as record bodies -- rec[i] the node of position i's record (0: the endmarker's), succ[i] its successor -- to the
// record stream on the host: run heads, edge lists, offsets (the caller's: BodyOffsets), sizes, scans, bytes.  The construction and the
// merge (merge.hip) both enter here.  rec and succ are given back on the way, temp (any size) is the scratch of the library calls; `begin` is an event the caller has recorded on s.
void encode_sorted_bodies(CountedBuf &rec, CountedBuf &succ, uint64_t slots, uint64_t records, uint64_t alphabet_offset, const BodyOffsets &offsets, CountedScratch &sc, CountedBuf &temp,
                          BuildOutput &out, hipEvent_t begin, hipStream_t s) {
    EventSet<5> ev;
    Buf head(sc, slots * sizeof(uint32_t)), count(sc, sizeof(uint64_t));
    uint64_t runs = 0;
    {
        Buf flag(sc, slots);
        k_build_run_flags<<<blocks_for(slots), THREADS, 0, s>>>(rec.as<uint32_t>(), succ.as<uint32_t>(), slots, flag.as<uint8_t>());
        hipcub::CountingInputIterator<uint32_t> positions(0);
        size_t bytes = 0;
        HIP_CHECK(hipcub::DeviceSelect::Flagged(nullptr, bytes, positions, flag.as<uint8_t>(), head.as<uint32_t>(), count.as<uint64_t>(), static_cast<int64_t>(slots), s));
        if (bytes > temp.bytes) temp.alloc(sc, bytes);
        HIP_CHECK(hipcub::DeviceSelect::Flagged(temp.ptr, bytes, positions, flag.as<uint8_t>(), head.as<uint32_t>(), count.as<uint64_t>(), static_cast<int64_t>(slots), s));
        HIP_CHECK(hipGetLastError());
        runs = read_value(count.as<uint64_t>(), s);
    }

    // 4. the edge lists: the distinct (record, successor) pairs of the run heads, sorted
    Buf run_key(sc, runs * sizeof(uint64_t)), edge(sc, runs * sizeof(uint64_t));
    uint64_t edges = 0;
    {
        Buf key_sorted(sc, runs * sizeof(uint64_t));
        k_build_run_keys<<<blocks_for(runs), THREADS, 0, s>>>(head.as<uint32_t>(), runs, rec.as<uint32_t>(), succ.as<uint32_t>(), run_key.as<uint64_t>());
        size_t sort_bytes = 0, unique_bytes = 0;
        HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, run_key.as<uint64_t>(), key_sorted.as<uint64_t>(), runs, 0, 64, s));
        HIP_CHECK(hipcub::DeviceSelect::Unique(nullptr, unique_bytes, key_sorted.as<uint64_t>(), edge.as<uint64_t>(), count.as<uint64_t>(), static_cast<int64_t>(runs), s));
        if (std::max(sort_bytes, unique_bytes) > temp.bytes) temp.alloc(sc, std::max(sort_bytes, unique_bytes));
        HIP_CHECK(hipcub::DeviceRadixSort::SortKeys(temp.ptr, sort_bytes, run_key.as<uint64_t>(), key_sorted.as<uint64_t>(), runs, 0, 64, s));
        HIP_CHECK(hipcub::DeviceSelect::Unique(temp.ptr, unique_bytes, key_sorted.as<uint64_t>(), edge.as<uint64_t>(), count.as<uint64_t>(), static_cast<int64_t>(runs), s));
        HIP_CHECK(hipGetLastError());
        edges = read_value(count.as<uint64_t>(), s);
    }
    succ.release();
    Buf edge_first(sc, (records + 1) * sizeof(uint32_t)), run_first(sc, (records + 1) * sizeof(uint32_t)), visit_first(sc, (records + 1) * sizeof(uint32_t));
    k_build_record_bounds<<<blocks_for(records + 1), THREADS, 0, s>>>(edge.as<uint64_t>(), edges, run_key.as<uint64_t>(), runs, rec.as<uint32_t>(), slots, records, alphabet_offset,
                                                                      edge_first.as<uint32_t>(), run_first.as<uint32_t>(), visit_first.as<uint32_t>());

    // 5. the edge offsets
    Buf edge_offset(sc, edges * sizeof(uint32_t));
    HIP_CHECK(hipMemsetAsync(edge_offset.ptr, 0, edge_offset.bytes, s));
    offsets.launch(BodyEdges{edge.as<uint64_t>(), edges, edge_first.as<uint32_t>(), visit_first.as<uint32_t>(), edge_offset.as<uint32_t>()});
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[0], s));
    HIP_CHECK(hipStreamSynchronize(s));
    rec.release(); visit_first.release();
    if (offsets.release) offsets.release();

    // 6. sizes, scans, starts, bytes
    Buf run_rank(sc, runs * sizeof(uint32_t)), sizes(sc, (std::max({edges, runs, records}) + 1) * sizeof(uint64_t));
    Buf edge_at(sc, (edges + 1) * sizeof(uint64_t)), run_at(sc, (runs + 1) * sizeof(uint64_t)), hdr_at(sc, (records + 1) * sizeof(uint64_t));
    Buf starts(sc, (records + 1) * sizeof(uint64_t));
    k_build_edge_sizes<<<blocks_for(edges + 1), THREADS, 0, s>>>(edge.as<uint64_t>(), edges, edge_first.as<uint32_t>(), edge_offset.as<uint32_t>(), alphabet_offset, sizes.as<uint64_t>());
    exclusive_sum(sizes.as<uint64_t>(), edge_at.as<uint64_t>(), edges + 1, sc, temp, s);
    k_build_run_sizes<<<blocks_for(runs + 1), THREADS, 0, s>>>(run_key.as<uint64_t>(), head.as<uint32_t>(), runs, slots, edge.as<uint64_t>(), edge_first.as<uint32_t>(), alphabet_offset,
                                                               run_rank.as<uint32_t>(), sizes.as<uint64_t>());
    exclusive_sum(sizes.as<uint64_t>(), run_at.as<uint64_t>(), runs + 1, sc, temp, s);
    k_build_header_sizes<<<blocks_for(records + 1), THREADS, 0, s>>>(edge_first.as<uint32_t>(), records, sizes.as<uint64_t>());
    exclusive_sum(sizes.as<uint64_t>(), hdr_at.as<uint64_t>(), records + 1, sc, temp, s);
    k_build_starts<<<blocks_for(records + 1), THREADS, 0, s>>>(hdr_at.as<uint64_t>(), edge_at.as<uint64_t>(), run_at.as<uint64_t>(), edge_first.as<uint32_t>(), run_first.as<uint32_t>(),
                                                               records, starts.as<uint64_t>());
    HIP_CHECK(hipGetLastError());
    const uint64_t data_bytes = read_value(starts.as<uint64_t>() + records, s);
    Buf data(sc, data_bytes);
    k_build_fill_headers<<<blocks_for(records), THREADS, 0, s>>>(starts.as<uint64_t>(), edge_first.as<uint32_t>(), records, data.as<uint8_t>());
    k_build_fill_edges<<<blocks_for(edges), THREADS, 0, s>>>(edge.as<uint64_t>(), edges, edge_first.as<uint32_t>(), run_first.as<uint32_t>(), edge_offset.as<uint32_t>(),
                                                             hdr_at.as<uint64_t>(), edge_at.as<uint64_t>(), run_at.as<uint64_t>(), alphabet_offset, data.as<uint8_t>());
    k_build_fill_runs<<<blocks_for(runs), THREADS, 0, s>>>(run_key.as<uint64_t>(), head.as<uint32_t>(), run_rank.as<uint32_t>(), runs, slots, edge_first.as<uint32_t>(),
                                                           hdr_at.as<uint64_t>(), edge_at.as<uint64_t>(), run_at.as<uint64_t>(), alphabet_offset, data.as<uint8_t>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[1], s));

    // 7. to the host
    out.data.resize(data_bytes);
    out.starts.resize(records);
    HIP_CHECK(hipMemcpyAsync(out.data.data(), data.ptr, data_bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(out.starts.data(), starts.ptr, records * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventElapsedTime(&out.edges_ms, begin, ev.e[0]));
    HIP_CHECK(hipEventElapsedTime(&out.encode_ms, ev.e[0], ev.e[1]));
}

void build_records_on_device(const BuildInput &in, BuildOutput &out, hipStream_t s) {
    const uint64_t sequences = in.bidirectional ? 2 * in.n_paths : in.n_paths;
    const uint64_t visits = in.bidirectional ? 2 * in.path_visits : in.path_visits;
    const uint64_t slots = visits + sequences;
    const uint64_t alphabet_offset = in.min_node - 1, alphabet_size = in.max_node + 1, records = alphabet_size - alphabet_offset;
    out.sequences = sequences; out.visits = visits; out.records = records; out.alphabet_offset = alphabet_offset; out.alphabet_size = alphabet_size;
    Scratch sc;
    EventSet<5> ev;
    Buf temp;
    HIP_CHECK(hipEventRecord(ev.e[0], s));

    // 1. the text
    Buf node(sc, slots * sizeof(uint32_t)), first_slot(sc, slots * sizeof(uint32_t)), sorted(sc, slots * sizeof(uint32_t));
    {
        Buf key_a(sc, slots * sizeof(uint64_t)), key_b(sc, slots * sizeof(uint64_t)), val_a(sc, slots * sizeof(uint32_t)), rank(sc, slots * sizeof(uint32_t)),
            dense(sc, slots * sizeof(uint32_t));         // (rank holds the flags of a round until the new ranks are scattered into it)
        k_build_expand<<<blocks_for(slots), THREADS, 0, s>>>(in.d_offsets, in.d_nodes, in.n_paths, in.bidirectional ? 1u : 0u, slots, node.as<uint32_t>(), first_slot.as<uint32_t>(),
                                                             key_a.as<uint64_t>(), val_a.as<uint32_t>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ev.e[1], s));

        // 2. ranks by reverse prefix: the first sort by the symbol of the slot, then doubling rounds until every rank is its own
        const int bits = bits_for(slots, 63);
        size_t sort_bytes = 0, scan_bytes = 0;
        for (int end_bit : {33, 2 * bits}) {             // (the two sorts below)
            size_t need = 0;
            HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, key_a.as<uint64_t>(), key_b.as<uint64_t>(), val_a.as<uint32_t>(), sorted.as<uint32_t>(), slots, 0, end_bit, s));
            sort_bytes = std::max(sort_bytes, need);
        }
        HIP_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, rank.as<uint32_t>(), dense.as<uint32_t>(), slots, s));
        temp.alloc(sc, std::max(sort_bytes, scan_bytes));
        uint32_t rounds = 0;
        for (uint64_t h = 0;; h = h ? 2 * h : 1) {       // h: symbols the ranks in hand have compared (0: none yet)
            const int end_bit = h == 0 ? 33 : 2 * bits;
            if (h != 0) {
                k_build_round_keys<<<blocks_for(slots), THREADS, 0, s>>>(sorted.as<uint32_t>(), rank.as<uint32_t>(), first_slot.as<uint32_t>(), slots, h, static_cast<uint32_t>(bits),
                                                                         key_a.as<uint64_t>(), val_a.as<uint32_t>());
                rounds++;
            }
            HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp.ptr, sort_bytes, key_a.as<uint64_t>(), key_b.as<uint64_t>(), val_a.as<uint32_t>(), sorted.as<uint32_t>(), slots, 0, end_bit, s));
            k_build_rank_flags<<<blocks_for(slots), THREADS, 0, s>>>(key_b.as<uint64_t>(), slots, rank.as<uint32_t>());
            HIP_CHECK(hipcub::DeviceScan::InclusiveSum(temp.ptr, scan_bytes, rank.as<uint32_t>(), dense.as<uint32_t>(), slots, s));
            HIP_CHECK(hipGetLastError());
            if (read_value(dense.as<uint32_t>() + (slots - 1), s) == slots - 1) break;     // all distinct
            if (h > slots) throw HipError{hipErrorUnknown, "GBWT construction: the ranks of the reverse prefixes did not become distinct"};
            k_build_rank_scatter<<<blocks_for(slots), THREADS, 0, s>>>(sorted.as<uint32_t>(), dense.as<uint32_t>(), slots, rank.as<uint32_t>());
        }
        out.rounds = rounds;
        HIP_CHECK(hipEventRecord(ev.e[2], s));
        HIP_CHECK(hipStreamSynchronize(s));              // the sorts are done with the buffers that go out of scope here
    }

    // 3. successors, predecessors, runs
    Buf rec(sc, slots * sizeof(uint32_t)), succ(sc, slots * sizeof(uint32_t)), pred(sc, slots * sizeof(uint32_t));
    k_build_gather<<<blocks_for(slots), THREADS, 0, s>>>(sorted.as<uint32_t>(), node.as<uint32_t>(), first_slot.as<uint32_t>(), slots, rec.as<uint32_t>(), succ.as<uint32_t>(),
                                                         pred.as<uint32_t>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    node.release(); first_slot.release(); sorted.release();

    // 4. - 7. from the sorted bodies to the bytes; the offset of edge v -> w is where the block of v starts in w's record
    BodyOffsets offsets;
    offsets.launch = [&](const BodyEdges &e) {
        if (visits) k_build_edge_offsets<<<blocks_for(visits), THREADS, 0, s>>>(rec.as<uint32_t>(), pred.as<uint32_t>(), sequences, slots, e.edge, e.edge_first, e.visit_first, alphabet_offset,
                                                                                e.edge_offset);
    };
    offsets.release = [&] { pred.release(); };
    encode_sorted_bodies(rec, succ, slots, records, alphabet_offset, offsets, sc, temp, out, ev.e[2], s);
    HIP_CHECK(hipEventElapsedTime(&out.expand_ms, ev.e[0], ev.e[1]));
    HIP_CHECK(hipEventElapsedTime(&out.rank_ms, ev.e[1], ev.e[2]));
    out.peak_scratch = sc.peak;
}

}  // namespace gbwt_hip
