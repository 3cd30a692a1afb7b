// merge.hip -- GBWT merging on the device: the index of the sequences of a, then those of b, without ranking anything.
//
// Both inputs are sorted by reverse prefix already.  What is missing is, for every visit of one input, how many visits of the OTHER input
// lie below it in the merged record: its CROSS RANK.  The input with fewer visits (W) is walked, one lane per sequence: the lane follows
// its sequence in W with the plain LF step and, in the same loop, in the other input (R) with the successor forced -- from node v with
// cross rank c to the next node w,  c' = P_R(w, v) + (occurrences of w among the first c entries of R's body of v),  where P_X(w, v) is
// the number of visits of w in X whose predecessor is below v.  P comes from the stored edge offsets: of v -> w where X has that edge,
// else of u -> w for the smallest predecessor u > v of w (the predecessors of w are the flipped successors of flip(w): the inputs are
// bidirectional), else the length of w's record.  With the cross ranks the merged body of a record is an interleave: W's visit j lies at
// j + c_j, R's visit i at i + |{j : c_j <= i}|.  The interleaved bodies are what build.hip has after its ranking, and its edge, size and
// fill phases make the bytes (encode_sorted_bodies); the offset of a merged edge v -> w is P_a(w, v) + P_b(w, v).
// Positions are u32 (build.hpp); every kernel indexes with 64 bits and checks what it writes against the size of the array.  No
// atomics: the same inputs give the same bytes.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "build.hpp"
#include "capi_internal.hpp"
#include "device_common.hpp"
#include "hip_raii.hpp"
#include "lf_device.hpp"
#include "merge.hpp"

namespace gbwt_hip {

namespace {

using namespace record_access;

constexpr uint32_t THREADS = 256;

using Scratch = CountedScratch;
using Buf = CountedBuf;

__device__ __forceinline__ uint64_t global_thread() { return static_cast<uint64_t>(blockIdx.x) * THREADS + threadIdx.x; }

// An input with the first position of every record (first[records] = sequences + visits)
struct Side {
    DeviceIndex ix;
    const uint32_t *first;
    uint64_t sequences;
};

// P_X(w, v) where X has no edge v -> w: through the smallest predecessor of w above v.  The edge list of flip(w) is sorted by the
// successor, that is by flip(u): of the two orientations of a node the reverse one comes first as a predecessor, so the whole list
// is looked at and the minimum taken.
__device__ __forceinline__ uint64_t pred_rank_without_edge(const Side &x, uint64_t w, uint64_t v) {
    const uint64_t rw = record_of_node(x.ix, w);
    if (rw == NO_RECORD) return 0;
    const uint64_t len = x.first[rw + 1] - x.first[rw];
    if (len == 0) return 0;
    uint64_t best = NO_RECORD;
    ByteCursor c(x.ix.data, 0, 0);
    uint64_t sigma;
    const uint64_t rf = record_of_node(x.ix, w ^ 1);
    if (rf != NO_RECORD && open_by_record(x.ix, rf, c, sigma)) {
        uint64_t node = 0;
        for (uint64_t e = 0; e < sigma; e++) {
            uint64_t delta, off;
            if (!c.varint(delta) || !c.varint(off)) break;
            node += delta;
            const uint64_t u = node ^ 1;
            if (node != 0 && u > v && u < best) best = u;
        }
    }
    uint64_t offset = len;
    if (best != NO_RECORD) (void)edge_offset_of(x.ix, best, w, offset);
    return offset;
}

// P_X(w, v): visits of w in X whose predecessor is below v; v = 0 is the endmarker, v = 1 stands for "below every node"
__device__ __forceinline__ uint64_t pred_rank(const Side &x, uint64_t w, uint64_t v) {
    if (v == 0 || w == 0) return 0;
    uint64_t offset;
    if (v >= 2 && edge_offset_of(x.ix, v, w, offset)) return offset;
    return pred_rank_without_edge(x, w, v);
}

// the cross rank behind the step v -> w for a sequence with cross rank c in v's record of R
__device__ __forceinline__ uint64_t cross_step(const Side &R, uint64_t v, uint64_t w, uint64_t c) {
    ByteCursor cur(R.ix.data, 0, 0);
    uint64_t sigma;
    const uint64_t r = record_of_node(R.ix, v);
    if (r != NO_RECORD && open_by_record(R.ix, r, cur, sigma)) {
        uint64_t node = 0, rank = 0, offset = 0;
        bool found = false;
        for (uint64_t e = 0; e < sigma; e++) {
            uint64_t delta, off;
            if (!cur.varint(delta) || !cur.varint(off)) { found = false; break; }
            node += delta;
            if (node == w) { found = true; rank = e; offset = off; }
        }
        if (found) {
            RunDecoder rd(sigma);
            uint64_t at = 0, value, len;
            while (at < c && rd.next(cur, value, len)) {
                if (value == rank) offset += overlap(at, at + len, 0, c);
                at += len;
            }
            return offset;
        }
    }
    return pred_rank_without_edge(R, w, v);
}

// ---- lengths and bodies ----------------------------------------------------------------------------------------------------------------
// len[r] of every record (the endmarker's: the sequences), 0 at r == records, and whether a workgroup fills its body
__global__ __launch_bounds__(THREADS) void k_merge_count(DeviceIndex ix, uint64_t sequences, uint32_t *__restrict__ len, uint8_t *__restrict__ is_long) {
    const uint64_t r = global_thread();
    if (r > ix.n_records) return;
    uint64_t n = 0;
    if (r == 0) n = sequences;
    else if (r < ix.n_records) {
        ByteCursor c(ix.data, 0, 0);
        uint64_t sigma;
        if (open_by_record(ix, r, c, sigma)) n = record_len(c, sigma);
    }
    len[r] = static_cast<uint32_t>(n);
    is_long[r] = (r != 0 && r < ix.n_records && n > MERGE_LONG_RECORD) ? 1 : 0;
}

// the successor with rank `value` in the edge list that starts at `header`
__device__ __forceinline__ uint32_t successor_of_rank(const DeviceIndex &ix, uint64_t header, uint64_t limit, uint64_t value) {
    ByteCursor c(ix.data, header, limit);
    uint64_t node = 0;
    for (uint64_t e = 0; e <= value; e++) {
        uint64_t delta;
        if (!c.varint(delta) || !c.skip_varint()) return 0;
        node += delta;
    }
    return static_cast<uint32_t>(node);
}

// the endmarker's body: the first node of every sequence
__global__ __launch_bounds__(THREADS) void k_merge_decode_starts(DeviceIndex ix, uint64_t sequences, uint32_t *__restrict__ body) {
    const uint64_t x = global_thread();
    if (x >= sequences) return;
    body[x] = x < ix.n_endmarker ? ix.endmarker[x].x : 0u;
}

// bodies of at most MERGE_LONG_RECORD visits: one lane per record
__global__ __launch_bounds__(THREADS) void k_merge_decode(DeviceIndex ix, const uint32_t *__restrict__ first, uint32_t *__restrict__ body) {
    const uint64_t r = global_thread() + 1;
    if (r >= ix.n_records) return;
    const uint64_t base = first[r], n = first[r + 1] - base;
    if (n == 0 || n > MERGE_LONG_RECORD) return;
    ByteCursor c(ix.data, 0, 0);
    uint64_t sigma;
    if (!open_by_record(ix, r, c, sigma)) return;
    const uint64_t header = c.pos, limit = c.limit;
    for (uint64_t k = 0; k < 2 * sigma; k++)
        if (!c.skip_varint()) return;
    RunDecoder rd(sigma);
    uint64_t at = 0, value, len, known = NO_RECORD;
    uint32_t node = 0;
    while (at < n && rd.next(c, value, len)) {
        if (value != known) { node = successor_of_rank(ix, header, limit, value); known = value; }
        for (uint64_t k = 0; k < len && at < n; k++) body[base + at++] = node;
    }
}

// longer bodies: one workgroup per record.  The run stream has no random access, so lane 0 reads it, 256 runs at a time, into LDS;
// then every lane resolves the successor of one run and all of them write the positions of the batch.
__global__ __launch_bounds__(THREADS) void k_merge_decode_long(DeviceIndex ix, const uint32_t *__restrict__ first, const uint32_t *__restrict__ long_records, uint64_t n_long,
                                                               uint32_t *__restrict__ body) {
    __shared__ uint32_t s_value[THREADS], s_start[THREADS + 1], s_runs;
    if (blockIdx.x >= n_long) return;
    const uint64_t r = long_records[blockIdx.x];
    if (r == 0 || r >= ix.n_records) return;
    const uint64_t base = first[r], n = first[r + 1] - base;
    ByteCursor c(ix.data, 0, 0);
    uint64_t sigma = 0;
    const bool ok = open_by_record(ix, r, c, sigma);       // (the same answer in every lane)
    if (!ok) return;
    const uint64_t header = c.pos, limit = c.limit;
    if (threadIdx.x == 0)
        for (uint64_t k = 0; k < 2 * sigma; k++)
            if (!c.skip_varint()) break;
    RunDecoder rd(sigma);
    uint64_t at = 0;                                        // lane 0: positions read so far
    for (;;) {
        if (threadIdx.x == 0) {
            uint32_t runs = 0;
            uint64_t value, len;
            while (runs < THREADS && at < n && rd.next(c, value, len)) {
                s_value[runs] = static_cast<uint32_t>(value);
                s_start[runs] = static_cast<uint32_t>(at);
                at = at + len < n ? at + len : n;
                runs++;
            }
            s_start[runs] = static_cast<uint32_t>(at);
            s_runs = runs;
        }
        __syncthreads();
        const uint32_t runs = s_runs;
        if (runs == 0) break;
        uint32_t node = 0;
        if (threadIdx.x < runs) node = successor_of_rank(ix, header, limit, s_value[threadIdx.x]);
        __syncthreads();
        if (threadIdx.x < runs) s_value[threadIdx.x] = node;
        __syncthreads();
        const uint64_t lo = s_start[0], hi = s_start[runs];
        for (uint64_t p = lo + threadIdx.x; p < hi; p += THREADS) {
            const uint64_t k = merge_upper_bound(s_start, runs, p) - 1;       // s_start[0] <= p
            body[base + p] = s_value[k];
        }
        __syncthreads();
    }
}

// ---- the walk --------------------------------------------------------------------------------------------------------------------------
// One lane per sequence of W.  walked_is_b: W's sequences follow R's in the result, so in R's endmarker a sequence of W stands behind
// all of R's (cross rank sequences(R)), else in front of them (0).
__global__ __launch_bounds__(THREADS) void k_merge_walk(Side W, Side R, uint32_t walked_is_b, uint64_t positions, uint64_t max_steps, uint32_t *__restrict__ cross) {
    const uint64_t x = global_thread();
    if (x >= W.sequences) return;
    cross[x] = walked_is_b ? static_cast<uint32_t>(R.sequences) : 0u;
    if (x >= W.ix.n_endmarker) return;
    const uint2 start = W.ix.endmarker[x];
    uint64_t v = start.x, i = start.y;
    if (v == 0) return;
    uint64_t c = walked_is_b ? pred_rank(R, v, 1) : 0;
    for (uint64_t step = 0; step < max_steps; step++) {
        const uint64_t r = record_of_node(W.ix, v);
        if (r == NO_RECORD) return;
        const uint64_t at = static_cast<uint64_t>(W.first[r]) + i;
        if (at >= W.first[r + 1] || at >= positions) return;
        cross[at] = static_cast<uint32_t>(c);
        uint64_t w, j;
        if (!gbwt_forward(W.ix, v, i, w, j)) return;
        c = cross_step(R, v, w, c);
        v = w; i = j;
    }
}

// ---- the interleave ------------------------------------------------------------------------------------------------------------------------
// lengths of the merged records (0 at r == records)
__global__ __launch_bounds__(THREADS) void k_merge_lengths(Side A, Side B, uint64_t records, uint64_t alphabet_offset, uint32_t *__restrict__ len) {
    const uint64_t r = global_thread();
    if (r > records) return;
    uint64_t n = 0;
    if (r < records) {
        const uint64_t v = r == 0 ? 0 : r + alphabet_offset;
        const uint64_t ra = record_of_node(A.ix, v), rb = record_of_node(B.ix, v);
        if (ra != NO_RECORD) n += A.first[ra + 1] - A.first[ra];
        if (rb != NO_RECORD) n += B.first[rb + 1] - B.first[rb];
    }
    len[r] = static_cast<uint32_t>(n);
}

// Position t of X's bodies: its record and its place in it
__device__ __forceinline__ void locate_position(const Side &X, uint64_t t, uint64_t &r, uint64_t &k) {
    r = merge_upper_bound(X.first, X.ix.n_records + 1, t) - 1;     // the last record that starts at or before t: the one that is not empty
    k = t - X.first[r];
}

__global__ __launch_bounds__(THREADS) void k_merge_interleave(Side W, Side R, const uint32_t *__restrict__ body_w, const uint32_t *__restrict__ body_r, const uint32_t *__restrict__ cross,
                                                             uint64_t positions_w, uint64_t positions_r, const uint32_t *__restrict__ first, uint64_t records, uint64_t alphabet_offset,
                                                             uint64_t slots, uint32_t *__restrict__ rec, uint32_t *__restrict__ succ) {
    const uint64_t t = global_thread();
    if (t >= positions_w + positions_r) return;
    uint64_t r, k, v, at;
    uint32_t next;
    if (t < positions_w) {                                   // W's visit j with cross rank c_j lies at j + c_j
        locate_position(W, t, r, k);
        v = node_of_record(W.ix, r);
        at = k + cross[t];
        next = body_w[t];
    } else {                                                 // R's visit i at i + |{j : c_j <= i}|
        const uint64_t u = t - positions_w;
        locate_position(R, u, r, k);
        v = node_of_record(R.ix, r);
        const uint64_t rw = record_of_node(W.ix, v);
        at = k;
        if (rw != NO_RECORD) at += merge_upper_bound(cross + W.first[rw], W.first[rw + 1] - W.first[rw], k);
        next = body_r[u];
    }
    const uint64_t rm = v == 0 ? 0 : v - alphabet_offset;
    if (rm >= records) return;                                // (an input whose header understates its alphabet)
    const uint64_t out = static_cast<uint64_t>(first[rm]) + at;
    if (out >= first[rm + 1] || out >= slots) return;        // (cannot happen for consistent inputs)
    rec[out] = static_cast<uint32_t>(v);
    succ[out] = next;
}

// ---- edge offsets ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void k_merge_edge_offsets(Side A, Side B, const uint64_t *__restrict__ edge, uint64_t edges, uint32_t *__restrict__ edge_offset) {
    const uint64_t e = global_thread();
    if (e >= edges) return;
    const uint64_t v = edge[e] >> 32, w = edge[e] & 0xFFFFFFFFull;
    if (v == 0 || w == 0) return;                            // (the 0 of the memset)
    edge_offset[e] = static_cast<uint32_t>(pred_rank(A, w, v) + pred_rank(B, w, v));
}

__global__ __launch_bounds__(THREADS) void k_merge_concat(const uint64_t *__restrict__ off_a, const uint32_t *__restrict__ nodes_a, uint64_t na, uint64_t ta, const uint64_t *__restrict__ off_b,
                                                         const uint32_t *__restrict__ nodes_b, uint64_t nb, uint64_t tb, uint64_t *__restrict__ offsets, uint32_t *__restrict__ nodes) {
    const uint64_t t = global_thread();
    if (t < ta) nodes[t] = nodes_a[t];
    else if (t < ta + tb) nodes[t] = nodes_b[t - ta];
    if (t < na) offsets[t] = off_a[t];
    else if (t < na + nb) offsets[t] = ta + off_b[t - na];
    else if (t == na + nb) offsets[t] = ta + tb;
}

}  // namespace

void merge_decode_bodies(const MergeInput &in, MergeDecoded &d, CountedScratch &sc, CountedBuf &temp, hipStream_t s) {
    const uint64_t records = in.ix.n_records;
    d.positions = in.sequences + in.visits;
    d.first.alloc(sc, (records + 1) * sizeof(uint32_t));
    d.body.alloc(sc, d.positions * sizeof(uint32_t));
    Buf len(sc, (records + 1) * sizeof(uint32_t)), is_long(sc, records + 1), long_records(sc, (records + 1) * sizeof(uint32_t)), count(sc, sizeof(uint64_t));
    k_merge_count<<<blocks_for(records + 1), THREADS, 0, s>>>(in.ix, in.sequences, len.as<uint32_t>(), is_long.as<uint8_t>());
    exclusive_sum(len.as<uint32_t>(), d.first.as<uint32_t>(), records + 1, sc, temp, s);
    hipcub::CountingInputIterator<uint32_t> ids(0);
    size_t bytes = 0;
    HIP_CHECK(hipcub::DeviceSelect::Flagged(nullptr, bytes, ids, is_long.as<uint8_t>(), long_records.as<uint32_t>(), count.as<uint64_t>(), static_cast<int64_t>(records), s));
    if (bytes > temp.bytes) temp.alloc(sc, bytes);
    HIP_CHECK(hipcub::DeviceSelect::Flagged(temp.ptr, bytes, ids, is_long.as<uint8_t>(), long_records.as<uint32_t>(), count.as<uint64_t>(), static_cast<int64_t>(records), s));
    uint64_t n_long = 0, total = 0;
    uint32_t last = 0;
    HIP_CHECK(hipMemcpyAsync(&n_long, count.ptr, sizeof(n_long), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(&last, d.first.as<uint32_t>() + records, sizeof(last), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    total = last;
    if (total != d.positions) throw InvalidData("merge: the records of an input hold " + std::to_string(total) + " positions, its header says " + std::to_string(d.positions));
    HIP_CHECK(hipMemsetAsync(d.body.ptr, 0, d.body.bytes, s));
    if (in.sequences) k_merge_decode_starts<<<blocks_for(in.sequences), THREADS, 0, s>>>(in.ix, in.sequences, d.body.as<uint32_t>());
    if (records > 1) k_merge_decode<<<blocks_for(records - 1), THREADS, 0, s>>>(in.ix, d.first.as<uint32_t>(), d.body.as<uint32_t>());
    if (n_long) k_merge_decode_long<<<static_cast<uint32_t>(n_long), THREADS, 0, s>>>(in.ix, d.first.as<uint32_t>(), long_records.as<uint32_t>(), n_long, d.body.as<uint32_t>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));                     // (len, is_long and long_records go out of scope)
}

void merge_records_on_device(const MergeInput &a, const MergeInput &b, BuildOutput &out, MergeWalk &walk, hipStream_t s) {
    const uint64_t slots = out.sequences + out.visits, records = out.records, alphabet_offset = out.alphabet_offset;
    Scratch sc;
    EventSet<4> ev;
    Buf temp;
    HIP_CHECK(hipEventRecord(ev.e[0], s));

    // 2. lengths and bodies of both inputs (the walk wants the lengths)
    MergeDecoded da, db;
    merge_decode_bodies(a, da, sc, temp, s);
    merge_decode_bodies(b, db, sc, temp, s);
    HIP_CHECK(hipEventRecord(ev.e[1], s));
    const Side A{a.ix, da.first.as<uint32_t>(), a.sequences}, B{b.ix, db.first.as<uint32_t>(), b.sequences};

    // 1. cross ranks of the input with fewer visits; ties go to b
    const bool walk_b = b.visits <= a.visits;
    const Side &W = walk_b ? B : A, &R = walk_b ? A : B;
    const MergeDecoded &dw = walk_b ? db : da, &dr = walk_b ? da : db;
    const MergeInput &w_in = walk_b ? b : a;
    walk.walked_input = walk_b ? 1 : 0; walk.walked_sequences = w_in.sequences; walk.walked_steps = w_in.visits;
    Buf cross(sc, dw.positions * sizeof(uint32_t));
    HIP_CHECK(hipMemsetAsync(cross.ptr, 0, cross.bytes, s));
    if (w_in.sequences) k_merge_walk<<<blocks_for(w_in.sequences), THREADS, 0, s>>>(W, R, walk_b ? 1u : 0u, dw.positions, w_in.visits, cross.as<uint32_t>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[2], s));

    // 3. the interleave
    Buf first(sc, (records + 1) * sizeof(uint32_t)), rec(sc, slots * sizeof(uint32_t)), succ(sc, slots * sizeof(uint32_t));
    {
        Buf len(sc, (records + 1) * sizeof(uint32_t));
        k_merge_lengths<<<blocks_for(records + 1), THREADS, 0, s>>>(A, B, records, alphabet_offset, len.as<uint32_t>());
        exclusive_sum(len.as<uint32_t>(), first.as<uint32_t>(), records + 1, sc, temp, s);
        HIP_CHECK(hipMemsetAsync(rec.ptr, 0, rec.bytes, s));
        HIP_CHECK(hipMemsetAsync(succ.ptr, 0, succ.bytes, s));
        k_merge_interleave<<<blocks_for(slots), THREADS, 0, s>>>(W, R, dw.body.as<uint32_t>(), dr.body.as<uint32_t>(), cross.as<uint32_t>(), dw.positions, dr.positions,
                                                                 first.as<uint32_t>(), records, alphabet_offset, slots, rec.as<uint32_t>(), succ.as<uint32_t>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ev.e[3], s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    cross.release(); first.release(); da.body.release(); db.body.release();

    // 4. edges, offsets, bytes: the construction's
    BodyOffsets offsets;
    offsets.launch = [&](const BodyEdges &e) {
        if (e.edges) k_merge_edge_offsets<<<blocks_for(e.edges), THREADS, 0, s>>>(A, B, e.edge, e.edges, e.edge_offset);
    };
    encode_sorted_bodies(rec, succ, slots, records, alphabet_offset, offsets, sc, temp, out, ev.e[3], s);
    HIP_CHECK(hipEventElapsedTime(&walk.decode_ms, ev.e[0], ev.e[1]));
    HIP_CHECK(hipEventElapsedTime(&walk.walk_ms, ev.e[1], ev.e[2]));
    HIP_CHECK(hipEventElapsedTime(&walk.interleave_ms, ev.e[2], ev.e[3]));
    out.peak_scratch = sc.peak;
}

void merge_concat_rows(const uint64_t *off_a, const uint32_t *nodes_a, uint64_t na, uint64_t ta, const uint64_t *off_b, const uint32_t *nodes_b, uint64_t nb, uint64_t tb,
                       uint64_t *offsets, uint32_t *nodes, hipStream_t s) {
    const uint64_t n = std::max(ta + tb, na + nb + 1);
    k_merge_concat<<<blocks_for(n), THREADS, 0, s>>>(off_a, nodes_a, na, ta, off_b, nodes_b, nb, tb, offsets, nodes);
    HIP_CHECK(hipGetLastError());
}

}  // namespace gbwt_hip
