// locate.hip -- locate queries: the sequence whose visit a BWT position is (the C++ GBWT's locate(node, i) and locate(SearchState); the
// reference has none: "we cannot interpret the document array samples", src/gbwt.rs:416, and its README leaves "Locate queries" open).
//
// THE LOCATE INDEX of a handle (capi_locate.hip: ensure_locate), built once by the first locate call:
//   rec_base  u64 per record (+ 1): where the positions of a SAMPLED record start in `table`, LOCATE_NONE for the others.  A record is sampled
//             when a multiplicative hash of its index falls below a threshold (the rule of the open's checkpoints, open_walks.hip, but for
//             records of any outdegree: locate takes plain single LF steps).  GBWT_HIP_LOCATE_INTERVAL = the expected records between two.
//   table     u32 per BWT position of a sampled record: the sequence id.
//   ends      for the last position of every non-empty sequence -- the one whose LF leaves to the endmarker -- the key
//             (record << 32) | offset and the sequence id, sorted by key.
//   k_locate_lengths   Record::len of every record (desc_raw where the handle has it, the record bytes otherwise); a scan places the sampled ones
//   k_locate_build     one lane per sample segment of every sequence (as k_refpos_walk numbers them; one per sequence without samples) walks
//                      its stretch carrying Pos and stores the sequence id at every position of a sampled record; the lane that reaches the
//                      end of the sequence stores the end entry.  LF is injective: every slot is written exactly once -- a slot is claimed by
//                      compare-and-swap from LOCATE_EMPTY, a second writer raises a flag, and the host compares the count with the table size.
// THE QUERY
//   k_locate_valid     valid[k] and end - start of every state, from the record's length
//   k_locate           one lane per located position: read the table when the record is sampled, else take one LF step; a lane whose step
//                      says that the sequence ended looks its (record, offset) up in the ends.  Neighbouring offsets of a record mostly take
//                      the same edge, so the lanes of a wave stay on the same records: their loads share cache lines.  A latency-bound
//                      gather like k_search: no LDS, few registers, what bounds it is the number of dependent round trips to HBM / L2 per
//                      lane (about GBWT_HIP_LOCATE_INTERVAL of them) times the waves in flight.
//   unique rows        keys (row << 32) | id, a radix sort over the bits in use, a flag at the first of every run, a scan, a compaction.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "kernels.hpp"

#include "device_common.hpp"
#include "lf_device.hpp"
#include "pos_step.hpp"

namespace gbwt_hip {

namespace {

constexpr uint32_t LOCATE_HASH = 2654435761u;     // the checkpoints' hash (open_walks.hip: CP_HASH)

__device__ __forceinline__ bool locate_sampled(uint64_t rec, uint64_t threshold) {
    return rec != 0 && static_cast<uint64_t>(static_cast<uint32_t>(rec) * LOCATE_HASH) < threshold;
}

// Record::len of record `rec` < n_records; 0 for an absent or empty one.  DESC: from the raw descriptor (C.y; saturated at 2^32 - 1).
template <bool DESC>
__device__ __forceinline__ uint64_t locate_record_len(const DeviceIndex &ix, uint64_t rec) {
    if (DESC) {
        const uint4 B = ix.desc_raw[4 * rec + 1];
        return B.y == 0 ? 0u : ix.desc_raw[4 * rec + 2].y;
    }
    uint64_t start, limit;
    record_bounds(ix, rec, start, limit);
    if (start >= limit) return 0;
    ByteCursor c(ix.data, start, limit);
    uint64_t sigma;
    if (!c.varint(sigma) || sigma == 0) return 0;
    return record_len(c, sigma);
}

// the record of a node as GBWT::find opens it (src/gbwt.rs:269-279): false for the endmarker, a node at or below the offset, past the alphabet
__device__ __forceinline__ bool locate_record_of(const DeviceIndex &ix, uint64_t node, uint64_t &rec) {
    if (node < ix.first_node) return false;
    rec = node - ix.alphabet_offset;
    return rec < ix.n_records;
}

template <bool DESC>
__global__ void __launch_bounds__(256) k_locate_lengths(DeviceIndex ix, uint64_t threshold, uint64_t *__restrict__ lens, uint32_t *flags) {
    const uint64_t rec = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (rec >= ix.n_records) return;
    const uint64_t len = rec == 0 ? 0u : locate_record_len<DESC>(ix, rec);
    if (len >= 0xFFFFFFFFull) atomicOr(flags, LOCATE_FLAG_WIDE);
    lens[rec] = locate_sampled(rec, threshold) ? len : 0u;
}

__global__ void __launch_bounds__(256) k_locate_bases(const uint64_t *__restrict__ lens, uint64_t *__restrict__ base, uint64_t n_records, uint64_t *sampled) {
    const uint64_t rec = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    const bool holds = rec < n_records && lens[rec] != 0;
    if (rec < n_records && !holds) base[rec] = LOCATE_NONE;
    const uint64_t wave = __ballot(holds);
    if (wave != 0 && (threadIdx.x & (WAVE - 1)) == 0) atomicAdd(reinterpret_cast<unsigned long long *>(sampled), static_cast<unsigned long long>(__popcll(wave)));
}

struct LocateBuild { const uint64_t *seg_first; uint64_t walkers, step_limit; uint64_t *counts; uint32_t *flags; uint32_t segmented; };

template <bool FAST>
__global__ void __launch_bounds__(256) k_locate_build(DeviceIndex ix, LocateIndex L, LocateBuild b) {
    const uint64_t t = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (t >= b.walkers) return;
    // the sequence of lane t < seg_first[n]: the last one that starts at or before t (sequences without lanes start where the next one does)
    const uint64_t id = b.segmented ? last_at_or_before(b.seg_first, ix.n_sequences, t) : t, j = b.segmented ? t - b.seg_first[id] : 0u;
    if (id >= ix.n_sequences || id >= ix.n_endmarker) { atomicOr(b.flags, LOCATE_FLAG_WALK); return; }
    // Nodes [from, to) of the sequence are this lane's (device_index.hpp: row_segments); the LAST lane of a sequence runs to its end, wherever
    // that is.  Pos of node `from`: the endmarker entry (segment 0), or one step from sample j, which is the position of node from - 1.
    uint64_t node = 0, offset = 0, stores = 0, to = ~uint64_t(0), k = 0;
    bool last = true, ok = true;
    if (b.segmented) {
        const RowSegments rs = row_segments(ix, id);
        if (j >= rs.count) { atomicOr(b.flags, LOCATE_FLAG_WALK); return; }
        last = j + 1 == rs.count;
        if (!last) to = ix.samples[rs.base + (j + 1) * rs.stride].w;
        if (j != 0) {
            const uint4 s = ix.samples[rs.base + j * rs.stride];
            k = s.w;
            node = static_cast<uint64_t>(s.x) + ix.alphabet_offset; offset = s.y;
            if (k >= to) { if (k > to) atomicOr(b.flags, LOCATE_FLAG_WALK); return; }
            const uint64_t rec = s.x, at = offset;
            if (!pos_step<FAST>(ix, node, offset)) {
                // the sample stands on the last node of the sequence: an empty stretch, and this lane knows the end
                if (last) { L.end_keys[id] = (rec << 32) | at; L.end_ids[id] = static_cast<uint32_t>(id); atomicAdd(reinterpret_cast<unsigned long long *>(b.counts + 1), 1ull); }
                else atomicOr(b.flags, LOCATE_FLAG_WALK);
                return;
            }
        }
    }
    if (j == 0) {
        const uint2 e = ix.endmarker[id];
        node = e.x; offset = e.y;
        if (node == 0) return;                       // an empty sequence: no position, no end entry
    }
    for (uint64_t steps = 0;; steps++) {
        uint64_t rec;
        if (!locate_record_of(ix, node, rec) || offset >= 0xFFFFFFFFull || steps > b.step_limit) { ok = false; break; }
        const uint64_t base = L.rec_base[rec];
        if (base != LOCATE_NONE) {
            const uint64_t slot = base + offset;
            if (slot >= L.table_positions) { ok = false; break; }
            if (atomicCAS(L.table + slot, LOCATE_EMPTY, static_cast<uint32_t>(id)) == LOCATE_EMPTY) stores++;
            else atomicOr(b.flags, LOCATE_FLAG_TWICE);
        }
        if (++k == to) break;                         // (never for the last lane)
        const uint64_t at = offset;
        if (!pos_step<FAST>(ix, node, offset)) {
            if (last) { L.end_keys[id] = (rec << 32) | at; L.end_ids[id] = static_cast<uint32_t>(id); atomicAdd(reinterpret_cast<unsigned long long *>(b.counts + 1), 1ull); }
            else ok = false;                          // the sequence ended in front of the next sample
            break;
        }
    }
    if (stores) atomicAdd(reinterpret_cast<unsigned long long *>(b.counts), static_cast<unsigned long long>(stores));
    if (!ok) atomicOr(b.flags, LOCATE_FLAG_WALK);
}

template <bool DESC>
__global__ void __launch_bounds__(256) k_locate_valid(DeviceIndex ix, const gbwt_hip_state *__restrict__ states, const uint8_t *__restrict__ given, uint64_t n,
                                                       uint64_t *__restrict__ counts, uint8_t *__restrict__ valid) {
    const uint64_t k = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (k >= n) return;
    const gbwt_hip_state st = states[k];
    uint64_t rec;
    bool ok = (given == nullptr || given[k] != 0) && st.start < st.end && locate_record_of(ix, st.node, rec);
    if (ok) ok = st.end <= locate_record_len<DESC>(ix, rec);
    valid[k] = ok ? 1 : 0;
    counts[k] = ok ? st.end - st.start : 0u;
}

// The sequence id of position (node, offset) of an existing record, offset < its length.  false: no table entry and no end entry on the way.
template <bool FAST>
__device__ __forceinline__ bool locate_one(const DeviceIndex &ix, const LocateIndex &L, uint64_t node, uint64_t offset, uint64_t step_limit, uint32_t &id, uint64_t &steps) {
    for (steps = 0; steps <= step_limit; steps++) {
        uint64_t rec;
        if (!locate_record_of(ix, node, rec)) return false;
        const uint64_t base = L.rec_base[rec];
        if (base != LOCATE_NONE) {
            if (base + offset >= L.table_positions) return false;
            id = L.table[base + offset];
            return true;
        }
        const uint64_t at = offset;
        if (!pos_step<FAST>(ix, node, offset)) {     // the sequence ended here: its end entry
            steps++;                                 // (the step that leaves to the endmarker is one)
            const uint64_t key = (rec << 32) | at;
            uint64_t lo = 0, hi = L.end_entries;
            while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (L.end_keys[mid] < key) lo = mid + 1; else hi = mid; }
            if (at > 0xFFFFFFFFull || lo >= L.end_entries || L.end_keys[lo] != key) return false;
            id = L.end_ids[lo];
            return true;
        }
    }
    return false;
}

struct LocateQuery { const gbwt_hip_state *states; const uint64_t *offsets; uint64_t n, total, step_limit; uint64_t *out, *steps; uint32_t *flags; uint32_t keyed; };

template <bool FAST>
__global__ void __launch_bounds__(256) k_locate(DeviceIndex ix, LocateIndex L, LocateQuery q) {
    const uint64_t t = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (t >= q.total) return;
    const uint64_t row = last_at_or_before(q.offsets, q.n, t);
    const uint64_t node = q.states[row].node, offset = q.states[row].start + (t - q.offsets[row]);
    uint32_t id = 0;
    uint64_t steps = 0;
    if (!locate_one<FAST>(ix, L, node, offset, q.step_limit, id, steps)) { id = 0; atomicOr(q.flags, LOCATE_FLAG_LOST); }
    q.out[t] = (q.keyed ? row << 32 : 0u) | id;
    if (q.steps != nullptr && steps != 0) atomicAdd(reinterpret_cast<unsigned long long *>(q.steps), static_cast<unsigned long long>(steps));
}

template <bool FAST>
__global__ void __launch_bounds__(256) k_locate_positions(DeviceIndex ix, LocateIndex L, const gbwt_hip_pos *__restrict__ pos, uint64_t n, uint64_t step_limit,
                                                           uint64_t *__restrict__ ids, uint8_t *__restrict__ valid, uint32_t *flags) {
    const uint64_t k = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (k >= n) return;
    const gbwt_hip_pos p = pos[k];
    uint64_t rec, steps = 0;
    uint32_t id = 0;
    bool ok = locate_record_of(ix, p.node, rec);
    if (ok) ok = p.offset < locate_record_len<FAST>(ix, rec);
    if (ok && !locate_one<FAST>(ix, L, p.node, p.offset, step_limit, id, steps)) { ok = false; id = 0; atomicOr(flags, LOCATE_FLAG_LOST); }
    ids[k] = ok ? id : 0u;
    valid[k] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_locate_run_flags(const uint64_t *__restrict__ sorted, uint64_t total, uint64_t *__restrict__ flag) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i < total) flag[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1u : 0u;
}

// rank[i] = first-of-run flags in front of item i (rank[total] = the ids kept).  The sort keeps every row's stretch of the items where it was,
// so row k keeps the ids of ranks rank[offsets[k]] .. rank[offsets[k + 1]).
__global__ void __launch_bounds__(256) k_locate_compact(const uint64_t *__restrict__ sorted, const uint64_t *__restrict__ rank, uint64_t total, const uint64_t *__restrict__ offsets,
                                                         uint64_t n, uint64_t *__restrict__ ids, uint64_t *__restrict__ new_offsets) {
    const uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x;
    if (i < total && rank[i + 1] != rank[i]) ids[rank[i]] = sorted[i] & 0xFFFFFFFFull;
    if (i <= n) new_offsets[i] = rank[offsets[i]];
}


}  // namespace

uint64_t locate_threshold(uint32_t interval) {
    if (interval == 0) return 0;
    return (uint64_t(1) << 32) / interval;
}

void launch_locate_lengths(const DeviceIndex &ix, uint64_t threshold, uint64_t *d_lens, uint32_t *d_flags, hipStream_t s) {
    if (ix.n_records == 0) return;
    if (ix.desc_raw != nullptr) hipLaunchKernelGGL(k_locate_lengths<true>, blocks_for(ix.n_records), dim3(256), 0, s, ix, threshold, d_lens, d_flags);
    else hipLaunchKernelGGL(k_locate_lengths<false>, blocks_for(ix.n_records), dim3(256), 0, s, ix, threshold, d_lens, d_flags);
}

void launch_locate_bases(const uint64_t *d_lens, uint64_t *d_base, uint64_t n_records, uint64_t *d_sampled, hipStream_t s) {
    if (n_records) hipLaunchKernelGGL(k_locate_bases, blocks_for(n_records), dim3(256), 0, s, d_lens, d_base, n_records, d_sampled);
}

void launch_locate_build(const DeviceIndex &ix, const LocateIndex &L, const uint64_t *d_seg_first, uint64_t walkers, bool segmented, uint64_t step_limit, uint64_t *d_counts,
                         uint32_t *d_flags, bool fast, hipStream_t s) {
    if (walkers == 0) return;
    const LocateBuild b{d_seg_first, walkers, step_limit, d_counts, d_flags, segmented ? 1u : 0u};
    if (fast) hipLaunchKernelGGL(k_locate_build<true>, blocks_for(walkers), dim3(256), 0, s, ix, L, b);
    else hipLaunchKernelGGL(k_locate_build<false>, blocks_for(walkers), dim3(256), 0, s, ix, L, b);
}

size_t locate_sort_temp_bytes(uint64_t n) {
    size_t pairs = 0, keys = 0;
    const int items = static_cast<int>(std::max<uint64_t>(n, 1));
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, pairs, static_cast<const uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), static_cast<const uint32_t *>(nullptr),
                                             static_cast<uint32_t *>(nullptr), items, 0, 64);
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, keys, static_cast<const uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), items, 0, 64);
    return std::max<size_t>(std::max(pairs, keys), 16);
}

void launch_locate_sort_ends(const uint64_t *d_keys_in, uint64_t *d_keys_out, const uint32_t *d_ids_in, uint32_t *d_ids_out, uint64_t n, void *d_temp, size_t temp_bytes, hipStream_t s) {
    if (n) (void)hipcub::DeviceRadixSort::SortPairs(d_temp, temp_bytes, d_keys_in, d_keys_out, d_ids_in, d_ids_out, static_cast<int>(n), 0, 64, s);
}

void launch_locate_valid(const DeviceIndex &ix, const gbwt_hip_state *d_states, const uint8_t *d_given, uint64_t n, uint64_t *d_counts, uint8_t *d_valid, hipStream_t s) {
    if (n == 0) return;
    if (ix.desc_raw != nullptr) hipLaunchKernelGGL(k_locate_valid<true>, blocks_for(n), dim3(256), 0, s, ix, d_states, d_given, n, d_counts, d_valid);
    else hipLaunchKernelGGL(k_locate_valid<false>, blocks_for(n), dim3(256), 0, s, ix, d_states, d_given, n, d_counts, d_valid);
}

void launch_locate(const DeviceIndex &ix, const LocateIndex &L, const gbwt_hip_state *d_states, const uint64_t *d_offsets, uint64_t n, uint64_t total, bool keyed,
                   uint64_t step_limit, uint64_t *d_out, uint64_t *d_steps, uint32_t *d_flags, bool fast, hipStream_t s) {
    if (total == 0 || n == 0) return;
    const LocateQuery q{d_states, d_offsets, n, total, step_limit, d_out, d_steps, d_flags, keyed ? 1u : 0u};
    if (fast) hipLaunchKernelGGL(k_locate<true>, blocks_for(total), dim3(256), 0, s, ix, L, q);
    else hipLaunchKernelGGL(k_locate<false>, blocks_for(total), dim3(256), 0, s, ix, L, q);
}

void launch_locate_positions(const DeviceIndex &ix, const LocateIndex &L, const gbwt_hip_pos *d_pos, uint64_t n, uint64_t step_limit, uint64_t *d_ids, uint8_t *d_valid,
                             uint32_t *d_flags, bool fast, hipStream_t s) {
    if (n == 0) return;
    if (fast) hipLaunchKernelGGL(k_locate_positions<true>, blocks_for(n), dim3(256), 0, s, ix, L, d_pos, n, step_limit, d_ids, d_valid, d_flags);
    else hipLaunchKernelGGL(k_locate_positions<false>, blocks_for(n), dim3(256), 0, s, ix, L, d_pos, n, step_limit, d_ids, d_valid, d_flags);
}

void launch_locate_sort_keys(const uint64_t *d_in, uint64_t *d_out, uint64_t n, int bits, void *d_temp, size_t temp_bytes, hipStream_t s) {
    if (n) (void)hipcub::DeviceRadixSort::SortKeys(d_temp, temp_bytes, d_in, d_out, static_cast<int>(n), 0, bits, s);
}

void launch_locate_run_flags(const uint64_t *d_sorted, uint64_t total, uint64_t *d_flag, hipStream_t s) {
    if (total) hipLaunchKernelGGL(k_locate_run_flags, blocks_for(total), dim3(256), 0, s, d_sorted, total, d_flag);
}

void launch_locate_compact(const uint64_t *d_sorted, const uint64_t *d_rank, uint64_t total, const uint64_t *d_offsets, uint64_t n, uint64_t *d_ids, uint64_t *d_new_offsets,
                           hipStream_t s) {
    hipLaunchKernelGGL(k_locate_compact, blocks_for(std::max(total, n + 1)), dim3(256), 0, s, d_sorted, d_rank, total, d_offsets, n, d_ids, d_new_offsets);
}

}  // namespace gbwt_hip
