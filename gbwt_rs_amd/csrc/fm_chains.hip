// fm_chains.hip -- the colinear chains of a read's hits (include/gbwt_hip.h, "Chains of seeds"): the kernels of the chaining
// behind a seeds request.  What a predecessor, a score and a chain are is fm_chains.hpp, shared with the host; the calls are capi_fm_chains.hip.
//
// EXPAND.  The seeds rows hold a read's forward seeds and then its reverse seeds, and the hits stand in seed order: the hits of an item --
// one read on one strand -- are one stretch of the hits, and the items in read-major order are the order of the result.  One lane per
// match writes (item << 32 | y, x << 32 | w) in that order, where x ascends inside an item; a stable radix sort over the bits in use
// leaves every item ordered by (y, x).
//
// THE DP is the hot kernel: one wave per item.  The wave takes the matches i of its item in order, 64 at a time into registers (one per
// lane, read back with v_readlane), and for each i its lanes take the candidates j of the window [first j with y_j >= low(i), i) 64 at a
// time: y, x of every j and the f the wave has written for it come from LDS (8 + 4 bytes per match, up to FM_CHAIN_TILE matches; a larger
// item runs the same body over global memory, its f through L2).  The first chunk of a window also tells how far its lower end moves:
// low(i) never decreases.  One reduction of the key (c << 32) | j picks f(i) and pred(i).  The loop is sequential in i and bound by the
// LDS round trip of a chunk and the shuffles of the reduction, so the waves in flight are the throughput: 24 KB of LDS per workgroup of
// four waves leaves six workgroups on a CU.
//
// PEEL.  A second stable sort by (item, f descending) gives the visiting order; one lane per item walks it with a byte of `used` per
// match.  Flags and member counts per visiting slot, their scans, and the chains and members go to their places: a walk runs backward, so
// a member's place counts from the end of its chain's row.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "device_common.hpp"
#include "fm_chain_kernels.hpp"
#include "fm_chain_plan.hpp"
#include "fm_seeds.hpp"

namespace gbwt_hip {

namespace {

constexpr unsigned THREADS = 256;
constexpr unsigned DP_WAVES = 4, DP_THREADS = DP_WAVES * WAVE;
constexpr uint32_t TILE = static_cast<uint32_t>(FM_CHAIN_TILE);

// the bits of the keys (item << 32 | 32 bits) that a request uses
inline int key_bits(uint64_t items) { return 32 + bits_for(items, 32); }

// The seeds of item q in the seeds rows: [first, last)
__device__ __forceinline__ void item_seeds(const ChainBatch &b, uint64_t q, uint64_t &first, uint64_t &last) {
    const uint64_t r = q / b.ns;
    first = b.seed_read_offsets[r];
    last = b.seed_read_offsets[r + 1];
    if (b.ns == 1) return;
    uint64_t lo = first, hi = last;                      // the first seed of the row on the reverse strand
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (b.seeds[mid].strand < FM_STRAND_REVERSE) lo = mid + 1; else hi = mid;
    }
    if (q % b.ns == 0) last = lo; else first = lo;
}

__global__ void __launch_bounds__(THREADS) k_chain_item_counts(ChainBatch b) {
    const uint64_t q = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (q == 0) b.hit_first[b.items] = b.total_hits;
    if (q >= b.items) return;
    uint64_t first = 0, last = 0;
    item_seeds(b, q, first, last);
    const uint64_t from = b.hit_offsets[first];
    uint64_t count = b.hit_offsets[last] - from;
    if (b.max_matches != 0 && count > b.max_matches) {
        count = 0;
        atomicAdd(reinterpret_cast<unsigned long long *>(b.words), 1ull);
    }
    b.counts[q] = count;
    b.hit_first[q] = from;
}

__global__ void __launch_bounds__(THREADS) k_chain_expand(ChainBatch b) {
    const uint64_t g = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (g >= b.matches) return;
    const uint64_t q = last_at_or_before(b.match_offsets, b.items, g);
    const uint64_t h = b.hit_first[q] + (g - b.match_offsets[q]);
    const gbwt_hip_fm_seed seed = b.seeds[last_at_or_before(b.hit_offsets, b.total_seeds, h)];
    b.key_a[g] = (q << 32) | static_cast<uint32_t>(b.positions[h]);
    b.val_a[g] = (static_cast<uint64_t>(seed.start) << 32) | (seed.end - seed.start);
}

__global__ void __launch_bounds__(THREADS) k_chain_unpack(ChainBatch b) {
    const uint64_t g = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (g >= b.matches) return;
    const uint32_t y = static_cast<uint32_t>(b.key_b[g]);
    const uint64_t xw = b.val_b[g];
    uint32_t seg = 0, seg_start = 0;
    if (b.path_offsets) {
        seg = static_cast<uint32_t>(last_at_or_before(b.path_offsets, 0, b.n_paths, y));
        seg_start = static_cast<uint32_t>(b.path_offsets[seg]);
    }
    b.y[g] = y;
    b.x[g] = static_cast<uint32_t>(xw >> 32);
    b.w[g] = static_cast<uint32_t>(xw);
    b.seg[g] = seg;
    b.low[g] = fm_chain_low(y, seg_start, b.P.max_gap);
}

__device__ __forceinline__ uint64_t wave_max64(uint64_t v, uint32_t lane) {
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        const uint64_t other = shfl64(v, static_cast<int>(lane ^ d));
        v = other > v ? other : v;
    }
    return v;
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v, uint32_t lane) {
    for (int d = WAVE / 2; d > 0; d >>= 1) v += shfl64(v, static_cast<int>(lane ^ d));
    return v;
}

__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t lane) {           // lane: the same in every lane of the wave
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), static_cast<int>(lane)));
}

// What one lane of the wave has written to LDS, every lane may read behind this
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The n matches of one item that starts at match a, by one wave.  STAGED: n <= TILE, and (y, x) and f of the item go through syx / sf;
// otherwise y and x are read from global memory and f travels through L2: written by lane 0 and acknowledged before any lane reads it.
template <bool STAGED>
__device__ __forceinline__ void dp_item(const ChainBatch &b, uint64_t a, uint32_t n, uint2 *syx, uint32_t *sf, uint32_t lane, uint64_t &pairs) {
    const uint32_t *gy = b.y + a, *gx = b.x + a, *gw = b.w + a, *glow = b.low + a;
    uint32_t *gf = b.f + a, *gpred = b.pred + a;
    const FmChainParams P = b.P;
    uint32_t lo = 0;                                     // the lower end of the window: it only moves forward
    for (uint32_t i0 = 0; i0 < n; i0 += WAVE) {
        const uint32_t mine = i0 + lane;
        uint32_t my_y = 0, my_x = 0, my_w = 0, my_low = 0, my_f = 0, my_pred = FM_CHAIN_NONE;
        if (mine < n) { my_y = gy[mine]; my_x = gx[mine]; my_w = gw[mine]; my_low = glow[mine]; }
        if (STAGED) {
            if (mine < n) syx[mine] = make_uint2(my_y, my_x);
            wave_lds_fence();
        }
        const uint32_t count = n - i0 < WAVE ? n - i0 : WAVE;
        for (uint32_t ii = 0; ii < count; ii++) {
            const uint32_t i = i0 + ii;
            const uint32_t yi = lane_value(my_y, ii), xi = lane_value(my_x, ii), wi = lane_value(my_w, ii), low_i = lane_value(my_low, ii);
            uint64_t best = 0;
            bool advancing = true;
            for (uint32_t base = lo; base < i; base += WAVE) {
                const uint32_t j = base + lane;
                const bool valid = j < i;
                uint32_t yj = 0, xj = 0, fj = 0;
                if (valid) {
                    if (STAGED) {
                        const uint2 yx = syx[j];
                        yj = yx.x; xj = yx.y; fj = sf[j];
                    } else {
                        yj = gy[j]; xj = gx[j];
                        fj = __hip_atomic_load(gf + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                if (advancing) {                         // the matches ascend by y: those below low(i) are a prefix of the chunk
                    const uint32_t below = static_cast<uint32_t>(__popcll(__ballot(valid && yj < low_i)));
                    lo += below;
                    advancing = below == WAVE;
                }
                if (valid) best = fm_chain_step(best, j, yj, xj, fj, yi, xi, wi, low_i, P, pairs);
            }
            if (__ballot(best != 0) != 0) best = wave_max64(best, lane);
            uint32_t fi = 0, pi = 0;
            fm_chain_result(best, wi, fi, pi);
            if (lane == ii) { my_f = fi; my_pred = pi; }
            if (STAGED) {
                if (lane == 0) sf[i] = fi;
                wave_lds_fence();
            } else {
                if (lane == 0) __hip_atomic_store(gf + i, fi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (mine < n) {
            if (STAGED) gf[mine] = my_f;
            gpred[mine] = my_pred;
        }
    }
}

__global__ void __launch_bounds__(DP_THREADS) k_chain_dp(ChainBatch b) {
    __shared__ uint2 syx[DP_WAVES][TILE];
    __shared__ uint32_t sf[DP_WAVES][TILE];
    const uint32_t wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const uint64_t q = uint64_t(blockIdx.x) * DP_WAVES + wave;
    if (q >= b.items) return;                            // (no barrier of the workgroup below: a wave is on its own)
    const uint64_t a = b.match_offsets[q];
    const uint64_t n = b.match_offsets[q + 1] - a;
    uint64_t pairs = 0;
    if (n <= TILE) dp_item<true>(b, a, static_cast<uint32_t>(n), syx[wave], sf[wave], lane, pairs);
    else dp_item<false>(b, a, static_cast<uint32_t>(n), nullptr, nullptr, lane, pairs);
    if (n < 2) return;
    pairs = wave_sum64(pairs, lane);
    if (lane == 0 && pairs != 0) atomicAdd(reinterpret_cast<unsigned long long *>(b.words + 1), static_cast<unsigned long long>(pairs));
}

__global__ void __launch_bounds__(THREADS) k_chain_visit_keys(ChainBatch b, uint32_t *__restrict__ index) {
    const uint64_t g = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (g >= b.matches) return;
    b.key_a[g] = fm_chain_visit_key(b.key_b[g] >> 32, b.f[g]);
    index[g] = static_cast<uint32_t>(g);
}

__global__ void __launch_bounds__(THREADS) k_chain_peel(ChainBatch b, const uint32_t *__restrict__ order) {
    const uint64_t q = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (q >= b.items) return;
    const uint64_t a = b.match_offsets[q];
    const uint32_t n = static_cast<uint32_t>(b.match_offsets[q + 1] - a);
    for (uint32_t t = 0; t < n; t++) {
        const uint32_t head = static_cast<uint32_t>(order[a + t] - a);
        uint64_t flag = 0, members = 0;
        if (!b.used[a + head]) {
            int64_t score = 0;
            uint32_t tail = head;
            const uint32_t walked = fm_chain_peel(head, t, b.f + a, b.pred + a, b.used + a, b.member_slot + a, b.member_pos + a, score, tail);
            b.slot_score[a + t] = static_cast<uint32_t>(score);          // (read for reported chains only: there it is 1 .. f)
            b.slot_tail[a + t] = tail;
            if (fm_chain_reported(score, b.P)) { flag = 1; members = walked; }
        }
        b.flags[a + t] = flag;
        b.members[a + t] = members;
    }
}

__global__ void __launch_bounds__(THREADS) k_chain_fill(ChainBatch b, uint64_t total_chains, uint64_t *__restrict__ read_offsets, gbwt_hip_fm_chain *__restrict__ chains,
                                                        uint64_t *__restrict__ chain_match_offsets, gbwt_hip_fm_chain_match *__restrict__ matches) {
    const uint64_t g = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (g <= b.m) read_offsets[g] = b.rank[b.match_offsets[g * b.ns < b.items ? g * b.ns : b.items]];
    if (g == 0) chain_match_offsets[total_chains] = b.member_rank[b.matches];
    if (g >= b.matches) return;
    const uint64_t q = b.key_b[g] >> 32;
    const uint64_t a = b.match_offsets[q];
    const uint64_t t = a + b.member_slot[g];
    if (!b.flags[t]) return;
    const uint64_t c = b.rank[t], first = b.member_rank[t];
    const uint32_t members = static_cast<uint32_t>(b.members[t]), pos = b.member_pos[g];
    matches[first + (members - 1 - pos)] = gbwt_hip_fm_chain_match{b.y[g], b.x[g], b.w[g]};
    if (pos != 0) return;
    const uint64_t tail = a + b.slot_tail[t];
    chains[c] = fm_chain_summary(b.y[tail], b.x[tail], b.y[g], b.x[g], b.w[g], b.slot_score[t], members, fm_strand_at(b.strands, static_cast<uint32_t>(q % b.ns)), b.seg[g]);
    chain_match_offsets[c] = first;
}

}  // namespace

namespace {

// The temporary storage hipcub asks for the sorts of `count` pairs: the matches by (item, y), and the visits
hipError_t sort_temp_bytes(uint64_t count, uint64_t items, size_t &matches, size_t &visits) {
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, matches, static_cast<const uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), static_cast<const uint64_t *>(nullptr),
                                                      static_cast<uint64_t *>(nullptr), static_cast<int>(count), 0, key_bits(items));
    if (e != hipSuccess) return e;
    return hipcub::DeviceRadixSort::SortPairs(nullptr, visits, static_cast<const uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), static_cast<const uint32_t *>(nullptr),
                                              static_cast<uint32_t *>(nullptr), static_cast<int>(count), 0, key_bits(items));
}

}  // namespace

hipError_t chain_sort_temp_bytes(uint64_t hits, uint64_t items, size_t &bytes) {
    size_t matches = 0, visits = 0;
    const hipError_t e = sort_temp_bytes(hits, items, matches, visits);
    bytes = std::max<size_t>(std::max(matches, visits), 1);
    return e;
}

void launch_chain_item_counts(const ChainBatch &b, hipStream_t s) {
    hipLaunchKernelGGL(k_chain_item_counts, blocks_for(std::max<uint64_t>(b.items, 1)), dim3(THREADS), 0, s, b);
}

void launch_chain_expand(const ChainBatch &b, hipStream_t s) {
    if (b.matches) hipLaunchKernelGGL(k_chain_expand, blocks_for(b.matches), dim3(THREADS), 0, s, b);
}

// The plan sizes the temporary storage for the hits and a sort runs over the matches, which may be fewer: what hipcub asks for them is
// asked again and held against what there is, so that storage too small is an error and never a sort into it
hipError_t launch_chain_sort_matches(const ChainBatch &b, void *d_temp, size_t temp_bytes, hipStream_t s) {
    if (!b.matches) return hipSuccess;
    size_t need = 0, visits = 0;
    hipError_t e = sort_temp_bytes(b.matches, b.items, need, visits);
    if (e == hipSuccess && need > temp_bytes) e = hipErrorInvalidValue;
    if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(d_temp, temp_bytes, b.key_a, b.key_b, b.val_a, b.val_b, static_cast<int>(b.matches), 0, key_bits(b.items), s);   // radix sort: stable
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_chain_unpack, blocks_for(b.matches), dim3(THREADS), 0, s, b);
    return hipSuccess;
}

void launch_chain_dp(const ChainBatch &b, hipStream_t s) {
    if (b.matches) hipLaunchKernelGGL(k_chain_dp, grid_for(b.items, DP_WAVES), dim3(DP_THREADS), 0, s, b);
}

hipError_t launch_chain_sort_visits(const ChainBatch &b, void *d_temp, size_t temp_bytes, hipStream_t s) {
    if (!b.matches) return hipSuccess;
    size_t matches = 0, need = 0;
    const hipError_t e = sort_temp_bytes(b.matches, b.items, matches, need);
    if (e != hipSuccess) return e;
    if (need > temp_bytes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_chain_visit_keys, blocks_for(b.matches), dim3(THREADS), 0, s, b, chain_visit_index(b));
    return hipcub::DeviceRadixSort::SortPairs(d_temp, temp_bytes, b.key_a, b.val_a, chain_visit_index(b), chain_visit_order(b), static_cast<int>(b.matches), 0, key_bits(b.items), s);
}

void launch_chain_peel(const ChainBatch &b, hipStream_t s) {
    if (b.matches) hipLaunchKernelGGL(k_chain_peel, blocks_for(b.items), dim3(THREADS), 0, s, b, chain_visit_order(b));
}

void launch_chain_fill(const ChainBatch &b, uint64_t total_chains, uint64_t *d_read_offsets, gbwt_hip_fm_chain *d_chains, uint64_t *d_chain_match_offsets,
                       gbwt_hip_fm_chain_match *d_matches, hipStream_t s) {
    hipLaunchKernelGGL(k_chain_fill, blocks_for(std::max(b.matches, b.m + 1)), dim3(THREADS), 0, s, b, total_chains, d_read_offsets, d_chains, d_chain_match_offsets, d_matches);
}

}  // namespace gbwt_hip
