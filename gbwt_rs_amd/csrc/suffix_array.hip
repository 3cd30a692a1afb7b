// suffix_array.hip -- suffix array and BWT of a text in HBM: what stands between gbz-extract's `sequences` and `tag-array` modes
// (src/bin/gbz-extract.rs:321-344, 373-406 read a `base`.sa and a `base`.bwt that nothing in the reference makes).
//
// ORDER (sa_key.hpp): the suffixes of T[0, n) as unsigned byte strings compared to the end of the text, a proper prefix first.  All suffixes
// differ in length, so the array is unique and no step below needs a tie-break or a stable sort.
//
// PREFIX DOUBLING OVER THE ACTIVE SET.  `sa` (u32) is the array as it settles, `rank` (u32) its inverse: rank[p] = 1 + the place in `sa` of
// the first suffix of p's GROUP, the suffixes not yet told apart from p.  Round 0 sorts all suffixes by their first key (7 bytes and how
// many of them the suffix has; k_sa_pack).  Behind a sort, k_sa_heads marks the entries whose key differs from the one in front with their
// own place + 1, a max-scan spreads the marks over the groups, and k_sa_scatter writes rank and sa and flags what still shares its rank.
// Those -- the ACTIVE SET -- are selected (hipcub) and, by k_sa_next, given the key (rank of the group, rank[p + h]) for the next round:
// only they are sorted again, over the 2 * rank_bits bits in use, and since the groups are contiguous and in order in the set, entry c of
// it belongs to a place of `sa` that does not change while its group is sorted: slot[c].  A group's new ranks start at its old first
// rank, so a settled suffix never moves and its rank is final.  Round k compares 7 * 2^k bytes; the host reads one word per round, the
// size of the active set, and stops at 0.  A suffix that ends within h positions has second rank 0: it is a proper prefix of the others.
//
// OUTPUT (k_sa_output): the u64 array, BWT[i] = T[sa[i] - 1] (the sentinel for suffix 0) and the runs of the BWT in one pass, counted as
// k_tags counts its runs: a workgroup owns a contiguous range of tiles, the byte in front of a tile is kept in LDS, one atomic per workgroup.
//
// hipcub sorts, scans and selects; the kernels here use no atomics but that one.  Registers, LDS and bounds of the kernels: DESIGN.md 4n.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>

#include "build.hpp"
#include "sa_key.hpp"
#include "sa_plan.hpp"
#include "suffix_array.hpp"

using namespace gbwt_hip;

namespace {

constexpr uint32_t SA_THREADS = 256, SA_PER = 4, SA_TILE = SA_THREADS * SA_PER;
// The words of a pack tile: its SA_TILE positions, the 8 bytes behind the last one that its key window reads, up to 3 bytes in front
// (the text need not be aligned), rounded up: ceil((3 + 1024 + 8) / 4) = 259, and one so that every window has a third word
constexpr uint32_t PACK_WORDS = (3 + SA_TILE + 8 + 3) / 4 + 1;
constexpr unsigned MAX_BLOCKS = 2048;

// First keys (sa_key.hpp).  A tile of the text goes through LDS as aligned words -- one coalesced load per lane -- and every lane cuts the
// eight bytes of its four positions out of three of them.  A word is loaded only when it holds a byte of the text; entry i of a tile is
// position j * 256 + t of thread t, so that keys and positions leave coalesced.
__global__ void __launch_bounds__(SA_THREADS) k_sa_pack(const uint8_t *__restrict__ text, uint64_t n, uint64_t *__restrict__ keys, uint32_t *__restrict__ pos) {
    __shared__ uint32_t words[PACK_WORDS];
    const uint32_t t = threadIdx.x;
    const uint64_t tiles = (n + SA_TILE - 1) / SA_TILE;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t base = tile * SA_TILE, left = n - base;
        const uintptr_t addr = reinterpret_cast<uintptr_t>(text) + base;
        const uint32_t mis = static_cast<uint32_t>(addr & 3u);
        const uint32_t *const src = reinterpret_cast<const uint32_t *>(addr - mis);
        const uint32_t span = left < SA_TILE + 8 ? static_cast<uint32_t>(left) : SA_TILE + 8;   // bytes of the text from `base` on that a window may touch
        const uint32_t have = (mis + span + 3) / 4;                                                // words that hold one of them (<= 259)
        for (uint32_t w = t; w < PACK_WORDS; w += SA_THREADS) words[w] = w < have ? src[w] : 0u;
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < SA_PER; j++) {
            const uint32_t local = j * SA_THREADS + t;
            const uint64_t i = base + local;
            if (i < n) {
                const uint32_t off = mis + local, w = off / 4, shift = off & 3u;                 // w + 2 <= (3 + 1023) / 4 + 2 = 258
                const uint32_t lo = __builtin_amdgcn_alignbyte(words[w + 1], words[w], shift), hi = __builtin_amdgcn_alignbyte(words[w + 2], words[w + 1], shift);
                const uint64_t rest = n - i;
                keys[i] = sa_first_key(lo, hi, rest < SA_KEY_BYTES ? static_cast<uint32_t>(rest) : SA_KEY_BYTES);
                pos[i] = static_cast<uint32_t>(i);
            }
        }
        __syncthreads();
    }
}

// The place in `sa` of entry c of the active set (round 0: the set is everything, in place)
__device__ __forceinline__ uint32_t slot_of(const uint32_t *slot, uint64_t c) { return slot ? slot[c] : static_cast<uint32_t>(c); }

// Group boundaries behind a sort: dense[c] = place + 1 where the key differs from the one in front (a new group, or a new part of a group
// that the second rank has split), else 0.  The max-scan over it gives every entry the rank of its group: places ascend with c.
__global__ void __launch_bounds__(SA_THREADS) k_sa_heads(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ slot, uint64_t m, uint32_t *__restrict__ dense) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * SA_THREADS;
    for (uint64_t c = blockIdx.x * static_cast<uint64_t>(SA_THREADS) + threadIdx.x; c < m; c += stride) {
        const bool head = c == 0 || keys[c] != keys[c - 1];
        dense[c] = head ? slot_of(slot, c) + 1u : 0u;
    }
}

// The scatter back: rank of the suffix, the suffix at its place, and whether it stays active -- unless it is a group of its own (its
// rank is its place + 1 and the next entry starts a group as well)
__global__ void __launch_bounds__(SA_THREADS) k_sa_scatter(const uint32_t *__restrict__ pos, const uint32_t *__restrict__ slot, const uint32_t *__restrict__ dense, uint64_t m,
                                                          uint32_t *__restrict__ rank, uint32_t *__restrict__ sa, uint8_t *__restrict__ flag) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * SA_THREADS;
    for (uint64_t c = blockIdx.x * static_cast<uint64_t>(SA_THREADS) + threadIdx.x; c < m; c += stride) {
        const uint32_t r = dense[c], place = slot_of(slot, c), p = pos[c];
        const bool next_heads = c + 1 == m || dense[c + 1] == slot_of(slot, c + 1) + 1u;
        rank[p] = r;
        sa[place] = p;
        flag[c] = (r == place + 1u && next_heads) ? 0 : 1;
    }
}

// The active set of the next round from the selected entries of this one: suffix, place, and the key (rank of the group, rank h positions on)
__global__ void __launch_bounds__(SA_THREADS) k_sa_next(const uint32_t *__restrict__ picked, uint64_t m, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ slot,
                                                       const uint32_t *__restrict__ dense, const uint32_t *__restrict__ rank, uint64_t n, uint64_t h, uint32_t rank_bits,
                                                       uint64_t *__restrict__ keys_out, uint32_t *__restrict__ pos_out, uint32_t *__restrict__ slot_out) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * SA_THREADS;
    for (uint64_t k = blockIdx.x * static_cast<uint64_t>(SA_THREADS) + threadIdx.x; k < m; k += stride) {
        const uint32_t c = picked[k], p = pos[c];
        keys_out[k] = sa_round_key(dense[c], sa_second_rank(rank, n, p, h), rank_bits);
        pos_out[k] = p;
        slot_out[k] = slot_of(slot, c);
    }
}

// See the top of the file.  Entries base + 4 t .. + 3 of a tile are thread t's: one 16-byte load of sa, four gathered bytes of the text,
// four u64 stores and one word of BWT (bytes where out_bwt is not aligned, and in the last tile).  tile[1 + t]: its bytes; tile[0]'s top
// byte: the BWT byte in front of the tile.
__global__ void __launch_bounds__(SA_THREADS) k_sa_output(const uint32_t *__restrict__ sa, const uint8_t *__restrict__ text, uint64_t n, uint32_t sentinel,
                                                         uint64_t *__restrict__ out_sa, uint8_t *__restrict__ out_bwt, unsigned long long *runs_out) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    __shared__ uint32_t tile[SA_THREADS + 1];
    __shared__ uint32_t wave_runs[SA_THREADS / 64];
    const uint32_t t = threadIdx.x;
    const uint64_t tiles = (n + SA_TILE - 1) / SA_TILE, share = (tiles + gridDim.x - 1) / gridDim.x;
    const uint64_t first = blockIdx.x * share, end = first + share < tiles ? first + share : tiles;
    if (first >= end) return;
    const bool words_fit = out_bwt != nullptr && (reinterpret_cast<uintptr_t>(out_bwt) & 3u) == 0;
    uint32_t runs = 0;
    if (t == 0) {
        uint32_t front = 0;                          // (entry 0 starts a run whatever stands here)
        if (first != 0) { const uint32_t p = sa[first * SA_TILE - 1]; front = p ? text[p - 1] : sentinel; }
        tile[0] = front << 24;
    }
    for (uint64_t tl = first; tl < end; tl++) {
        const uint64_t at = tl * SA_TILE + SA_PER * t;
        const bool whole = at + SA_PER <= n;
        uint32_t p[SA_PER], b[SA_PER];
        if (whole) {
            const u32x4 v = *reinterpret_cast<const u32x4 *>(sa + at);
            p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < SA_PER; j++) p[j] = at + j < n ? sa[at + j] : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < SA_PER; j++) b[j] = at + j < n ? (p[j] ? text[p[j] - 1] : sentinel) : 0u;
        const uint32_t word = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        tile[1 + t] = word;
#pragma unroll
        for (uint32_t j = 0; j < SA_PER; j++)
            if (at + j < n) __builtin_nontemporal_store(static_cast<uint64_t>(p[j]), out_sa + at + j);
        if (out_bwt) {
            if (whole && words_fit) {
                __builtin_nontemporal_store(word, reinterpret_cast<uint32_t *>(out_bwt + at));
            } else {
#pragma unroll
                for (uint32_t j = 0; j < SA_PER; j++)
                    if (at + j < n) out_bwt[at + j] = static_cast<uint8_t>(b[j]);
            }
        }
        __syncthreads();
        uint32_t prev = tile[t] >> 24;               // the last byte of the thread in front, or of the tile in front
#pragma unroll
        for (uint32_t j = 0; j < SA_PER; j++) {
            if (at + j < n) runs += (at + j == 0 || b[j] != prev) ? 1u : 0u;
            prev = b[j];
        }
        const uint32_t carry = tile[SA_THREADS];
        __syncthreads();
        if (t == 0) tile[0] = carry;
    }
    for (int d = 32; d > 0; d >>= 1) runs += __shfl_down(runs, d, 64);
    if (t % 64 == 0) wave_runs[t / 64] = runs;
    __syncthreads();
    if (t == 0) {
        uint32_t r = 0;
        for (uint32_t w = 0; w < SA_THREADS / 64; w++) r += wave_runs[w];
        if (r) atomicAdd(runs_out, static_cast<unsigned long long>(r));
    }
}

// The temporary storage of the library calls of a round over m entries: the sort of `bits` key bits, the max-scan, the select
size_t round_temp_bytes(uint64_t m, uint32_t bits) {
    size_t sort = 0, scan = 0, select = 0;
    hipcub::DoubleBuffer<uint64_t> keys(nullptr, nullptr);
    hipcub::DoubleBuffer<uint32_t> suffixes(nullptr, nullptr);
    HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sort, keys, suffixes, static_cast<size_t>(m), 0, static_cast<int>(bits)));
    HIP_CHECK(hipcub::DeviceScan::InclusiveScan(nullptr, scan, static_cast<const uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr), hipcub::Max(), static_cast<size_t>(m)));
    HIP_CHECK(hipcub::DeviceSelect::Flagged(nullptr, select, hipcub::CountingInputIterator<uint32_t>(0), static_cast<const uint8_t *>(nullptr), static_cast<uint32_t *>(nullptr),
                                            static_cast<uint64_t *>(nullptr), static_cast<int64_t>(m)));
    return std::max(sort, std::max(scan, select));
}

}  // namespace

namespace gbwt_hip {

gbwt_hip_status build_suffix_array(const uint8_t *d_text, uint64_t n, uint8_t sentinel, uint64_t *d_sa, uint8_t *d_bwt, SaContext &ctx, hipStream_t s,
                                   gbwt_hip_suffix_array_info &info) {
    info = gbwt_hip_suffix_array_info{};
    info.n = n;
    if (n > SA_MAX_TEXT) return fail(GBWT_HIP_UNSUPPORTED, sa_plan(n, 0, 0).message);
    if (n == 0) return GBWT_HIP_OK;
    const uint32_t rank_bits = sa_rank_bits(n);
    size_t free_bytes = 0, all_bytes = 0;
    HIP_CHECK(hipMemGetInfo(&free_bytes, &all_bytes));
    const SaPlan plan = sa_plan(n, std::max(round_temp_bytes(n, 64), round_temp_bytes(n, 2 * rank_bits)), free_bytes);
    if (plan.status == SaStatus::Capacity) return fail(GBWT_HIP_CAPACITY, plan.message);
    info.rank_bits = plan.rank_bits;
    info.planned_scratch_bytes = plan.peak_bytes;
    int device = 0, cus = 0;
    HIP_CHECK(hipGetDevice(&device));
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    const auto blocks = [](uint64_t items) { return dim3(static_cast<unsigned>(std::min<uint64_t>((items + SA_THREADS - 1) / SA_THREADS, MAX_BLOCKS))); };
    const uint64_t tiles = (n + SA_TILE - 1) / SA_TILE;
    const dim3 tile_blocks(static_cast<unsigned>(std::min<uint64_t>(tiles, 8ull * static_cast<unsigned>(std::max(cus, 1)))));

    CountedScratch sc;
    CountedBuf rank(sc, plan.rank_bytes), sa(sc, plan.sa_bytes), key_a(sc, plan.key_bytes), key_b(sc, plan.key_bytes), pos_a(sc, plan.pos_bytes), pos_b(sc, plan.pos_bytes);
    CountedBuf slot_a(sc, plan.slot_bytes), slot_b(sc, plan.slot_bytes), dense(sc, plan.dense_bytes), picked(sc, plan.picked_bytes), flag(sc, plan.flag_bytes);
    CountedBuf temp(sc, plan.temp_bytes), words(sc, plan.words_bytes);     // words[0]: the size of the active set, words[1]: the runs
    uint64_t *const d_words = words.as<uint64_t>();
    HIP_CHECK(hipMemsetAsync(d_words, 0, 2 * sizeof(uint64_t), s));
    HIP_CHECK(hipEventRecord(ctx.ev[1], s));
    hipLaunchKernelGGL(k_sa_pack, tile_blocks, dim3(SA_THREADS), 0, s, d_text, n, key_a.as<uint64_t>(), pos_a.as<uint32_t>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ctx.ev[2], s));

    // The two key and position buffers are the library's pair: a sort leaves its result in either, the other is free for the next keys
    hipcub::DoubleBuffer<uint64_t> keys(key_a.as<uint64_t>(), key_b.as<uint64_t>());
    hipcub::DoubleBuffer<uint32_t> suffixes(pos_a.as<uint32_t>(), pos_b.as<uint32_t>());
    uint64_t m = n, h = SA_KEY_BYTES;
    const uint32_t *slot = nullptr;
    uint32_t round = 0;
    for (;;) {
        const uint32_t bits = round == 0 ? plan.first_key_bits : plan.key_bits;
        size_t temp_bytes = round_temp_bytes(m, bits);
        if (temp_bytes > temp.bytes) temp.alloc(sc, temp_bytes);     // (the library asks for no more for fewer entries; counted if it ever does)
        HIP_CHECK(hipEventRecord(ctx.ev[5], s));
        HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(temp.ptr, temp_bytes, keys, suffixes, static_cast<size_t>(m), 0, static_cast<int>(bits), s));
        const uint32_t *const sorted = suffixes.Current();
        hipLaunchKernelGGL(k_sa_heads, blocks(m), dim3(SA_THREADS), 0, s, static_cast<const uint64_t *>(keys.Current()), slot, m, dense.as<uint32_t>());
        temp_bytes = temp.bytes;
        HIP_CHECK(hipcub::DeviceScan::InclusiveScan(temp.ptr, temp_bytes, dense.as<const uint32_t>(), dense.as<uint32_t>(), hipcub::Max(), static_cast<size_t>(m), s));
        hipLaunchKernelGGL(k_sa_scatter, blocks(m), dim3(SA_THREADS), 0, s, sorted, slot, dense.as<const uint32_t>(), m, rank.as<uint32_t>(), sa.as<uint32_t>(),
                           flag.as<uint8_t>());
        temp_bytes = temp.bytes;
        HIP_CHECK(hipcub::DeviceSelect::Flagged(temp.ptr, temp_bytes, hipcub::CountingInputIterator<uint32_t>(0), flag.as<const uint8_t>(), picked.as<uint32_t>(), d_words,
                                                static_cast<int64_t>(m), s));
        HIP_CHECK(hipMemcpyAsync(ctx.words.p, d_words, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipEventRecord(ctx.ev[6], s));
        HIP_CHECK(hipStreamSynchronize(s));          // the one wait of a round
        HIP_CHECK(hipGetLastError());
        const uint64_t active = ctx.words.p[0];
        if (round < SA_INFO_ROUNDS) {
            info.active[round] = active;
            HIP_CHECK(hipEventElapsedTime(&info.round_ms[round], ctx.ev[5], ctx.ev[6]));
        }
        if (active == 0) break;
        if (active > m || h >= n) return fail(GBWT_HIP_DEVICE_ERROR, "the ranking of the suffix array did not settle: " + std::to_string(active) + " suffixes tied at step " + std::to_string(h));
        uint32_t *const slot_next = slot == slot_a.as<uint32_t>() ? slot_b.as<uint32_t>() : slot_a.as<uint32_t>();
        hipLaunchKernelGGL(k_sa_next, blocks(active), dim3(SA_THREADS), 0, s, picked.as<const uint32_t>(), active, sorted, slot, dense.as<const uint32_t>(),
                           rank.as<const uint32_t>(), n, h, plan.rank_bits, keys.Alternate(), suffixes.Alternate(), slot_next);
        keys.selector ^= 1;                          // the next keys are the current ones
        suffixes.selector ^= 1;
        slot = slot_next;
        m = active;
        h *= 2;
        round++;
    }
    info.rounds = round;
    HIP_CHECK(hipEventRecord(ctx.ev[3], s));
    hipLaunchKernelGGL(k_sa_output, tile_blocks, dim3(SA_THREADS), 0, s, sa.as<const uint32_t>(), d_text, n, static_cast<uint32_t>(sentinel), d_sa, d_bwt,
                       reinterpret_cast<unsigned long long *>(d_words + 1));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(ctx.words.p + 1, d_words + 1, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipEventRecord(ctx.ev[4], s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    info.bwt_runs = ctx.words.p[1];
    HIP_CHECK(hipEventElapsedTime(&info.pack_ms, ctx.ev[1], ctx.ev[2]));
    HIP_CHECK(hipEventElapsedTime(&info.rank_ms, ctx.ev[2], ctx.ev[3]));
    HIP_CHECK(hipEventElapsedTime(&info.output_ms, ctx.ev[3], ctx.ev[4]));
    info.peak_scratch_bytes = sc.peak;
    return GBWT_HIP_OK;
}

}  // namespace gbwt_hip
