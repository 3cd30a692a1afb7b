// fm_seeds.hip -- the maximal exact matches of reads on the FM-index (include/gbwt_hip.h, "Seeds of reads"): the kernels of
// one request.  What a start, an anchor and a seed are is fm_seeds.hpp, shared with the host; the calls are capi_fm_seeds.hip.
//
// THE SEARCH is k_fm_count's chain -- two dependent ranks per backward step, each one line in the packed layout -- with one lane per END of
// a read instead of one per pattern: first the anchors (every K-th end, counted from the end of the read), then, behind a count and a
// scan over the anchors, the ends between two anchors whose starts differ.  Nothing but memory latency paces a lane, so the ends in
// flight are the throughput.  Neighbouring lanes hold neighbouring ends of one read: the lanes of a wave differ in length by K from one
// to the next, and a wave lasts as long as its longest lane; words[2] sums those, so that the idle share can be reported.  The items are
// STRAND-MAJOR -- all reads on the first strand, then all on the second -- so that a wave does not hold the long matches of the strand a
// read came from beside the short ones of its other strand.
//
// THE SEEDS: every end whose start is known has a position in one order (fm_seed_kernels.hpp); a flag where the seed rule holds, a scan of
// the flags, and the seeds go behind those in front of them: the rows of the reads, each with the seeds of its first strand and then
// those of its second, starts and ends ascending.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "fm_seed_kernels.hpp"

namespace gbwt_hip {

namespace {

constexpr unsigned THREADS = 256;

// The read of item q, or an empty one where its offsets are no good
struct SeedRead { const uint8_t *bytes; uint32_t len, strand; bool bad; };

__device__ __forceinline__ SeedRead read_of(const SeedBatch &b, uint64_t q) {
    const uint64_t r = q % b.m;
    const uint64_t from = b.offsets[r], to = b.offsets[r + 1];
    SeedRead read{nullptr, 0, fm_strand_at(b.strands, static_cast<uint32_t>(q / b.m)), false};
    if (to < from || to > b.total_bytes || to - from > 0xFFFFFFFFull) { read.bad = true; return read; }
    read.bytes = b.bytes + from;
    read.len = static_cast<uint32_t>(to - from);
    return read;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int d = WAVE / 2; d > 0; d >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(v, d, WAVE)));
    return v;
}

// The steps of the block's lanes and the longest lane of each of its waves into words[1], words[2]; every lane of the block calls it
__device__ __forceinline__ void add_steps(uint32_t steps, uint64_t *words) {
    __shared__ unsigned long long block_steps, block_longest;
    if (threadIdx.x == 0) { block_steps = 0; block_longest = 0; }
    __syncthreads();
    const uint32_t longest = wave_max(steps);
    if (steps) atomicAdd(&block_steps, static_cast<unsigned long long>(steps));
    if (threadIdx.x % WAVE == 0 && longest) atomicAdd(&block_longest, static_cast<unsigned long long>(longest));
    __syncthreads();
    if (threadIdx.x == 0 && block_longest) {
        atomicAdd(reinterpret_cast<unsigned long long *>(words + 1), block_steps);
        atomicAdd(reinterpret_cast<unsigned long long *>(words + 2), block_longest);
    }
}

__global__ void __launch_bounds__(THREADS) k_seed_anchor_count(SeedBatch b) {
    const uint64_t q = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (q >= b.items) return;
    const SeedRead read = read_of(b, q);
    if (read.bad) atomicOr(reinterpret_cast<uint32_t *>(b.words), FM_FLAG_OFFSETS);
    b.anchor_counts[q] = fm_anchor_count(read.len);
}

__global__ void __launch_bounds__(THREADS) k_seed_anchors(SeedBatch b) {
    const uint64_t g = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    uint32_t steps = 0;
    if (g < b.anchors) {
        const uint64_t q = last_at_or_before(b.anchor_offsets, b.items, g);
        const SeedRead read = read_of(b, q);
        const uint32_t e = fm_anchor_end(read.len, static_cast<uint32_t>(g - b.anchor_offsets[q]));
        uint32_t start = 0;
        uint64_t lo = 0, hi = 0;
        steps = fm_longest_suffix(b.L, b.t.code, b.t.C, read.bytes, e, read.strand, read.len, start, lo, hi);
        b.anchor_start[g] = start;
        b.anchor_lo[g] = static_cast<uint32_t>(lo);
        b.anchor_hi[g] = static_cast<uint32_t>(hi);
        b.anchor_item[g] = static_cast<uint32_t>(q);
    }
    add_steps(steps, b.words);
}

// Anchor g as the kernels behind the search see it: its item's read, its end, and the end and start in front of it
struct SeedAnchor { SeedRead read; uint32_t end, end_before, start_before; };

__device__ __forceinline__ SeedAnchor anchor_of(const SeedBatch &b, uint64_t g) {
    const uint64_t q = b.anchor_item[g];
    SeedAnchor a;
    a.read = read_of(b, q);
    const uint32_t rank = static_cast<uint32_t>(g - b.anchor_offsets[q]);
    a.end = fm_anchor_end(a.read.len, rank);
    a.end_before = fm_anchor_before(a.read.len, rank);
    a.start_before = rank == 0 ? 0 : b.anchor_start[g - 1];
    return a;
}

__global__ void __launch_bounds__(THREADS) k_seed_refine_count(SeedBatch b) {
    const uint64_t g = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (g >= b.anchors) return;
    const SeedAnchor a = anchor_of(b, g);
    b.refined_counts[g] = fm_refined_ends(a.end_before, a.start_before, a.end, b.anchor_start[g]);
}

__global__ void __launch_bounds__(THREADS) k_seed_refine(SeedBatch b) {
    const uint64_t j = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    uint32_t steps = 0;
    if (j < b.refined) {
        const uint64_t g = last_at_or_before(b.refined_offsets, b.anchors, j);
        const SeedAnchor a = anchor_of(b, g);
        const uint32_t e = a.end_before + 1 + static_cast<uint32_t>(j - b.refined_offsets[g]);
        uint32_t start = 0;
        uint64_t lo = 0, hi = 0;
        steps = fm_longest_suffix(b.L, b.t.code, b.t.C, a.read.bytes, e, a.read.strand, a.read.len, start, lo, hi);
        b.refined_start[j] = start;
        b.refined_lo[j] = static_cast<uint32_t>(lo);
        b.refined_hi[j] = static_cast<uint32_t>(hi);
    }
    add_steps(steps, b.words);
}

// One end whose start is known -- lane i < anchors: anchor i; behind them: refined end i - anchors -- with its place in the order of the
// ends and the start of the end behind it
struct SeedEnd { uint64_t position, item; uint32_t start, end, lo, hi, len, strand; bool seed; };

__device__ __forceinline__ SeedEnd end_of(const SeedBatch &b, uint64_t i) {
    SeedEnd x;
    uint32_t next_start = 0;
    if (i < b.anchors) {
        const uint64_t g = i;
        const SeedAnchor a = anchor_of(b, g);
        x.position = g + b.refined_offsets[g + 1];
        x.item = b.anchor_item[g];
        x.start = b.anchor_start[g]; x.end = a.end; x.lo = b.anchor_lo[g]; x.hi = b.anchor_hi[g]; x.len = a.read.len; x.strand = a.read.strand;
        if (x.end != x.len) {
            // the next anchor is this read's: where its start is the same, so is the start of the end behind this one
            const uint64_t ahead = b.refined_offsets[g + 2] - b.refined_offsets[g + 1];
            next_start = ahead != 0 ? b.refined_start[b.refined_offsets[g + 1]] : b.anchor_start[g + 1];
        }
    } else {
        const uint64_t j = i - b.anchors;
        const uint64_t g = last_at_or_before(b.refined_offsets, b.anchors, j);
        const SeedAnchor a = anchor_of(b, g);
        x.position = g + j;
        x.item = b.anchor_item[g];
        x.start = b.refined_start[j]; x.end = a.end_before + 1 + static_cast<uint32_t>(j - b.refined_offsets[g]); x.lo = b.refined_lo[j]; x.hi = b.refined_hi[j];
        x.len = a.read.len; x.strand = a.read.strand;
        next_start = j + 1 < b.refined_offsets[g + 1] ? b.refined_start[j + 1] : b.anchor_start[g];
    }
    x.seed = fm_is_seed(x.start, x.end, x.len, next_start, b.min_length);
    return x;
}

// The seeds in front of item q (q == items: all of them): the rank of the first end of the item
__device__ __forceinline__ uint64_t seeds_before_item(const SeedBatch &b, uint64_t q) {
    const uint64_t g = b.anchor_offsets[q];
    return b.rank[g + b.refined_offsets[g]];
}

// The seeds in the rows of the reads in front of read r (r == m: all of them): those of their first strand and of their second
__device__ __forceinline__ uint64_t seeds_before_read(const SeedBatch &b, uint64_t r) {
    const uint64_t first = seeds_before_item(b, r);
    return fm_strand_count(b.strands) == 1 ? first : first + seeds_before_item(b, b.m + r) - seeds_before_item(b, b.m);
}

__global__ void __launch_bounds__(THREADS) k_seed_flags(SeedBatch b) {
    const uint64_t i = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (i >= b.anchors + b.refined) return;
    const SeedEnd x = end_of(b, i);
    b.flags[x.position] = x.seed ? 1 : 0;
}

__global__ void __launch_bounds__(THREADS) k_seed_fill(SeedBatch b, gbwt_hip_fm_seed *__restrict__ seeds, uint64_t *__restrict__ read_offsets, uint64_t max_occurrences,
                                                       uint64_t *__restrict__ hit_ranges, uint64_t *__restrict__ hit_counts) {
    const uint64_t i = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (i <= b.m) read_offsets[i] = seeds_before_read(b, i);
    if (i >= b.anchors + b.refined) return;
    const SeedEnd x = end_of(b, i);
    if (!x.seed) return;
    // behind the seeds of the reads in front, and behind the forward seeds of this read where this is its second strand
    const uint64_t r = x.item % b.m;
    const uint64_t at = seeds_before_read(b, r) + (x.item >= b.m ? seeds_before_item(b, r + 1) - seeds_before_item(b, r) : 0) + (b.rank[x.position] - seeds_before_item(b, x.item));
    seeds[at] = gbwt_hip_fm_seed{x.lo, x.hi, x.start, x.end, x.strand, 0};
    if (!hit_ranges) return;
    const uint64_t count = uint64_t(x.hi) - x.lo;
    const bool kept = count <= max_occurrences;
    if (!kept) atomicAdd(reinterpret_cast<unsigned long long *>(b.words + 3), 1ull);
    hit_ranges[2 * at] = x.lo;
    hit_ranges[2 * at + 1] = kept ? x.hi : x.lo;
    hit_counts[at] = kept ? count : 0;
}

}  // namespace

void launch_seed_anchor_count(const SeedBatch &b, hipStream_t s) {
    if (b.items) hipLaunchKernelGGL(k_seed_anchor_count, blocks_for(b.items), dim3(THREADS), 0, s, b);
}

void launch_seed_anchors(const SeedBatch &b, hipStream_t s) {
    if (b.anchors) hipLaunchKernelGGL(k_seed_anchors, blocks_for(b.anchors), dim3(THREADS), 0, s, b);
}

void launch_seed_refine_count(const SeedBatch &b, hipStream_t s) {
    if (b.anchors) hipLaunchKernelGGL(k_seed_refine_count, blocks_for(b.anchors), dim3(THREADS), 0, s, b);
}

void launch_seed_refine(const SeedBatch &b, hipStream_t s) {
    if (b.refined) hipLaunchKernelGGL(k_seed_refine, blocks_for(b.refined), dim3(THREADS), 0, s, b);
}

void launch_seed_flags(const SeedBatch &b, hipStream_t s) {
    if (b.anchors) hipLaunchKernelGGL(k_seed_flags, blocks_for(b.anchors + b.refined), dim3(THREADS), 0, s, b);
}

void launch_seed_fill(const SeedBatch &b, gbwt_hip_fm_seed *d_seeds, uint64_t *d_read_offsets, uint64_t max_occurrences, uint64_t *d_hit_ranges, uint64_t *d_hit_counts, hipStream_t s) {
    hipLaunchKernelGGL(k_seed_fill, blocks_for(std::max(b.anchors + b.refined, b.m + 1)), dim3(THREADS), 0, s, b, d_seeds, d_read_offsets, max_occurrences, d_hit_ranges, d_hit_counts);
}

}  // namespace gbwt_hip
