// fm_align.hip -- the alignments of chains (include/gbwt_hip.h, "Alignments of chains"): the kernels of the banded edit distance
// behind a chains request.  What a band, a cell and a direction are is fm_align.hpp, shared with the host; the calls are capi_fm_align.hip.
//
// SELECT and SETUP.  One lane per item counts the chains of its strand that are considered; behind the scan one lane per considered chain
// reads the members of its chain for the band, takes the bounds of its segment and says what it needs of the scratch.
//
// THE DP is the hot kernel: one wave per alignment, row by row.  A lane owns the diagonals k = lane, lane + 64, ..: ceil(W / 64) registers
// hold a row, and a template instance per 1, 2, 4, 8 and 16 of them keeps them registers.  The read byte of a row is the same in every
// lane (64 of them are loaded at a time and read back with v_readlane); the text byte of cell (i, k) is T[i - 1 + d0 + k], read from a
// window staged once in LDS where it fits.  The diagonal candidate is the lane's own register, the insertion its upper neighbour's: one
// lane shift, and lane 0 of the next chunk for lane 63.  The deletion chain of a row is a prefix minimum of A(k) - k: six shifts per
// chunk and a carry between chunks.  An anti-diagonal wavefront would need no scan, but it keeps two fronts in registers, reads a
// different read byte in every lane and scatters the directions of a row over W words; row by row the read byte is a scalar and two
// ballots are the packed directions of 64 cells, so the scan's six shifts are the cheaper price.  The directions go to an LDS tile of
// FM_ALIGN_TILE_BYTES per wave where L x ceil(W / 16) words fit, else to counted scratch in HBM; lane 0 walks them back in the same kernel.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_common.hpp"
#include "fm_align_kernels.hpp"
#include "fm_seeds.hpp"

namespace gbwt_hip {

namespace {

constexpr unsigned THREADS = 256;
constexpr unsigned DP_WAVES = 4, DP_THREADS = DP_WAVES * WAVE;
constexpr uint32_t TILE_WORDS = static_cast<uint32_t>(FM_ALIGN_TILE_BYTES / sizeof(uint32_t));
constexpr uint32_t TEXT_TILE = static_cast<uint32_t>(FM_ALIGN_TEXT_TILE);

__device__ __forceinline__ void count(uint64_t *word, uint64_t by = 1) { atomicAdd(reinterpret_cast<unsigned long long *>(word), static_cast<unsigned long long>(by)); }

__global__ void __launch_bounds__(THREADS) k_align_select(AlignBatch b) {
    const uint64_t q = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (q >= b.items) return;
    const uint64_t r = q / b.ns;
    uint64_t first = b.chain_read_offsets[r], last = b.chain_read_offsets[r + 1];
    if (b.ns == 2) {                                     // the first chain of the row on the reverse strand
        uint64_t lo = first, hi = last;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (b.chains[mid].strand < FM_STRAND_REVERSE) lo = mid + 1; else hi = mid;
        }
        if (q % b.ns == 0) last = lo; else first = lo;
    }
    uint64_t considered = last - first;
    if (b.max_alignments != 0 && considered > b.max_alignments) considered = b.max_alignments;
    b.item_counts[q] = considered;
    b.item_first[q] = first;
}

__global__ void __launch_bounds__(THREADS) k_align_setup(AlignBatch b) {
    const uint64_t a = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (a >= b.alignments) return;
    const uint64_t q = last_at_or_before(b.item_offsets, b.items, a);
    const uint64_t c = b.item_first[q] + (a - b.item_offsets[q]);
    const gbwt_hip_fm_chain chain = b.chains[c];
    const uint64_t r = q / b.ns;
    int64_t dmin = 0, dmax = 0;
    const uint64_t from = b.chain_match_offsets[c], to = b.chain_match_offsets[c + 1];
    for (uint64_t t = from; t < to; t++) {
        const int64_t d = fm_align_diagonal(b.matches[t].y, b.matches[t].x);
        if (t == from || d < dmin) dmin = d;
        if (t == from || d > dmax) dmax = d;
    }
    FmAlignTask task{};
    task.d0 = fm_align_d0(dmin, b.band);
    const uint64_t width = fm_align_width(dmin, dmax, b.band);
    task.W = width > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(width);
    task.lo = b.path_offsets ? b.path_offsets[chain.path] : 0;
    task.hi = b.path_offsets ? b.path_offsets[chain.path + 1] - 1 : b.n;
    task.read_first = b.q_offsets[r];
    const uint64_t L = b.q_offsets[r + 1] - task.read_first;
    task.L = static_cast<uint32_t>(L);
    task.chain = static_cast<uint32_t>(c);
    task.strand = chain.strand;
    task.path = chain.path;
    task.status = width > b.max_width ? GBWT_HIP_ALIGN_WIDE : GBWT_HIP_ALIGN_OK;
    task.edit_distance = FM_ALIGN_INF;
    const bool computed = task.status == GBWT_HIP_ALIGN_OK;
    if (computed && L > FM_ALIGN_MAX_READ) count(b.words + 6);
    b.tasks[a] = task;
    b.direction_words[a] = computed && !fm_align_in_tile(L, width) ? L * fm_align_row_words(task.W) : 0;
    b.cigar_bound[a] = computed ? fm_align_cigar_bound(L) : 0;
    b.cigar_count[a] = 0;
}

__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t lane) {           // lane: the same in every lane of the wave
    return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), static_cast<int>(lane)));
}

// What the lanes of the wave have written, to LDS or to HBM, every lane may read behind this
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

__device__ __forceinline__ uint64_t wave_min64(uint64_t v, uint32_t lane) {
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        const uint64_t other = shfl64(v, static_cast<int>(lane ^ d));
        v = other < v ? other : v;
    }
    return v;
}

// The rows 1 .. L of one alignment over N chunks of 64 diagonals: the directions of every row into `directions`, and the key of the
// smallest H of row L with its smallest k.  window: the text from position `window_first` on; read: the bytes of the read as given.
template <int N>
__device__ __forceinline__ uint64_t dp_rows(const FmAlignTask &task, const uint8_t *read, const uint8_t *window, int64_t window_first, uint32_t *directions, uint32_t lane) {
    const uint32_t L = task.L, W = task.W, words = fm_align_row_words(W);
    uint32_t h[N];
    int32_t first = 0, last = -1;
    fm_align_row_range(task.d0, W, task.lo, task.hi, 0, first, last);
#pragma unroll
    for (int c = 0; c < N; c++) {
        const int32_t k = c * WAVE + static_cast<int32_t>(lane);
        h[c] = k >= first && k <= last ? 0u : FM_ALIGN_INF;
    }
    for (uint32_t i0 = 0; i0 < L; i0 += WAVE) {
        const uint32_t mine = i0 + lane;
        const uint32_t my_byte = mine < L ? fm_strand_byte(read, L, task.strand, mine) : 0u;
        const uint32_t rows = L - i0 < static_cast<uint32_t>(WAVE) ? L - i0 : static_cast<uint32_t>(WAVE);
        for (uint32_t ii = 0; ii < rows; ii++) {
            const uint32_t i = i0 + ii + 1;
            const uint32_t p = lane_value(my_byte, ii);
            fm_align_row_range(task.d0, W, task.lo, task.hi, i, first, last);
            const int64_t text_base = task.d0 + static_cast<int64_t>(i) - 1 - window_first;      // T[j - 1] of k == 0, in the window
            uint32_t *row = directions + static_cast<uint64_t>(i - 1) * words;
            uint32_t carry = FM_ALIGN_INF;
#pragma unroll
            for (int c = 0; c < N; c++) {
                const int32_t k = c * WAVE + static_cast<int32_t>(lane);
                const bool exists = k >= first && k <= last;
                const uint32_t diagonal = h[c];
                uint32_t above = static_cast<uint32_t>(__shfl_down(static_cast<int>(diagonal), 1, WAVE));
                const uint32_t next_chunk = c + 1 < N ? lane_value(h[c + 1 < N ? c + 1 : c], 0) : FM_ALIGN_INF;
                if (lane == WAVE - 1) above = next_chunk;
                const uint32_t t = exists && diagonal != FM_ALIGN_INF ? window[text_base + k] : 0u;
                uint32_t direction = FM_ALIGN_DIAGONAL;
                const uint32_t a = exists ? fm_align_cell(diagonal, p != t, above, direction) : FM_ALIGN_INF;
                uint32_t v = fm_align_skew(a, static_cast<uint32_t>(k));
#pragma unroll
                for (int d = 1; d < WAVE; d <<= 1) {
                    const uint32_t other = static_cast<uint32_t>(__shfl_up(static_cast<int>(v), d, WAVE));
                    if (lane >= static_cast<uint32_t>(d) && other < v) v = other;
                }
                if (carry < v) v = carry;
                carry = lane_value(v, WAVE - 1);
                const uint32_t value = exists ? fm_align_unskew(v, static_cast<uint32_t>(k)) : FM_ALIGN_INF;
                if (value < a) direction = FM_ALIGN_DELETION;
                h[c] = value;
                const uint64_t low_bits = __ballot((direction & 1u) != 0), high_bits = __ballot((direction & 2u) != 0);
                const uint32_t word = 4 * c + lane;
                if (lane < 4 && word < words) row[word] = fm_align_direction_word(low_bits, high_bits, lane);
            }
        }
    }
    uint64_t key = ~uint64_t(0);
#pragma unroll
    for (int c = 0; c < N; c++) {
        const uint64_t mine = fm_align_end_key(h[c], static_cast<uint32_t>(c * WAVE) + lane);
        key = mine < key ? mine : key;
    }
    return wave_min64(key, lane);
}

__global__ void __launch_bounds__(DP_THREADS) k_align_dp(AlignBatch b) {
    __shared__ uint32_t tile[DP_WAVES][TILE_WORDS];
    __shared__ uint8_t staged[DP_WAVES][TEXT_TILE];
    const uint32_t wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const uint64_t a = uint64_t(blockIdx.x) * DP_WAVES + wave;
    if (a >= b.alignments) return;                       // (no barrier of the workgroup below: a wave is on its own)
    FmAlignTask task = b.tasks[a];
    if (task.status != GBWT_HIP_ALIGN_OK) {
        if (lane == 0) count(b.words + 1);
        return;
    }
    if (task.L > FM_ALIGN_MAX_READ) return;              // (the request is refused: words[6])
    const uint32_t L = task.L, W = task.W;
    const bool in_tile = fm_align_in_tile(L, W);
    uint32_t *directions = in_tile ? tile[wave] : b.directions + b.direction_offsets[a];
    // the text the cells read: T[j - 1] for j - 1 in [max(lo, d0), min(hi, d0 + L + W - 1))
    const int64_t reach = task.d0 + static_cast<int64_t>(L) + static_cast<int64_t>(W) - 1;
    const int64_t window_first = task.d0 > static_cast<int64_t>(task.lo) ? task.d0 : static_cast<int64_t>(task.lo);
    const int64_t window_last = reach < static_cast<int64_t>(task.hi) ? reach : static_cast<int64_t>(task.hi);
    const uint64_t window_bytes = window_last > window_first ? static_cast<uint64_t>(window_last - window_first) : 0;
    const uint8_t *window = b.text + window_first;       // (read only where a cell exists: inside [lo, hi))
    if (window_bytes <= TEXT_TILE) {
        for (uint32_t t = lane; t < window_bytes; t += WAVE) staged[wave][t] = window[t];
        window = staged[wave];
        wave_fence();
    }
    const uint8_t *read = b.q_bytes + task.read_first;
    const uint32_t chunks = (W + WAVE - 1) / WAVE;
    uint64_t key;
    if (chunks <= 1) key = dp_rows<1>(task, read, window, window_first, directions, lane);
    else if (chunks <= 2) key = dp_rows<2>(task, read, window, window_first, directions, lane);
    else if (chunks <= 4) key = dp_rows<4>(task, read, window, window_first, directions, lane);
    else if (chunks <= 8) key = dp_rows<8>(task, read, window, window_first, directions, lane);
    else key = dp_rows<16>(task, read, window, window_first, directions, lane);
    wave_fence();
    if (lane != 0) return;
    const uint32_t distance = static_cast<uint32_t>(key >> 32), k_end = static_cast<uint32_t>(key);
    count(b.words + 0);
    count(b.words + 3, (static_cast<uint64_t>(L) + 1) * W);
    count(b.words + (in_tile ? 4 : 5));
    if (distance == FM_ALIGN_INF) {
        count(b.words + 2);
        b.tasks[a].status = GBWT_HIP_ALIGN_NONE;
        return;
    }
    uint32_t k_start = 0;
    const uint32_t bound = static_cast<uint32_t>(fm_align_cigar_bound(L));
    const uint32_t strand = task.strand;
    const uint32_t entries = fm_align_trace(L, W, task.d0, k_end, directions, [=](uint32_t i) { return fm_strand_byte(read, L, strand, i); },
                                            [=](uint64_t j) { return window[static_cast<int64_t>(j) - window_first]; }, b.cigar_scratch + b.cigar_first[a], bound, k_start);
    b.cigar_count[a] = entries;
    b.tasks[a].edit_distance = distance;
    b.tasks[a].text_start = static_cast<uint64_t>(task.d0 + static_cast<int64_t>(k_start));
    b.tasks[a].text_end = static_cast<uint64_t>(task.d0 + static_cast<int64_t>(L) + static_cast<int64_t>(k_end));
}

__global__ void __launch_bounds__(THREADS) k_align_rows(AlignBatch b, uint64_t *__restrict__ read_offsets, gbwt_hip_fm_alignment *__restrict__ alignments,
                                                        const uint64_t *__restrict__ cigar_offsets, uint32_t *__restrict__ cigars) {
    const uint64_t g = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (g <= b.m) read_offsets[g] = b.item_offsets[g * b.ns < b.items ? g * b.ns : b.items];
    if (g >= b.alignments) return;
    const FmAlignTask task = b.tasks[g];
    const bool ok = task.status == GBWT_HIP_ALIGN_OK;
    alignments[g] = gbwt_hip_fm_alignment{ok ? task.text_start : 0, ok ? task.text_end : 0, task.chain, ok ? task.edit_distance : FM_ALIGN_INF, task.W, task.status, task.strand, task.path};
    const uint64_t entries = b.cigar_count[g];
    const uint32_t *from = b.cigar_scratch + b.cigar_first[g] + (b.cigar_bound[g] - entries);
    for (uint64_t e = 0; e < entries; e++) cigars[cigar_offsets[g] + e] = from[e];
}

}  // namespace

void launch_align_select(const AlignBatch &b, hipStream_t s) {
    if (b.items) hipLaunchKernelGGL(k_align_select, blocks_for(b.items), dim3(THREADS), 0, s, b);
}

void launch_align_setup(const AlignBatch &b, hipStream_t s) {
    if (b.alignments) hipLaunchKernelGGL(k_align_setup, blocks_for(b.alignments), dim3(THREADS), 0, s, b);
}

void launch_align_dp(const AlignBatch &b, hipStream_t s) {
    if (b.alignments) hipLaunchKernelGGL(k_align_dp, grid_for(b.alignments, DP_WAVES), dim3(DP_THREADS), 0, s, b);
}

void launch_align_rows(const AlignBatch &b, uint64_t *d_read_offsets, gbwt_hip_fm_alignment *d_alignments, const uint64_t *d_cigar_offsets, uint32_t *d_cigars, hipStream_t s) {
    hipLaunchKernelGGL(k_align_rows, blocks_for(std::max(b.alignments, b.m + 1)), dim3(THREADS), 0, s, b, d_read_offsets, d_alignments, d_cigar_offsets, d_cigars);
}

}  // namespace gbwt_hip
