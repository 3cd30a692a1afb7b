// fm_index.hip -- the FM-index over a text on the device (include/gbwt_hip.h, "FM-index over a text"): the kernels that
// build it from a text and its suffix array, and the batched queries -- backward search, one lane per pattern, and the rows of located
// positions.  What a block, a rank and a step are is fm_layout.hpp, shared with the host; the calls are capi_fm.hip.
//
// THE BUILD, behind the suffix array: a byte histogram (the host turns its 256 numbers into the code table and C); the code of every
// row's BWT byte, T[SA[row - 1] - 1], gathered straight into its place in the blocks; the occurrences of every code in every block; their
// exclusive sums across the blocks, code by code; the sums into the heads of the lines (packed) or the counts beside them (plain); and
// the suffix array narrowed to u32.
//
// A QUERY is a chain of dependent ranks: 2 per step, each one line (packed).  Nothing but memory latency paces a lane, so the batch is the
// parallelism: one lane per pattern, lanes of a wave at different lengths, a lane out as soon as its range is empty.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "device_common.hpp"
#include "fm_index.hpp"
#include "scan.hpp"

namespace gbwt_hip {

namespace {

constexpr unsigned THREADS = 256;
constexpr unsigned WAVE = 64;


__global__ void __launch_bounds__(THREADS) k_fm_histogram(const uint8_t *__restrict__ text, uint64_t n, uint64_t *__restrict__ hist) {
    __shared__ uint32_t bins[256];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t stride = uint64_t(gridDim.x) * THREADS;
    for (uint64_t i = uint64_t(blockIdx.x) * THREADS + threadIdx.x; i < n; i += stride) atomicAdd(&bins[text[i]], 1u);
    __syncthreads();
    if (bins[threadIdx.x]) atomicAdd(reinterpret_cast<unsigned long long *>(hist + threadIdx.x), static_cast<unsigned long long>(bins[threadIdx.x]));
}

// primary[0] = the row of suffix 0, primary[1] |= 1 for a suffix array value outside the text
__global__ void __launch_bounds__(THREADS) k_fm_codes(const uint8_t *__restrict__ text, const uint64_t *__restrict__ sa, uint64_t n, const uint16_t *__restrict__ code, bool packed,
                                                      uint8_t *__restrict__ lines, uint64_t *__restrict__ primary) {
    const uint64_t row = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (row > n) return;
    uint8_t c = 0;
    if (row == 0) c = static_cast<uint8_t>(code[text[n - 1]]);
    else {
        const uint64_t p = sa[row - 1];
        if (p == 0) primary[0] = row;
        else if (p < n) c = static_cast<uint8_t>(code[text[p - 1]]);
        else primary[1] = 1;
    }
    lines[fm_code_at(row, packed)] = c;
}

__global__ void __launch_bounds__(THREADS) k_fm_block_counts_packed(const uint8_t *__restrict__ lines, uint64_t rows, uint64_t blocks, uint32_t sigma,
                                                                    const uint64_t *__restrict__ primary, uint32_t *__restrict__ out) {
    const uint64_t b = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (b >= blocks) return;
    FmLayout L;
    L.sigma = sigma; L.packed = 1; L.rows = rows; L.blocks = blocks; L.primary = primary[0]; L.lines = lines;
    const uint64_t first = b * FM_PACKED_BLOCK;
    const uint32_t k = first >= rows ? 0 : static_cast<uint32_t>(rows - first < FM_PACKED_BLOCK ? rows - first : FM_PACKED_BLOCK);
    for (uint32_t c = 0; c < sigma; c++) out[uint64_t(c) * blocks + b] = fm_count_in_block(L, b, k, c);
}

// one workgroup per block of 256 rows
__global__ void __launch_bounds__(FM_PLAIN_BLOCK) k_fm_block_counts_plain(const uint8_t *__restrict__ lines, uint64_t rows, uint64_t blocks, uint32_t sigma,
                                                                          const uint64_t *__restrict__ primary, uint32_t *__restrict__ out) {
    __shared__ uint32_t bins[256];
    const uint64_t b = blockIdx.x;
    bins[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t row = b * FM_PLAIN_BLOCK + threadIdx.x;
    if (row < rows && row != primary[0]) atomicAdd(&bins[lines[row]], 1u);
    __syncthreads();
    if (threadIdx.x < sigma) out[uint64_t(threadIdx.x) * blocks + b] = bins[threadIdx.x];
}

__global__ void __launch_bounds__(THREADS) k_fm_fill_packed(const uint32_t *__restrict__ scanned, uint64_t blocks, uint32_t sigma, uint8_t *__restrict__ lines) {
    const uint64_t i = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    const uint64_t b = i / FM_PACKED_SIGMA;
    const uint32_t c = static_cast<uint32_t>(i % FM_PACKED_SIGMA);
    if (b >= blocks) return;
    reinterpret_cast<uint32_t *>(lines + b * FM_LINE)[c] = c < sigma ? scanned[uint64_t(c) * blocks + b] - scanned[uint64_t(c) * blocks] : 0;
}

__global__ void __launch_bounds__(THREADS) k_fm_fill_plain(const uint32_t *__restrict__ scanned, uint64_t blocks, uint32_t sigma, uint32_t *__restrict__ counts) {
    const uint64_t i = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (i >= blocks * sigma) return;
    const uint64_t b = i / sigma;
    const uint32_t c = static_cast<uint32_t>(i % sigma);
    counts[i] = scanned[uint64_t(c) * blocks + b] - scanned[uint64_t(c) * blocks];
}

__global__ void __launch_bounds__(THREADS) k_fm_narrow_sa(const uint64_t *__restrict__ sa, uint64_t n, uint32_t *__restrict__ sa32) {
    const uint64_t i = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (i < n) sa32[i] = static_cast<uint32_t>(sa[i]);
}

__global__ void __launch_bounds__(THREADS) k_fm_count(FmLayout L, FmTables t, const uint64_t *__restrict__ offsets, const uint8_t *__restrict__ bytes, uint64_t m, uint64_t total_bytes,
                                                      uint64_t *__restrict__ ranges, uint64_t *__restrict__ counts, uint64_t *__restrict__ words) {
    __shared__ unsigned long long block_steps;
    if (threadIdx.x == 0) block_steps = 0;
    __syncthreads();
    const uint64_t k = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (k < m) {
        const uint64_t from = offsets[k], to = offsets[k + 1];
        uint64_t lo = 0, hi = 0;
        if (to < from || to > total_bytes) atomicOr(reinterpret_cast<uint32_t *>(words), FM_FLAG_OFFSETS);
        else {
            const uint64_t steps = fm_search(L, t.code, t.C, bytes + from, to - from, lo, hi);
            if (steps) atomicAdd(&block_steps, static_cast<unsigned long long>(steps));
        }
        ranges[2 * k] = lo;
        ranges[2 * k + 1] = hi;
        counts[k] = hi - lo;
    }
    __syncthreads();
    if (threadIdx.x == 0 && block_steps) atomicAdd(reinterpret_cast<unsigned long long *>(words + 1), block_steps);
}

// A wave takes 64 rows: a lane copies its own row where it is short, and the wave copies the long ones together, 64 positions at a time
__global__ void __launch_bounds__(THREADS) k_fm_locate_fill(const uint32_t *__restrict__ sa32, const uint64_t *__restrict__ ranges, const uint64_t *__restrict__ row_offsets, uint64_t m,
                                                            uint64_t *__restrict__ positions, uint32_t *__restrict__ rows) {
    const uint64_t k = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    const unsigned lane = threadIdx.x % WAVE;
    uint64_t lo = 0, count = 0, at = 0;
    if (k < m) { lo = ranges[2 * k]; count = ranges[2 * k + 1] - lo; at = row_offsets[k]; }
    if (count <= FM_SHORT_ROW) {
        for (uint64_t j = 0; j < count; j++) {
            positions[at + j] = sa32[lo + j];
            if (rows) rows[at + j] = static_cast<uint32_t>(k);
        }
    }
    unsigned long long longer = __ballot(count > FM_SHORT_ROW);
    while (longer) {
        const int owner = __ffsll(longer) - 1;
        longer &= longer - 1;
        const uint64_t row_lo = shfl64(lo, owner), row_count = shfl64(count, owner), row_at = shfl64(at, owner);
        const uint32_t row = static_cast<uint32_t>(k - lane + owner);
        for (uint64_t j = lane; j < row_count; j += WAVE) {
            positions[row_at + j] = sa32[row_lo + j];
            if (rows) rows[row_at + j] = row;
        }
    }
}

__global__ void __launch_bounds__(THREADS) k_fm_run_flags(const uint64_t *__restrict__ values, const uint32_t *__restrict__ rows, uint64_t total, uint64_t *__restrict__ flag) {
    const uint64_t i = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (i < total) flag[i] = (i == 0 || rows[i] != rows[i - 1] || values[i] != values[i - 1]) ? 1 : 0;
}

// rank[i] = kept values in front of item i (rank[total]: all of them)
__global__ void __launch_bounds__(THREADS) k_fm_compact(const uint64_t *__restrict__ values, const uint64_t *__restrict__ rank, uint64_t total, const uint64_t *__restrict__ row_offsets,
                                                        uint64_t m, uint64_t *__restrict__ out, uint64_t *__restrict__ new_offsets) {
    const uint64_t i = uint64_t(blockIdx.x) * THREADS + threadIdx.x;
    if (i < total && rank[i + 1] != rank[i]) out[rank[i]] = values[i];
    if (i <= m) new_offsets[i] = rank[row_offsets[i]];
}

}  // namespace

void launch_fm_histogram(const uint8_t *d_text, uint64_t n, uint64_t *d_hist, hipStream_t s) {
    if (n == 0) return;
    const unsigned grid = std::min<unsigned>(grid_for(n, THREADS), 4096);
    hipLaunchKernelGGL(k_fm_histogram, dim3(grid), dim3(THREADS), 0, s, d_text, n, d_hist);
}

void launch_fm_codes(const uint8_t *d_text, const uint64_t *d_sa, uint64_t n, const uint16_t *d_code, bool packed, uint8_t *d_lines, uint64_t *d_primary, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_fm_codes, blocks_for(n + 1), dim3(THREADS), 0, s, d_text, d_sa, n, d_code, packed, d_lines, d_primary);
}

void launch_fm_block_counts(const uint8_t *d_lines, uint64_t rows, uint64_t blocks, uint32_t sigma, bool packed, const uint64_t *d_primary, uint32_t *d_block_counts, hipStream_t s) {
    if (packed) hipLaunchKernelGGL(k_fm_block_counts_packed, blocks_for(blocks), dim3(THREADS), 0, s, d_lines, rows, blocks, sigma, d_primary, d_block_counts);
    else hipLaunchKernelGGL(k_fm_block_counts_plain, dim3(static_cast<unsigned>(blocks)), dim3(FM_PLAIN_BLOCK), 0, s, d_lines, rows, blocks, sigma, d_primary, d_block_counts);
}

namespace {
uint64_t codes_per_piece(uint64_t blocks) { return std::max<uint64_t>(1, SCAN_PIECE / blocks); }
}  // namespace

size_t fm_scan_temp_bytes(uint64_t blocks, uint32_t sigma) {
    size_t bytes = 0;
    const uint64_t items = std::min<uint64_t>(codes_per_piece(blocks), std::max<uint32_t>(sigma, 1)) * blocks;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, static_cast<const uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr), static_cast<int>(items));
    return std::max<size_t>(bytes, 16);
}

void launch_fm_scan(const uint32_t *d_block_counts, uint32_t *d_scanned, uint64_t blocks, uint32_t sigma, void *d_temp, size_t temp_bytes, hipStream_t s) {
    const uint64_t per = codes_per_piece(blocks);
    for (uint64_t c = 0; c < sigma; c += per) {
        const uint64_t items = std::min<uint64_t>(per, sigma - c) * blocks;
        (void)hipcub::DeviceScan::ExclusiveSum(d_temp, temp_bytes, d_block_counts + c * blocks, d_scanned + c * blocks, static_cast<int>(items), s);
    }
}

void launch_fm_fill(const uint32_t *d_scanned, uint64_t blocks, uint32_t sigma, bool packed, uint8_t *d_lines, uint32_t *d_counts, hipStream_t s) {
    if (packed) hipLaunchKernelGGL(k_fm_fill_packed, blocks_for(blocks * FM_PACKED_SIGMA), dim3(THREADS), 0, s, d_scanned, blocks, sigma, d_lines);
    else hipLaunchKernelGGL(k_fm_fill_plain, blocks_for(blocks * sigma), dim3(THREADS), 0, s, d_scanned, blocks, sigma, d_counts);
}

void launch_fm_narrow_sa(const uint64_t *d_sa, uint64_t n, uint32_t *d_sa32, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_fm_narrow_sa, blocks_for(n), dim3(THREADS), 0, s, d_sa, n, d_sa32);
}

void launch_fm_count(const FmLayout &L, const FmTables &t, const uint64_t *d_offsets, const uint8_t *d_bytes, uint64_t m, uint64_t bytes, uint64_t *d_ranges, uint64_t *d_counts,
                     uint64_t *d_words, hipStream_t s) {
    if (m) hipLaunchKernelGGL(k_fm_count, blocks_for(m), dim3(THREADS), 0, s, L, t, d_offsets, d_bytes, m, bytes, d_ranges, d_counts, d_words);
}

void launch_fm_locate_fill(const uint32_t *d_sa32, const uint64_t *d_ranges, const uint64_t *d_row_offsets, uint64_t m, uint64_t *d_positions, uint32_t *d_rows, hipStream_t s) {
    if (m) hipLaunchKernelGGL(k_fm_locate_fill, blocks_for(m), dim3(THREADS), 0, s, d_sa32, d_ranges, d_row_offsets, m, d_positions, d_rows);
}

size_t fm_sort_temp_bytes(uint64_t total) {
    size_t by_value = 0, by_row = 0;
    const int items = static_cast<int>(std::max<uint64_t>(total, 1));
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, by_value, static_cast<const uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), static_cast<const uint32_t *>(nullptr),
                                             static_cast<uint32_t *>(nullptr), items, 0, 64);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, by_row, static_cast<const uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr), static_cast<const uint64_t *>(nullptr),
                                             static_cast<uint64_t *>(nullptr), items, 0, 32);
    return std::max<size_t>(std::max(by_value, by_row), 16);
}

void launch_fm_sort_rows(const uint64_t *d_values, const uint32_t *d_rows, uint64_t total, int row_bits, uint64_t *d_values_tmp, uint32_t *d_rows_tmp, uint64_t *d_values_out,
                         uint32_t *d_rows_out, void *d_temp, size_t temp_bytes, hipStream_t s) {
    if (total == 0) return;
    (void)hipcub::DeviceRadixSort::SortPairs(d_temp, temp_bytes, d_values, d_values_tmp, d_rows, d_rows_tmp, static_cast<int>(total), 0, 64, s);
    (void)hipcub::DeviceRadixSort::SortPairs(d_temp, temp_bytes, d_rows_tmp, d_rows_out, d_values_tmp, d_values_out, static_cast<int>(total), 0, row_bits, s);
}

void launch_fm_run_flags(const uint64_t *d_values, const uint32_t *d_rows, uint64_t total, uint64_t *d_flag, hipStream_t s) {
    if (total) hipLaunchKernelGGL(k_fm_run_flags, blocks_for(total), dim3(THREADS), 0, s, d_values, d_rows, total, d_flag);
}

void launch_fm_compact(const uint64_t *d_values, const uint64_t *d_rank, uint64_t total, const uint64_t *d_row_offsets, uint64_t m, uint64_t *d_out, uint64_t *d_new_offsets, hipStream_t s) {
    hipLaunchKernelGGL(k_fm_compact, blocks_for(std::max(total, m + 1)), dim3(THREADS), 0, s, d_values, d_rank, total, d_row_offsets, m, d_out, d_new_offsets);
}

}  // namespace gbwt_hip
