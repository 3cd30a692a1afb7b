// fm_index.hpp -- the kernels of the FM-index family (fm_index.hip) as the C ABI launches them (capi_fm.hip).  The layout is fm_layout.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fm_layout.hpp"

namespace gbwt_hip {

// ---- the build ----------------------------------------------------------------------------------
// d_hist[256] += the occurrences of every byte value in d_text[0, n) (zeroed by the caller)
void launch_fm_histogram(const uint8_t *d_text, uint64_t n, uint64_t *d_hist, hipStream_t s);
// The code of every row's BWT byte into its place in d_lines (fm_code_at), 0 for the row of suffix 0, whose number goes to *d_primary;
// rows = n + 1; d_code: the table of the index (u16[256])
void launch_fm_codes(const uint8_t *d_text, const uint64_t *d_sa, uint64_t n, const uint16_t *d_code, bool packed, uint8_t *d_lines, uint64_t *d_primary, hipStream_t s);
// d_block_counts[c * blocks + b] = occurrences of code c in block b, the primary row left out
void launch_fm_block_counts(const uint8_t *d_lines, uint64_t rows, uint64_t blocks, uint32_t sigma, bool packed, const uint64_t *d_primary, uint32_t *d_block_counts, hipStream_t s);
// d_scanned = the exclusive sums of d_block_counts in pieces of whole codes (a piece starts again at 0; the fill subtracts the value at a
// code's first block); temp: fm_scan_temp_bytes(blocks, sigma)
size_t fm_scan_temp_bytes(uint64_t blocks, uint32_t sigma);
void launch_fm_scan(const uint32_t *d_block_counts, uint32_t *d_scanned, uint64_t blocks, uint32_t sigma, void *d_temp, size_t temp_bytes, hipStream_t s);
// The occurrences in front of every block into the heads of the lines (packed) or into d_counts[b * sigma + c] (plain)
void launch_fm_fill(const uint32_t *d_scanned, uint64_t blocks, uint32_t sigma, bool packed, uint8_t *d_lines, uint32_t *d_counts, hipStream_t s);
// d_sa32[j] = d_sa[j]
void launch_fm_narrow_sa(const uint64_t *d_sa, uint64_t n, uint32_t *d_sa32, hipStream_t s);

// ---- queries ------------------------------------------------------------------------------------
struct FmTables { const uint16_t *code; const uint32_t *C; };
constexpr uint32_t FM_FLAG_OFFSETS = 1u;          // pattern offsets that descend or leave the pattern bytes
constexpr uint32_t FM_SHORT_ROW = 16;             // a located row of at most this many positions is copied by its own lane
// One lane per pattern k < m (bytes d_bytes[d_offsets[k], d_offsets[k + 1]) of `bytes` pattern bytes): d_ranges[2 k], [2 k + 1] = its SA range,
// d_counts[k] = its occurrences.  d_words: [0] flags (low half), [1] += backward steps
void launch_fm_count(const FmLayout &L, const FmTables &t, const uint64_t *d_offsets, const uint8_t *d_bytes, uint64_t m, uint64_t bytes, uint64_t *d_ranges, uint64_t *d_counts,
                     uint64_t *d_words, hipStream_t s);
// Row k of the result = d_sa32[lo_k, hi_k) as u64 at d_row_offsets[k]; d_rows (may be null): the row of every position
void launch_fm_locate_fill(const uint32_t *d_sa32, const uint64_t *d_ranges, const uint64_t *d_row_offsets, uint64_t m, uint64_t *d_positions, uint32_t *d_rows, hipStream_t s);
// Distinct values per row, ascending: (row, value) pairs sorted by value and then, stably, by row; a flag at the first of every run; behind
// the scan of the flags into d_rank[total + 1] the kept values and the offsets of their rows
size_t fm_sort_temp_bytes(uint64_t total);
void launch_fm_sort_rows(const uint64_t *d_values, const uint32_t *d_rows, uint64_t total, int row_bits, uint64_t *d_values_tmp, uint32_t *d_rows_tmp, uint64_t *d_values_out,
                         uint32_t *d_rows_out, void *d_temp, size_t temp_bytes, hipStream_t s);
void launch_fm_run_flags(const uint64_t *d_values, const uint32_t *d_rows, uint64_t total, uint64_t *d_flag, hipStream_t s);
void launch_fm_compact(const uint64_t *d_values, const uint64_t *d_rank, uint64_t total, const uint64_t *d_row_offsets, uint64_t m, uint64_t *d_out, uint64_t *d_new_offsets, hipStream_t s);

}  // namespace gbwt_hip
