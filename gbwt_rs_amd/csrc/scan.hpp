// scan.hpp -- the prefix sums of the library (scan.hip; HIP and hipcub only, no index types: a stand-alone program can compile the unit).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace gbwt_hip {

// d_out[0] = 0, d_out[i + 1] = d_in[0] + .. + d_in[i] for i < n, for any n: hipcub counts in int, so the items go `piece` at a time (1 <= piece
// <= SCAN_PIECE).  n <= piece is one memset of 8 bytes and one hipcub launch over the plain pointers; every further piece is one more hipcub
// launch, whose input yields the sum in front of the piece (the d_out word the piece before it has just written) on top of its first item.
// d_in is not modified.  temp_bytes >= scan_temp_bytes(n, piece), which is never 0 and sized for min(n, piece) items.  The hipcub status is
// ignored: callers check hipGetLastError.
constexpr uint64_t SCAN_PIECE = uint64_t(1) << 30;
size_t scan_temp_bytes(uint64_t n, uint64_t piece = SCAN_PIECE);
void launch_scan(const uint64_t *d_in, uint64_t *d_out, uint64_t n, void *d_temp, size_t temp_bytes, hipStream_t s, uint64_t piece = SCAN_PIECE);
// the hipcub launches of launch_scan(.., n, .., piece)
inline uint64_t scan_launches(uint64_t n, uint64_t piece = SCAN_PIECE) { return (n + piece - 1) / piece; }

// The exclusive scan of per-record block counts (n < 2^31; nothing is launched for n = 0)
size_t block_scan_temp_bytes(uint64_t n);
void launch_block_scan(const uint32_t *d_counts, uint32_t *d_block_base, uint64_t n, void *d_temp, size_t temp_bytes, hipStream_t stream);

}  // namespace gbwt_hip
