// suffix_array.hpp -- the suffix array builder (suffix_array.hip) as the C ABI calls it (capi_suffix_array.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "capi_internal.hpp"

namespace gbwt_hip {

// Suffix array, BWT and its runs of d_text[0, n) -- all three in HBM of the current device, d_bwt may be null -- on stream s; done when it
// returns, with all of its scratch given back.  sentinel: the BWT byte in front of suffix 0.  info: everything but text_ms, which the
// caller knows; ctx must have been made (ensure()).  GBWT_HIP_UNSUPPORTED / GBWT_HIP_CAPACITY by
// sa_plan.hpp, with the message in the thread's error slot; throws HipError.
gbwt_hip_status build_suffix_array(const uint8_t *d_text, uint64_t n, uint8_t sentinel, uint64_t *d_sa, uint8_t *d_bwt, SaContext &ctx, hipStream_t s,
                                   gbwt_hip_suffix_array_info &info);

}  // namespace gbwt_hip
