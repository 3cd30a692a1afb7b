// device_common.hpp -- small helpers shared by the kernel translation units.
#pragma once

#include <hip/hip_runtime.h>

#include "device_index.hpp"

namespace gbwt_hip {

constexpr int WAVE = 64;

inline unsigned grid_for(uint64_t n, unsigned block) { return static_cast<unsigned>((n + block - 1) / block); }
// the grid of a launch with one lane per item (items <= 2^32 at 256 threads: at most 2^24 blocks)
inline unsigned blocks_for(uint64_t items, unsigned threads = 256) { return grid_for(items, threads); }

// bits that hold 0 .. values - 1: at least one, at most `most`
inline int bits_for(uint64_t values, int most) {
    int b = 1;
    while (b < most && (uint64_t(1) << b) < values) b++;
    return b;
}

// lane `lane` of the wave's copies of v (any lane per lane: a permute, not a read of one lane into a scalar as coop_device.hpp's read_lane64)
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int lane) {
    const uint32_t lo = __shfl(static_cast<uint32_t>(v), lane, WAVE), hi = __shfl(static_cast<uint32_t>(v >> 32), lane, WAVE);
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// Bisections over a sorted a[lo, hi): the first index with a[i] >= x / with a[i] > x (hi: none)
template <class T>
__device__ __forceinline__ uint64_t lower_bound(const T *a, uint64_t lo, uint64_t hi, T x) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
template <class T>
__device__ __forceinline__ uint64_t upper_bound(const T *a, uint64_t lo, uint64_t hi, T x) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the last index of a sorted a[lo .. hi] (hi included) with a[i] <= x, where a[lo] <= x; over a[0, n), n > 0: the row, position or slot that holds x
__device__ __forceinline__ uint64_t last_at_or_before(const uint64_t *a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) { const uint64_t mid = lo + (hi - lo + 1) / 2; if (a[mid] <= x) lo = mid; else hi = mid - 1; }
    return lo;
}
__device__ __forceinline__ uint64_t last_at_or_before(const uint64_t *a, uint64_t n, uint64_t x) { return last_at_or_before(a, 0, n - 1, x); }

// GBWT::forward's guards (src/gbwt.rs:222-229): the node is in the alphabet
__device__ __forceinline__ bool landing_record(const DeviceIndex &ix, uint32_t node, uint64_t &rec) {
    if (node < ix.first_node) return false;
    rec = node - ix.alphabet_offset;
    return rec < ix.n_records;
}

// One raw descriptor (device_index.hpp) in registers.
struct RawDesc { uint4 A, B, C, D; };

__device__ __forceinline__ bool load_raw_desc(const DeviceIndex &ix, uint64_t node, RawDesc &d, uint64_t &rec) {
    if (node < ix.first_node) return false;
    rec = node - ix.alphabet_offset;
    if (rec >= ix.n_records) return false;
    d.A = ix.desc_raw[4 * rec]; d.B = ix.desc_raw[4 * rec + 1]; d.C = ix.desc_raw[4 * rec + 2]; d.D = ix.desc_raw[4 * rec + 3];
    return d.B.y != 0;   // empty record / sigma == 0 -> None
}

}  // namespace gbwt_hip
