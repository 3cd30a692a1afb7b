// scan.hip -- the prefix sums of the library (scan.hpp).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <iterator>

#include "scan.hpp"

namespace {

// The input of a piece behind the first: item i of the piece, and the sum in front of the piece on top of item 0
struct CarriedInput {
    using iterator_category = std::random_access_iterator_tag;
    using value_type = uint64_t;
    using difference_type = std::ptrdiff_t;
    using pointer = const uint64_t *;
    using reference = uint64_t;
    const uint64_t *in, *before;
    difference_type i;
    __host__ __device__ uint64_t operator[](difference_type k) const { return in[i + k] + (i + k == 0 ? *before : 0); }
    __host__ __device__ uint64_t operator*() const { return (*this)[0]; }
    __host__ __device__ CarriedInput operator+(difference_type k) const { return {in, before, i + k}; }
    __host__ __device__ CarriedInput operator-(difference_type k) const { return {in, before, i - k}; }
    __host__ __device__ difference_type operator-(const CarriedInput &o) const { return i - o.i; }
    __host__ __device__ CarriedInput &operator+=(difference_type k) { i += k; return *this; }
    __host__ __device__ CarriedInput &operator++() { i++; return *this; }
};

}  // namespace

namespace gbwt_hip {

size_t scan_temp_bytes(uint64_t n, uint64_t piece) {
    const int items = static_cast<int>(std::min(n, piece));
    size_t bytes = 0, carried = 0;
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, bytes, static_cast<const uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), items);
    if (n > piece) (void)hipcub::DeviceScan::InclusiveSum(nullptr, carried, CarriedInput{nullptr, nullptr, 0}, static_cast<uint64_t *>(nullptr), items);
    return std::max<size_t>(std::max(bytes, carried), 16);
}

void launch_scan(const uint64_t *d_in, uint64_t *d_out, uint64_t n, void *d_temp, size_t temp_bytes, hipStream_t s, uint64_t piece) {
    (void)hipMemsetAsync(d_out, 0, sizeof(uint64_t), s);
    if (n == 0) return;
    (void)hipcub::DeviceScan::InclusiveSum(d_temp, temp_bytes, d_in, d_out + 1, static_cast<int>(std::min(n, piece)), s);
    for (uint64_t at = piece; at < n; at += piece)
        (void)hipcub::DeviceScan::InclusiveSum(d_temp, temp_bytes, CarriedInput{d_in + at, d_out + at, 0}, d_out + at + 1, static_cast<int>(std::min(piece, n - at)), s);
}

size_t block_scan_temp_bytes(uint64_t n) {
    size_t bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, static_cast<const uint32_t *>(nullptr), static_cast<uint32_t *>(nullptr), static_cast<int>(n));
    return bytes;
}

void launch_block_scan(const uint32_t *d_counts, uint32_t *d_block_base, uint64_t n, void *d_temp, size_t temp_bytes, hipStream_t stream) {
    if (n == 0) return;
    (void)hipcub::DeviceScan::ExclusiveSum(d_temp, temp_bytes, d_counts, d_block_base, static_cast<int>(n), stream);
}

}  // namespace gbwt_hip
