// counted_buffer.hpp -- the scratch of the makers (construction, merge, removal, suffix array, GFA parse): HBM that is counted while it is held,
// and the prefix sum of the library calls over it.
#pragma once

#include <hip/hip_runtime.h>
#include <hipcub/device/device_scan.hpp>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "capi_status.hpp"

namespace gbwt_hip {

// What the buffers of one maker hold now and the most they ever held
struct CountedScratch {
    size_t now = 0, peak = 0;
};
struct CountedBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
    CountedScratch *owner = nullptr;
    CountedBuf() = default;
    CountedBuf(CountedScratch &sc, size_t need) { alloc(sc, need); }
    CountedBuf(const CountedBuf &) = delete;
    CountedBuf &operator=(const CountedBuf &) = delete;
    ~CountedBuf() { release(); }
    void alloc(CountedScratch &sc, size_t need) {
        release();
        const size_t want = std::max<size_t>(need, 256);
        if (hipError_t e = hipMalloc(&ptr, want); e != hipSuccess) { ptr = nullptr; throw HipError{e, "hipMalloc(&ptr, want)"}; }
        bytes = want; owner = &sc;
        sc.now += want; sc.peak = std::max(sc.peak, sc.now);
    }
    void release() noexcept {
        if (!ptr) return;
        (void)hipFree(ptr);
        owner->now -= bytes;
        ptr = nullptr; bytes = 0;
    }
    template <class T> T *as() const { return static_cast<T *>(ptr); }
};

// out[i] = in[0] + .. + in[i - 1] for i < n (in place where out == in); temp grows as needed
template <class T>
void exclusive_sum(const T *in, T *out, uint64_t n, CountedScratch &sc, CountedBuf &temp, hipStream_t s) {
    size_t bytes = 0;
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, n, s));
    if (bytes > temp.bytes || !temp.ptr) temp.alloc(sc, bytes);
    HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(temp.ptr, bytes, in, out, n, s));
}

}  // namespace gbwt_hip
