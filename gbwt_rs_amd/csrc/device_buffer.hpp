// device_buffer.hpp -- the grow-only device buffer every handle and workspace is made of, and where its memory lies (GBWT_HIP_VMM).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "capi_status.hpp"

namespace gbwt_hip {

// Grow-only device buffer.
// Where a pass's 13 GB of rows land physically is worth up to 10 % of its time: on a fresh box one hipMalloc of that size takes one
// contiguous stretch of VRAM, and a pass over it takes 4.95 ms where the same buffer put together from chunks that lie SPREAD over the
// VRAM takes 4.45 (profiles/r02_walk_bounds.txt #25; the fast and slow "states" of a box in round 1 were this).  So the rows buffer of
// a workspace (may_spread), from 4 GiB, is built with the virtual-memory API: `spread` times as many physical chunks as needed are created, every spread-th is
// kept and mapped into one virtual range, the others are given back.  Chunks of 2 GiB: with 256 MB chunks the rows of ragged batches
// (walks out of lock step) were written 5 % slower than into one hipMalloc -- smaller mappings, less TLB reach -- with 2 GiB 1 %.  The
// price is paid when a workspace is sized: the driver clears what it hands out, about 15 ms per GB created (1.7 s for a 13 GB buffer at
// spread 8; spread 4 keeps half of the gain, 2 nothing).  hipMalloc whenever any of that fails.
// GBWT_HIP_VMM="0": always hipMalloc;  "<chunk MiB>:<spread, 0 = as much as half of the free memory allows, at most 8>:<min MiB>:<after>"
// (after = requests served as one hipMalloc before the buffer is rebuilt from spread chunks; 0 = spread at once).
struct VmmPolicy { size_t chunk = size_t(2048) << 20, min = size_t(4) << 30; unsigned spread = 0, after = 2; };
// GBWT_HIP_VMM, read when a workspace is created (the policy travels with its rows buffer)
inline VmmPolicy vmm_policy_from_env() {
    VmmPolicy p;
    if (const char *v = std::getenv("GBWT_HIP_VMM")) {
        unsigned long chunk = 0, spread = 0, min = 4096, after = 2;
        const int got = std::sscanf(v, "%lu:%lu:%lu:%lu", &chunk, &spread, &min, &after);
        if (got >= 1) { p.chunk = chunk << 20; p.spread = static_cast<unsigned>(spread); p.min = min << 20; }
        if (got >= 4) p.after = static_cast<unsigned>(after);
    }
    return p;
}

struct DeviceBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;
    std::vector<hipMemGenericAllocationHandle_t> chunks;   // empty: ptr comes from hipMalloc
    size_t reserved = 0;                                     // bytes of virtual range reserved at ptr (0: hipMalloc)
    size_t chunk_bytes = 0, mapped_chunks = 0;               // the first mapped_chunks chunks are mapped at ptr + i * chunk_bytes
    bool may_spread = false;                                 // the extracted rows of a workspace only: spreading the index arrays gains nothing (#25)
    VmmPolicy policy;                                        // how (set by the workspace from GBWT_HIP_VMM)
    unsigned uses = 0;                                       // requests the buffer has served at its present size
    ~DeviceBuffer() { release(); }
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    // hipFree waits for the work that may still use the memory; unmapping does not.  The rows of a workspace are handed out as raw
    // device pointers (gbwt_hip_paths, dist.device_view) that a consumer may still be reading on ANOTHER stream -- a torch kernel,
    // an RCCL send -- so a mapped buffer waits for the whole device before it goes.
    void release() noexcept {
        if (reserved) {
            (void)hipDeviceSynchronize();
            // one hipMemUnmap per hipMemMap: a single call over the whole range is not documented to undo several mappings, and
            // a chunk that stays mapped keeps its 2 GiB of VRAM for good
            for (size_t i = 0; i < mapped_chunks; i++) (void)hipMemUnmap(static_cast<char *>(ptr) + i * chunk_bytes, chunk_bytes);
            (void)hipMemAddressFree(ptr, reserved);
        } else if (ptr) (void)hipFree(ptr);
        for (auto h : chunks) (void)hipMemRelease(h);
        (void)hipGetLastError();
        chunks.clear();
        ptr = nullptr; bytes = 0; reserved = 0; chunk_bytes = 0; mapped_chunks = 0;
    }
    // Spreading costs seconds (the driver clears every chunk it hands out, and gives the unused ones back lazily: the NEXT large
    // allocation of the process waits for that), so a buffer starts as one hipMalloc -- what a one-shot extraction sees -- and is
    // rebuilt from spread chunks once it has served `policy.after` requests: a workspace that is used again and again (a server, the
    // timed passes of bench.py) pays once and gains on every pass after that.  The contents do not survive; callers reserve before
    // they write.
    void reserve(size_t need) {
        if (need <= bytes) {
            if (may_spread && reserved == 0 && policy.chunk != 0 && bytes >= policy.min && ++uses == policy.after) {
                const size_t want = bytes;
                release();
                if (!spread_chunks(want)) HIP_CHECK(hipMalloc(&ptr, want));
                bytes = want;
            }
            return;
        }
        release();
        uses = 0;
        const size_t want = std::max<size_t>(need, 256);
        if (may_spread && policy.chunk != 0 && want >= policy.min && policy.after == 0 && spread_chunks(want)) { bytes = want; return; }
        HIP_CHECK(hipMalloc(&ptr, want));
        bytes = want;
    }
    template <class T> T *as() const { return static_cast<T *>(ptr); }

private:
    // false (and nothing held) when the virtual-memory API does not cooperate
    bool spread_chunks(size_t want) noexcept {
        int device = 0;
        if (hipGetDevice(&device) != hipSuccess) return false;
        hipMemAllocationProp prop{};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = device;
        size_t granule = 0, free_bytes = 0, total_bytes = 0;
        if (hipMemGetAllocationGranularity(&granule, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || granule == 0) return false;
        if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess || want > free_bytes) return false;   // sizes out of a corrupt file: let hipMalloc say no
        const size_t chunk = (policy.chunk + granule - 1) / granule * granule, n = want / chunk + (want % chunk != 0 ? 1 : 0);
        // spread 0 = automatic: at most 8, and never more than HALF of the free memory in flight while the chunks are chosen -- other
        // contexts on the device (a second rank sharing the GPU, a torch allocator) must not see a spurious out-of-memory
        size_t spread = policy.spread;
        if (spread == 0) spread = std::min<size_t>(8, std::max<size_t>(1, free_bytes / 2 / (n * chunk)));
        // more chunks than needed, every spread-th kept: the kept ones lie `spread` chunks apart in whatever order the driver hands them out
        std::vector<hipMemGenericAllocationHandle_t> all;
        all.reserve(n * spread);
        for (size_t i = 0; i < n * spread; i++) {
            hipMemGenericAllocationHandle_t h;
            if (hipMemCreate(&h, chunk, &prop, 0) != hipSuccess) break;
            all.push_back(h);
        }
        (void)hipGetLastError();
        const size_t step = all.size() / n;     // >= 1 unless not even n chunks could be had
        for (size_t i = 0; i < all.size(); i++) {
            if (step != 0 && i % step == 0 && chunks.size() < n) chunks.push_back(all[i]);
            else (void)hipMemRelease(all[i]);
        }
        bool ok = chunks.size() == n && hipMemAddressReserve(&ptr, n * chunk, 0, nullptr, 0) == hipSuccess;
        if (ok) {
            reserved = n * chunk; chunk_bytes = chunk;
            for (size_t i = 0; i < n && ok; i++) {
                ok = hipMemMap(static_cast<char *>(ptr) + i * chunk, chunk, 0, chunks[i], 0) == hipSuccess;
                if (ok) mapped_chunks = i + 1;                 // a failure half-way unwinds exactly what was mapped
            }
            hipMemAccessDesc access{};
            access.location = prop.location;
            access.flags = hipMemAccessFlagsProtReadWrite;
            ok = ok && hipMemSetAccess(ptr, reserved, &access, 1) == hipSuccess;
        }
        if (!ok) { (void)hipGetLastError(); release(); }
        return ok;
    }
};

// What device_bytes() of a struct that owns buffers returns: the list stands directly under the declaration of the buffers
inline uint64_t bytes_of(std::initializer_list<const DeviceBuffer *> buffers) { uint64_t b = 0; for (const DeviceBuffer *q : buffers) b += q->bytes; return b; }

}  // namespace gbwt_hip
