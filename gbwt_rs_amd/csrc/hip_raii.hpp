// hip_raii.hpp -- the small owners of the library: a stream, a set of events and a few words of pinned host memory (workspaces, the
// construction, the merge, the removal, the locate build, the GFA parse, the components), a workspace of the C ABI with the rows of a
// rebuild in it, and the host clock of the *_info structs.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>

#include "../../include/gbwt_hip.h"
#include "capi_status.hpp"

namespace gbwt_hip {

// How an owner that a workspace holds is made: by the first request that needs it, not with the workspace (gbwt_hip_workspace_create
// stays cheap, and a family that is never asked for costs nothing)
struct OnFirstUse {};

struct Stream {
    hipStream_t s = nullptr;
    Stream() { HIP_CHECK(hipStreamCreate(&s)); }
    explicit Stream(OnFirstUse) {}
    void create(unsigned flags) { HIP_CHECK(hipStreamCreateWithFlags(&s, flags)); }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    operator hipStream_t() const { return s; }
};

template <int N>
struct EventSet {
    hipEvent_t e[N] = {};
    EventSet() { ensure(); }
    explicit EventSet(OnFirstUse) {}
    void ensure() { for (auto &x : e) if (!x) HIP_CHECK(hipEventCreate(&x)); }
    ~EventSet() { for (auto &x : e) if (x) (void)hipEventDestroy(x); }
    EventSet(const EventSet &) = delete;
    EventSet &operator=(const EventSet &) = delete;
    hipEvent_t operator[](int i) const { return e[i]; }
};

// Four words of pinned host memory, made by the first request that reads a total back while the device goes on
struct PinnedWords {
    uint64_t *p = nullptr;
    void ensure() { if (!p) HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&p), 4 * sizeof(uint64_t))); }
    PinnedWords() = default;
    ~PinnedWords() { if (p) (void)hipHostFree(p); }
    PinnedWords(const PinnedWords &) = delete;
    PinnedWords &operator=(const PinnedWords &) = delete;
};

// one value from the device, behind everything the stream holds
template <class T> T read_value(const T *d, hipStream_t s) {
    T v{};
    HIP_CHECK(hipMemcpyAsync(&v, d, sizeof(T), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return v;
}

struct Workspace {
    gbwt_hip_workspace *ws = nullptr;
    Workspace() = default;
    ~Workspace() { if (ws) gbwt_hip_workspace_destroy(ws); }
    Workspace(const Workspace &) = delete;
    Workspace &operator=(const Workspace &) = delete;
};

// Sequences ids[0, n) of a handle as rows in HBM, for a kernel on any stream to read (they stay in the workspace, which is made here)
static inline gbwt_hip_status extract_rows(const gbwt_hip_index *ix, Workspace &w, const uint64_t *ids, uint64_t n, gbwt_hip_paths &rows) {
    rows = gbwt_hip_paths{nullptr, nullptr, 0, 0};
    if (n == 0) return GBWT_HIP_OK;
    gbwt_hip_status st = gbwt_hip_workspace_create(ix, &w.ws);
    if (st != GBWT_HIP_OK) return st;
    st = gbwt_hip_extract_device(ix, w.ws, ids, n, &rows);
    if (st != GBWT_HIP_OK) return st;
    HIP_CHECK(hipDeviceSynchronize());                     // (the rows were written on the workspace's stream)
    return GBWT_HIP_OK;
}

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

}  // namespace gbwt_hip
