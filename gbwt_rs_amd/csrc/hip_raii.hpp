// hip_raii.hpp -- the small owners the construction, the merge and the removal share (build.hip, capi_build.hip, capi_gfa_build.hip,
// merge.hip, capi_merge.hip, remove.hip, capi_remove.hip): a stream, a set of events, a workspace of the C ABI with the rows of a rebuild
// in it, and the host clock of the *_info structs.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>

#include "../../include/gbwt_hip.h"
#include "capi_internal.hpp"

namespace gbwt_hip {

struct Stream {
    hipStream_t s = nullptr;
    Stream() { HIP_CHECK(hipStreamCreate(&s)); }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
};

template <int N>
struct EventSet {
    hipEvent_t e[N] = {};
    EventSet() { for (auto &x : e) HIP_CHECK(hipEventCreate(&x)); }
    ~EventSet() { for (auto &x : e) if (x) (void)hipEventDestroy(x); }
    EventSet(const EventSet &) = delete;
    EventSet &operator=(const EventSet &) = delete;
};

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
