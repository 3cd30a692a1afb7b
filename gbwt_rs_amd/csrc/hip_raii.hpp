// hip_raii.hpp -- the small owners the construction, the merge and the removal share (build.hip, capi_build.hip, merge.hip, capi_merge.hip,
// remove.hip, capi_remove.hip): a stream, a set of events, a workspace of the C ABI, and the host clock of the *_info structs.
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

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

}  // namespace gbwt_hip
