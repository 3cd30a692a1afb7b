// lazy_build.hpp -- a part of a handle that is built on first use, by whichever thread asks first (plain C++: the loader uses it too).
#pragma once

#include <atomic>
#include <mutex>

namespace gbwt_hip {

// ensure(build) runs build() under the mutex unless an earlier build has succeeded; made() is a lock-free look at that.  A build that
// throws marks nothing: every later caller builds again and gets the same error from the same input.  (std::once_flag promises that
// retry as well, but libstdc++ before GCC 11 deadlocks or never retries after a throw.)
class LazyBuild {
public:
    bool made() const { return made_.load(std::memory_order_acquire); }
    template <class Build> void ensure(Build &&build) {
        if (made()) return;
        std::lock_guard<std::mutex> hold(lock_);
        if (made_.load(std::memory_order_relaxed)) return;
        build();
        made_.store(true, std::memory_order_release);
    }

private:
    std::mutex lock_;
    std::atomic<bool> made_{false};
};

}  // namespace gbwt_hip
