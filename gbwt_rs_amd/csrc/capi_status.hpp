// capi_status.hpp -- statuses, the HIP error of a failed call and the guards of an entry point of the C ABI: what every other internal header builds on.
#pragma once

#include <hip/hip_runtime.h>

#include <new>
#include <stdexcept>
#include <string>

#include "../../include/gbwt_hip.h"
#include "host_index.hpp"

namespace gbwt_hip {

std::string &last_error_slot();   // thread-local message of the last failing call

inline gbwt_hip_status fail(gbwt_hip_status st, const std::string &msg) {
    last_error_slot() = msg;
    return st;
}

struct HipError { hipError_t err; const char *what; };

#define HIP_CHECK(expr)                                            \
    do {                                                           \
        hipError_t e_ = (expr);                                    \
        if (e_ != hipSuccess) throw gbwt_hip::HipError{e_, #expr}; \
    } while (0)

inline gbwt_hip_status status_of(const HipError &e) {
    std::string msg = std::string(e.what) + ": " + hipGetErrorString(e.err);
    if (e.err == hipErrorNoDevice || e.err == hipErrorInvalidDevice) return fail(GBWT_HIP_NO_DEVICE, msg);
    return fail(GBWT_HIP_DEVICE_ERROR, msg);
}

// The catch of an entry point that allocates by the size of a request: out of device memory is the caller's to act on (`what`: "the
// merge", "a locate request", ...), and the error state is cleared so that the next call starts clean
inline gbwt_hip_status status_of(const HipError &e, const char *what) {
    if (e.err != hipErrorOutOfMemory) return status_of(e);
    (void)hipGetLastError();
    return fail(GBWT_HIP_CAPACITY, std::string(what) + " does not fit in device memory: " + e.what);
}

// The checks every call that makes a handle starts with: its flags, and -- once its arguments are through -- a device to make it on
inline gbwt_hip_status check_open_flags(uint32_t flags) {
    if (flags == 0 || (flags & ~uint32_t(GBWT_HIP_OPEN_ALL)) != 0) return fail(GBWT_HIP_BAD_ARGUMENT, "flags: a non-empty set of GBWT_HIP_OPEN_EXTRACT | _SEARCH | _GFA");
    return GBWT_HIP_OK;
}
inline uint32_t normalised_caps(uint32_t flags) { return (flags & GBWT_HIP_OPEN_GFA) ? (flags | GBWT_HIP_OPEN_EXTRACT) : flags; }   // the lines are formatted from extracted rows
inline gbwt_hip_status require_device() {
    int count = 0;
    if (hipGetDeviceCount(&count) == hipSuccess && count != 0) return GBWT_HIP_OK;
    (void)hipGetLastError();
    return fail(GBWT_HIP_NO_DEVICE, "no HIP device available (libgbwt_hip has no CPU fallback)");
}

// Lippincott function: the status of the exception in flight.  No exception may cross the C ABI (the caller is Rust / C /
// ctypes: it would be std::terminate), so every extern "C" entry point that can throw wraps its body in
// GBWT_HIP_GUARD_BEGIN / GBWT_HIP_GUARD_END, whatever it already catches inside.
inline gbwt_hip_status status_of_current_exception() noexcept {
    try {
        throw;
    } catch (const InvalidData &e) {
        return fail(GBWT_HIP_INVALID_DATA, e.what());
    } catch (const IoError &e) {
        return fail(GBWT_HIP_IO_ERROR, e.what());
    } catch (const Unsupported &e) {
        return fail(GBWT_HIP_UNSUPPORTED, e.what());
    } catch (const HipError &e) {
        return status_of(e);
    } catch (const std::bad_alloc &) {
        return fail(GBWT_HIP_DEVICE_ERROR, "out of host memory");
    } catch (const std::length_error &e) {   // a size taken from a file that no container can hold
        return fail(GBWT_HIP_INVALID_DATA, std::string("length error: ") + e.what());
    } catch (const std::exception &e) {
        return fail(GBWT_HIP_DEVICE_ERROR, std::string("unexpected exception: ") + e.what());
    } catch (...) {
        return fail(GBWT_HIP_DEVICE_ERROR, "unexpected exception");
    }
}

#define GBWT_HIP_GUARD_BEGIN try {
#define GBWT_HIP_GUARD_END } catch (...) { return gbwt_hip::status_of_current_exception(); }

}  // namespace gbwt_hip
