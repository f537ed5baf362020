// r48_host.h -- the host-side glue of the C-ABI entry points, stated once: error reporting (fail, launched),
// launch grids, pointer-alignment checks and the device guard (inline, here); the thread-local error
// string, the stream's device, the CU count and the dynamic-LDS opt-in (defined in r48_env.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/rein48.h"

namespace r48 {
void set_last_error(const std::string &msg);
// Device the stream's work runs on (the null stream: the calling thread's current device).
int stream_device(hipStream_t stream);
// Compute-unit count of `device` (queried once per device; 256 if the query fails).
int device_cus(int device);
// hipFuncAttributeMaxDynamicSharedMemorySize = bytes for `kernel` on `device`, set once per
// (kernel, device) pair; thread-safe (a mutex around a small set), the caller's current device kept.
// false (and r48_last_error set) when the opt-in fails; only a success is remembered.
bool ensure_dynamic_lds(const void *kernel, int bytes, int device);

// Record `msg` for r48_last_error and hand `code` back: `return fail(R48_EINVAL, "...")`.
inline int fail(int code, const std::string &msg)
{
    set_last_error(msg);
    return code;
}

// After a kernel launch: R48_OK, or R48_EHIP with "<what>: <HIP's error string>" recorded.
inline int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(R48_EHIP, std::string(what) + ": " + hipGetErrorString(e));
    return R48_OK;
}

// One thread per item, `block` threads per block.
inline dim3 grid_for(int64_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

// `a` is a power of two; NULL is aligned.
inline bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool aligned16(const void *p) { return aligned(p, 16); }
template <class... P>
inline bool all_aligned16(const P *...p)
{
    return (aligned16(p) && ...);
}

// Makes `dev` the calling thread's device for a scope and restores the previous one after it;
// `ok` is false when the switch failed.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess)
            prev = -1;
        if (prev != dev)
            ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
};
}  // namespace r48
