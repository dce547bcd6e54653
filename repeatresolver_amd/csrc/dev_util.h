// dev_util.h -- what the host side of every stage's .hip file needs around its kernels: the error macro, the clock, the device
// buffers of one call, and (abi_guard.h) the guard of the C ABI.  Not part of the ABI.  The including file defines PWR_STAGE,
// the prefix of its messages ("pmc", "pgr", ...), first.
#ifndef PWR_DEV_UTIL_H
#define PWR_DEV_UTIL_H

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <vector>

#include "abi_guard.h"

#define HIPC(call)                                                                             \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, PWR_STAGE ": %s failed: %s\n", #call, hipGetErrorString(e_));     \
            return PWR_ERR_DEVICE;                                                             \
        }                                                                                      \
    } while (0)

[[maybe_unused]] static double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

namespace {   // (per file, like everything else here: nothing of it reaches the library's dynamic symbols)
// device allocations of one call, released together on every way out.  After a null from get / put the caller returns `err`.
struct DevArena {
    std::vector<void *> all;
    int err = PWR_ERR_NOMEM;                                           // PWR_ERR_DEVICE once a copy has failed
    DevArena() = default;
    DevArena(const DevArena &) = delete;                               // (it frees what it holds)
    // n elements (at least one); null when the device has no room
    template <class T> T *get(size_t n)
    {
        all.push_back(nullptr);                                        // (the slot first: no pointer is lost to a failing push_back)
        if (hipMalloc(&all.back(), (n ? n : 1) * sizeof(T)) != hipSuccess) { all.pop_back(); return nullptr; }
        return (T *)all.back();
    }
    // get + the copy of host[n] to it; null when either fails
    template <class T> T *put(const T *host, size_t n)
    {
        T *p = get<T>(n);
        if (!p || !n) return p;
        const hipError_t e = hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice);
        if (e == hipSuccess) return p;
        fprintf(stderr, PWR_STAGE ": hipMemcpy to the device failed: %s\n", hipGetErrorString(e));
        err = PWR_ERR_DEVICE;
        return nullptr;
    }
    ~DevArena() { for (void *p : all) (void)hipFree(p); }
};

// n halved (rounding up) while fits(n) says that the device refuses the buffers of that size; the refusal's HIP error, which
// would stick, is cleared.  PWR_ERR_NOMEM when not even n == 1 fits.  fits() lets go of what a refused attempt has got.
template <class F> int largest_that_fits(int &n, F fits)
{
    for (; !fits(n); n = (n + 1) / 2) {
        (void)hipGetLastError();
        if (n == 1) return PWR_ERR_NOMEM;
    }
    return PWR_OK;
}
}   // namespace

#endif /* PWR_DEV_UTIL_H */
