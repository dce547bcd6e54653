// abi_guard.h -- no exception leaves the C ABI: the body of an extern "C" entry that can allocate on the host (a std::vector,
// a sort's buffer) runs inside abi_guard.  The library is loaded through ctypes, where an escaping std::bad_alloc ends the
// process; the inputs are MSAs of gigabytes.  Plain C++, no HIP: the host compiler alone can test it.  Not part of the ABI.
#ifndef PWR_ABI_GUARD_H
#define PWR_ABI_GUARD_H

#include <new>

#include "pwr.h"

// f's return code; PWR_ERR_NOMEM if it threw std::bad_alloc, PWR_ERR_INTERNAL if it threw anything else
template <class F> int abi_guard(F &&f) noexcept
{
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return PWR_ERR_NOMEM;
    } catch (...) {
        return PWR_ERR_INTERNAL;
    }
}

#endif /* PWR_ABI_GUARD_H */
