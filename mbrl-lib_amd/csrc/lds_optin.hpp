// lds_optin.hpp -- host side: a kernel that wants more dynamic LDS than the default 64 KB window opts in ONCE per device.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace hipets {

struct LdsOptIn {  // the per-device "has opted in" flags of ONE kernel
    std::atomic<bool> set[64] = {};
};

// Opt kernel `fn` in to `lds_max` bytes of dynamic LDS on the current device unless `once` says it has been done: one acquire load on the
// hot path, no lock (two host threads may both set it the first time: harmless; devices beyond the table set it at every launch).
inline hipError_t full_lds_once(LdsOptIn& once, const void* fn, int lds_max) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool slot = dev >= 0 && dev < 64;
    if (slot && once.set[dev].load(std::memory_order_acquire)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    if (e == hipSuccess && slot) once.set[dev].store(true, std::memory_order_release);
    return e;
}

}  // namespace hipets
