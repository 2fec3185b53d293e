// launch.hpp — the one launch path of the library's kernels: every launcher of the transform engines, and launch() /
// launch_named() of capi_internal.hpp, are this function.
#pragma once
#include <hip/hip_runtime.h>

#include "ntt_kernels.hpp"

namespace fhe {

// dynamic LDS above 64 KiB must be opted into per kernel
static inline hipError_t allow_big_lds(const void *fn, size_t bytes) {
    if (bytes <= 65536) return hipSuccess;
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// x is computed in 64 bits by the callers (rows x blocks): it is checked here before it narrows
struct LaunchGrid {
    u64 x;
    unsigned y = 1, z = 1;
};

// The launch itself: the LDS opt-in, the timer (label and tag name the row of fhe_ntt_kernel_timing_read) around the launch alone,
// one error check.  The grid is launched as it is: an empty one is HIP's to report (launch_named of capi_internal.hpp, whose
// callers in tfhe_boot.hip hand it an empty grid to have it reported)
template <class... P, class... A>
hipError_t launch_grid(void (*kernel)(P...), const char *label, int tag, dim3 grid, unsigned block, size_t lds_bytes, hipStream_t st, const A &...args) {
    if (hipError_t e = allow_big_lds((const void *)kernel, lds_bytes)) return e;
    {
        KernelTimer kt(label, tag, st);
        hipLaunchKernelGGL(kernel, grid, dim3(block), lds_bytes, st, static_cast<P>(args)...);
    }
    return hipGetLastError();
}

// The launchers' path: an empty grid is no launch, a grid past 2^31 - 1 workgroups is the caller's error, then launch_grid
template <class... P, class... A>
hipError_t launch_kernel(void (*kernel)(P...), const char *label, int tag, LaunchGrid grid, unsigned block, size_t lds_bytes, hipStream_t st,
                         const A &...args) {
    if (grid.x == 0) return hipSuccess;
    if (grid.x > 0x7fffffffull) return hipErrorInvalidValue;
    return launch_grid(kernel, label, tag, dim3((unsigned)grid.x, grid.y, grid.z), block, lds_bytes, st, args...);
}

}  // namespace fhe
