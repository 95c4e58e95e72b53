// hip_abi.h -- host plumbing shared by the C ABIs of the HIP libraries: the last-HIP-error slot, HIP_TRY / LAUNCH,
// DeviceGuard and the once-per-device dynamic-LDS limit.
//
// Define before including it:
//   HIP_ABI_TAG  the library's name, for the DMFB_VEC_DEBUG line ("dmfb_vec", "crnn_ops", ...)
//   HIP_ABI_ERR  the library's return code for a failed HIP call (its *_ERR_HIP)
// Everything here has internal linkage: every translation unit keeps its own last-error slot, which its
// *_last_hip_error() returns.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#if !defined(HIP_ABI_TAG) || !defined(HIP_ABI_ERR)
#error "define HIP_ABI_TAG and HIP_ABI_ERR before including hip_abi.h"
#endif

namespace {

thread_local int g_last_hip = 0;

// Records a failed HIP call and returns the library's error code; DMFB_VEC_DEBUG=1 in the environment prints it to stderr.
inline int hip_fail(hipError_t e, const char *what, int line) {
    g_last_hip = (int)e;
    if (getenv("DMFB_VEC_DEBUG"))
        fprintf(stderr, HIP_ABI_TAG ": %s failed at line %d: %s (%d)\n", what, line, hipGetErrorString(e), (int)e);
    return HIP_ABI_ERR;
}

#define HIP_TRY(expr)                                                 \
    do {                                                              \
        hipError_t _e = (expr);                                       \
        if (_e != hipSuccess) return hip_fail(_e, #expr, __LINE__);   \
    } while (0)

// The error of the launches `launch()` makes: stale errors left by other users of the runtime are dropped first.
template <class F> inline hipError_t launch_status(F &&launch) {
    (void)hipGetLastError();
    launch();
    return hipGetLastError();
}

#define LAUNCH(kernel, grid, block, lds, stream, ...)                      \
    do {                                                                   \
        (void)hipGetLastError();                                           \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__); \
        HIP_TRY(hipGetLastError());                                        \
    } while (0)

// Makes `dev` current for the guard's lifetime (the environment handles remember their device).
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        hipError_t e = hipGetDevice(&prev);
        if (e != hipSuccess) { ok = false; hip_fail(e, "hipGetDevice", __LINE__); prev = -1; return; }
        if (prev != dev) {
            e = hipSetDevice(dev);
            if (e != hipSuccess) { ok = false; hip_fail(e, "hipSetDevice", __LINE__); }
        } else {
            prev = -1;
        }
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// The dynamic-LDS limit is an attribute of the function ON ONE DEVICE: one LdsLimit per kernel (a function-local static)
// remembers per device whether it has been raised (a process may drive several GPUs; one rank per GPU is the normal case).
// Thread-compatible like the rest of the ABI.
struct LdsLimit {
    bool done[64] = {};
    int raise(const void *kernel, size_t bytes) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        const bool known = dev >= 0 && dev < 64;
        if (known && done[dev]) return 0;
        HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        if (known) done[dev] = true;
        return 0;
    }
};

// ---- last-workgroup-done hand-off: every workgroup of a launch writes partial results to global memory, then calls this
// (all threads, 1-D block); it returns true in every thread of the ONE workgroup that arrived last, which may then read all the
// partials with partial_load().  The XCDs' L2s are not coherent with each other, so: every wave drains its stores, one lane makes
// them visible with an agent-scope release, draws a ticket with ONE integer atomic, and the last arriver takes an agent-scope
// acquire before the workgroup reads.  `ticket` is a zero-initialised device word that only launches ordered on one stream
// share; atomicInc wraps it back to 0 with the last arrival, so the next launch (or a replay of a captured one) finds it reset.
__device__ __forceinline__ bool last_workgroup_arrives(unsigned *ticket, unsigned n_groups, int *s_last) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const bool last = atomicInc(ticket, n_groups - 1) == n_groups - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *s_last = last ? 1 : 0;
    }
    __syncthreads();
    return *s_last != 0;
}

// A partial another workgroup of this launch wrote: a device-scope vector load that bypasses this CU's L1
__device__ __forceinline__ float partial_load(const float *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace
