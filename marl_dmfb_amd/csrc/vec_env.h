// vec_env.h -- what the two environment libraries (dmfb_vec.hip, meda_vec.hip) share around their handles: the map
// accessor kernels, the observe-timing event ring and the skeleton of *_destroy.  Include after hip_abi.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// map selectors of *_get_map / *_set_map: DMFB_MAP_* and MEDA_MAP_* have these values
enum { kMapHealth = 0, kMapUsage = 1, kMapDegrade = 2 };

__global__ void k_get_map(size_t total, const double *health, const double *degrade, const uint16_t *usage, int which,
                          double *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    out[i] = which == kMapHealth ? health[i] : which == kMapDegrade ? degrade[i] : (double)usage[i];
}
__global__ void k_set_map(size_t total, double *health, double *degrade, uint16_t *usage, int which, const double *in) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    if (which == kMapHealth) health[i] = in[i];
    else if (which == kMapDegrade) degrade[i] = in[i];
    else usage[i] = (uint16_t)in[i];
}

// *_observe_timing: event pairs that receive the dispatch time stamps of the observation kernel
struct ObserveTiming {
    static constexpr int kPairs = 256;
    hipEvent_t ev[2 * kPairs] = {};
    int on = 0, used = 0;

    int enable(int enable) {  // creates the events the first time it is switched on
        if (enable && !ev[0])
            for (int i = 0; i < 2 * kPairs; ++i) HIP_TRY(hipEventCreate(&ev[i]));
        on = enable != 0;
        used = 0;
        return 0;
    }
    // the next pair for one launch; both stay nullptr (a plain launch) while off or once every pair is used
    void slot(hipEvent_t &t0, hipEvent_t &t1) {
        if (!on || used >= kPairs) return;
        t0 = ev[2 * used]; t1 = ev[2 * used + 1];
        used += 1;
    }
    int read(double *total_us, int *launches) {  // synchronises the host
        double sum = 0.0;
        for (int i = 0; i < used; ++i) {
            float ms = 0.f;
            HIP_TRY(hipEventSynchronize(ev[2 * i + 1]));
            HIP_TRY(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
            sum += (double)ms * 1e3;
        }
        *total_us = sum; *launches = used;
        used = 0;
        return 0;
    }
    void destroy() {
        for (int i = 0; i < 2 * kPairs; ++i)
            if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
};

// *_destroy: on the handle's device, free the device buffers and the timing events, then the handle
template <class Handle, class... Bufs> void destroy_handle(Handle *h, Bufs... bufs) {
    DeviceGuard g(h->cfg.device);
    ((void)hipFree((void *)bufs), ...);
    h->timing.destroy();
    delete h;
}

}  // namespace
