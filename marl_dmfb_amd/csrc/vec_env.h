// vec_env.h -- what the two environment libraries (dmfb_vec.hip, meda_vec.hip) share around their handles: the map
// accessor kernels, the episode close of the staged global state (*_global_obs_stage_close), the observe-timing event ring
// and the skeleton of *_destroy.  Include after hip_abi.h.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <type_traits>

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

// Bytes [lo, hi) of one staged episode row: src below `keep` is copied, the rest of the range is zeroed.  V-byte accesses (both
// rows V-aligned); a vector that straddles `keep` or the end of the range goes byte by byte.
template <int V> __device__ inline void close_range(const int8_t *__restrict__ src, int8_t *__restrict__ dst, size_t lo, size_t hi,
                                                    size_t keep) {
    using U = typename std::conditional<V == 16, uint4, typename std::conditional<V == 4, uint32_t, uint8_t>::type>::type;
    for (size_t o = lo + (size_t)threadIdx.x * V; o < hi; o += (size_t)blockDim.x * V) {
        if (o + V <= hi && (o + V <= keep || o >= keep)) {
            U v;
            if (o < keep) v = *(const U *)(src + o);
            else memset(&v, 0, sizeof(U));
            *(U *)(dst + o) = v;
        } else {
            for (size_t b = o; b < o + V && b < hi; ++b) dst[b] = b < keep ? src[b] : (int8_t)0;
        }
    }
}

// Episode close of the staged global state (dmfb_vec_global_obs_stage_close, meda_vec_global_obs_stage_close): work item =
// (chip, kCloseChunk bytes of its (T + 1) * S row), chip-major; workgroup b takes the items b, b + gridDim.x, ..., so that the
// copies of the chips closing in a lock-step spread over the whole grid.  The workgroup checks blockDim.x of its items at once
// (one lane each: the chip's slot and step index), lists those that copy (ballot + prefix count, in item order) and copies them
// one after the other with all its lanes: a chip that does not close costs one lane two loads, not a serial round trip.
constexpr int kCloseChunk = 16 * 1024;
constexpr int kCloseBlock = 256;
__global__ __launch_bounds__(kCloseBlock) void k_state_close(int E, int T, size_t S, int slots, int chunks,
                                                             const int32_t *__restrict__ t_ep, const int32_t *__restrict__ close_slot,
                                                             const int8_t *__restrict__ stage, int8_t *__restrict__ ring) {
    __shared__ int2 todo[kCloseBlock];   // (chip, chunk) of the items to copy, in item order
    __shared__ int wave_n[kCloseBlock / 64];
    const size_t R = (size_t)(T + 1) * S;
    const long long items = (long long)E * chunks, step = (long long)gridDim.x * kCloseBlock;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (long long g0 = blockIdx.x; g0 < items; g0 += step) {
        const long long it = g0 + (long long)threadIdx.x * gridDim.x;
        int e = 0, ck = 0;
        bool copy = false;
        if (it < items) {
            e = (int)(it / chunks);
            ck = (int)(it - (long long)e * chunks);
            const int slot = close_slot[e], t = t_ep[e];
            copy = slot >= 0 && slot < slots && t >= 0 && t < T;
        }
        const unsigned long long m = __ballot(copy);
        if (lane == 0) wave_n[wv] = __popcll(m);
        __syncthreads();
        int off = 0, n = 0;
        for (int w = 0; w < kCloseBlock / 64; ++w) {
            off += w < wv ? wave_n[w] : 0;
            n += wave_n[w];
        }
        if (copy) todo[off + __popcll(m & ((1ull << lane) - 1))] = make_int2(e, ck);
        __syncthreads();
        for (int q = 0; q < n; ++q) {
            const int ce = todo[q].x, cc = todo[q].y;
            const int8_t *src = stage + (size_t)ce * R;
            int8_t *dst = ring + (size_t)close_slot[ce] * R;
            const size_t lo = (size_t)cc * kCloseChunk, hi = min(R, lo + (size_t)kCloseChunk), keep = (size_t)(t_ep[ce] + 2) * S;
            const uintptr_t al = (uintptr_t)src | (uintptr_t)dst;
            if ((al & 15) == 0) close_range<16>(src, dst, lo, hi, keep);
            else if ((al & 3) == 0) close_range<4>(src, dst, lo, hi, keep);
            else close_range<1>(src, dst, lo, hi, keep);
        }
        __syncthreads();   // todo / wave_n are rewritten by the next batch
    }
}

// The launch of k_state_close over E chips whose staged rows are (T + 1) * S bytes (grid: at most 4 workgroups per CU).
inline int launch_state_close(int E, int T, size_t S, int slots, int n_cu, const int32_t *t_ep, const int32_t *close_slot,
                              const int8_t *stage, int8_t *ring, hipStream_t s) {
    const size_t R = (size_t)(T + 1) * S;
    const int chunks = (int)((R + kCloseChunk - 1) / kCloseChunk);
    const long long items = (long long)E * chunks;
    const int grid = (int)std::min<long long>(items, 4LL * n_cu);
    LAUNCH(k_state_close, dim3(grid), dim3(kCloseBlock), 0, s, E, T, S, slots, chunks, t_ep, close_slot, stage, ring);
    return 0;
}

// Grid of a persistent kernel with `lds` bytes of LDS per workgroup over `tiles` tiles: as many workgroups as fit the chip at
// once (160 KiB of LDS per CU, at most 8 per CU, at most `per_cu_cap` when that is positive), or one per tile if that is fewer.
inline int persistent_grid(size_t lds, int tiles, int n_cu, int per_cu_cap = 0) {
    int per_cu = (int)((size_t)160 * 1024 / lds);
    per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
    if (per_cu_cap > 0 && per_cu_cap < per_cu) per_cu = per_cu_cap;
    return tiles < n_cu * per_cu ? tiles : n_cu * per_cu;
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
