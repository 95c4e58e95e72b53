// dmfb_vec.hip -- C ABI (include/dmfb_vec.h) of the vectorised DMFB environment, the
// N-independent kernels (observation, task/state/map accessors) and the dispatch to the per-N
// transition/reset kernels built from dmfb_vec_n.hip.  Device code: dmfb_kernels.h.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "dmfb_kernels.h"
#include "dmfb_shield.h"

#define HIP_ABI_TAG "dmfb_vec"
#define HIP_ABI_ERR DMFB_ERR_HIP
#include "hip_abi.h"
#include "vec_env.h"

static_assert(DMFB_MAP_HEALTH == kMapHealth && DMFB_MAP_USAGE == kMapUsage && DMFB_MAP_DEGRADE == kMapDegrade, "map selectors");

using namespace dmfbk;

namespace {

// ---- small utility kernels -----------------------------------------------------------------------
__global__ void k_set_task(DevCfg c, DevPtrs p, const int32_t *starts, const int32_t *ends) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.E) return;
    const int n = c.n, np = (n + 1) / 2, E = c.E;
    bool dup = false;
    for (int w = 0; w < np; ++w) {
        uint32_t sw = 0, gw = 0;
        for (int h = 0; h < 2 && 2 * w + h < n; ++h) {
            const size_t k = ((size_t)e * n + 2 * w + h) * 2;
            sw |= ((uint32_t)(starts[k] & 0xff) | ((uint32_t)(starts[k + 1] & 0xff) << 8)) << (16 * h);
            gw |= ((uint32_t)(ends[k] & 0xff) | ((uint32_t)(ends[k + 1] & 0xff) << 8)) << (16 * h);
        }
        p.starts[(size_t)w * E + e] = sw;
        p.st[(size_t)w * E + e] = sw;
        p.st[(size_t)(np + w) * E + e] = gw;
    }
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const size_t a = ((size_t)e * n + i) * 2, b = ((size_t)e * n + j) * 2;
            dup |= (starts[a] == starts[b]) && (starts[a + 1] == starts[b + 1]);
        }
    // counters to zero; the usage log keeps its length (injecting a task does not touch the maps)
    p.st[(size_t)(2 * np) * E + e] = (p.st[(size_t)(2 * np) * E + e] & (0xfffu << kUlenShift)) | (dup ? (FLAG_DUP << 16) : 0u);
    p.st[(size_t)(2 * np + 1) * E + e] = 0;
}

// Fold every chip's usage log into its usage map (no updateHealth): before the map is read or overwritten from outside.
// One wave per chip, LDS histogram per wave (dynamic LDS = 4 * hist_bytes).
__global__ __launch_bounds__(kBlock) void k_flush_usage(DevCfg c, DevPtrs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int e = blockIdx.x * (kBlock / kWave) + (int)(threadIdx.x / kWave);
    if (e >= c.E) return;
    const int lane = (int)(threadIdx.x & (kWave - 1));
    const size_t wstep = (size_t)(2 * ((c.n + 1) / 2)) * c.E + e;
    const uint32_t s = p.st[wstep];
    const int ulen = (int)(s >> kUlenShift);
    if (ulen == 0) return;  // (wave-uniform)
    uint16_t *hist = c.hist_bytes ? (uint16_t *)(smem + (size_t)(threadIdx.x / kWave) * c.hist_bytes) : nullptr;
    flush_usage(c, p, e, ulen, false, hist, lane);
    if (lane == 0) p.st[wstep] = s & ~(0xfffu << kUlenShift);
}

__global__ void k_get_task(DevCfg c, DevPtrs p, int32_t *starts, int32_t *ends) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.E) return;
    const int n = c.n, np = (n + 1) / 2, E = c.E;
    for (int i = 0; i < n; ++i) {
        const uint32_t s = (p.starts[(size_t)(i >> 1) * E + e] >> (16 * (i & 1))) & 0xffff;
        const uint32_t g = (p.st[(size_t)(np + (i >> 1)) * E + e] >> (16 * (i & 1))) & 0xffff;
        const size_t k = ((size_t)e * n + i) * 2;
        if (starts) { starts[k] = s & 0xff; starts[k + 1] = s >> 8; }
        if (ends) { ends[k] = g & 0xff; ends[k + 1] = g >> 8; }
    }
}

__global__ void k_set_blocks(DevCfg c, DevPtrs p, const int32_t *blocks, int nb) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.E) return;
    for (int b = 0; b < nb; ++b) {
        const int32_t *q = blocks + ((size_t)e * nb + b) * 4;
        p.blocks[(size_t)b * c.E + e] = (uint32_t)(q[0] & 0xff) | ((uint32_t)(q[1] & 0xff) << 8) | ((uint32_t)(q[2] & 0xff) << 16) |
                                         ((uint32_t)(q[3] & 0xff) << 24);
    }
}
__global__ void k_get_blocks(DevCfg c, DevPtrs p, int32_t *blocks, int cap) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.E) return;
    for (int b = 0; b < c.nb; ++b) {
        const uint32_t o = p.blocks[(size_t)b * c.E + e];
        int32_t *q = blocks + ((size_t)e * cap + b) * 4;
        q[0] = o & 0xff; q[1] = (o >> 8) & 0xff; q[2] = (o >> 16) & 0xff; q[3] = o >> 24;
    }
}

__global__ void k_get_state(DevCfg c, DevPtrs p, int32_t *pos, int32_t *dist, int32_t *step_count, int64_t *cons) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.E) return;
    const int n = c.n, np = (n + 1) / 2, E = c.E;
    for (int i = 0; i < n; ++i) {
        const uint32_t s = (p.st[(size_t)(i >> 1) * E + e] >> (16 * (i & 1))) & 0xffff;
        const uint32_t g = (p.st[(size_t)(np + (i >> 1)) * E + e] >> (16 * (i & 1))) & 0xffff;
        const int x = s & 0xff, y = s >> 8, gx = g & 0xff, gy = g >> 8;
        if (pos) { pos[((size_t)e * n + i) * 2] = x; pos[((size_t)e * n + i) * 2 + 1] = y; }
        if (dist) dist[(size_t)e * n + i] = iabs(x - gx) + iabs(y - gy);
    }
    if (step_count) step_count[e] = (int32_t)(p.st[(size_t)(2 * np) * E + e] & 0xffff);
    if (cons) cons[e] = (int64_t)p.st[(size_t)(2 * np + 1) * E + e];
}

// dmfb_vec_route_append: lane k = e * n + i writes droplet i's packed (x, y) byte pair to route[e][slot][i], so that the lanes
// of one chip store n consecutive pairs
__global__ void k_route_append(DevCfg c, DevPtrs p, int slot, int T, uint16_t *route) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int n = c.n, E = c.E;
    if (k >= (long)E * n) return;
    const int e = (int)(k / n), i = (int)(k - (long)e * n);
    const uint32_t s = (p.st[(size_t)(i >> 1) * E + e] >> (16 * (i & 1))) & 0xffff;   // x | y << 8
    route[((size_t)e * (T + 1) + slot) * n + i] = (uint16_t)s;
}

// RoutingTaskManager.getglobalobs() (dmfb.py:368-391) of G chips per workgroup: each chip's int8[3][W][L] row (S bytes) is
// zero-filled in LDS, one thread per chip scatters blocks (layer 2) and then droplets in ascending order (layer 0: i + 1 at the
// position, layer 1: i + 1 at the goal; the last writer wins, as in the reference), and the tile leaves in 4-byte stores.
// Chip e's row goes to dst0 + e * stride0 when sel[e] != 0 (sel NULL = all) and, when dst1 is set, also to dst1 + e * stride1
// when in addition term[e] == 0.  With t_row set (the stage of the continuous rollout) chip e's row goes to row t_row[e] + 1 of
// its T + 1 rows instead, dst0 + e * stride0 + (t_row[e] + 1) * S, and a chip whose t_row is outside [0, T) is skipped.
__global__ __launch_bounds__(256) void k_global_obs(DevCfg c, DevPtrs p, int G, const uint8_t *sel, const uint8_t *term,
                                                    int8_t *dst0, size_t stride0, int8_t *dst1, size_t stride1, int words,
                                                    const int32_t *t_row, int T) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tile[];
    const int WL = c.W * c.L, S = 3 * WL, Sw = (S + 3) / 4, E = c.E;
    const int e0 = blockIdx.x * G;
    const int gn = min(G, E - e0);
    auto skip = [&](int e) { return (sel && !sel[e]) || (t_row && (unsigned)t_row[e] >= (unsigned)T); };
    auto base0 = [&](int e) { return dst0 + (size_t)e * stride0 + (t_row ? (size_t)(t_row[e] + 1) * S : 0); };
    for (int k = threadIdx.x; k < gn * Sw; k += blockDim.x) tile[k] = 0u;
    __syncthreads();
    if ((int)threadIdx.x < gn) {
        const int e = e0 + (int)threadIdx.x;
        uint8_t *row = (uint8_t *)(tile + (size_t)threadIdx.x * Sw);
        if (!skip(e)) {
            for (int b = 0; p.blocks && b < c.nb; ++b) {
                const uint32_t o = p.blocks[(size_t)b * E + e];
                const int x1 = min((int)((o >> 8) & 0xff), c.W - 1), y1 = min((int)(o >> 24), c.L - 1);
                for (int x = o & 0xff; x <= x1; ++x)
                    for (int y = (o >> 16) & 0xff; y <= y1; ++y) row[2 * WL + x * c.L + y] = 1;
            }
            const int np = (c.n + 1) / 2;
            for (int i = 0; i < c.n; ++i) {
                const uint32_t s = (p.st[(size_t)(i >> 1) * E + e] >> (16 * (i & 1))) & 0xffff;
                const uint32_t g = (p.st[(size_t)(np + (i >> 1)) * E + e] >> (16 * (i & 1))) & 0xffff;
                const int x = s & 0xff, y = s >> 8, gx = g & 0xff, gy = g >> 8;
                if (x < c.W && y < c.L) row[x * c.L + y] = (uint8_t)(i + 1);
                if (gx < c.W && gy < c.L) row[WL + gx * c.L + gy] = (uint8_t)(i + 1);
            }
        }
    }
    __syncthreads();
    if (words) {  // S % 4 == 0 and 4-byte aligned destinations
        for (int k = threadIdx.x; k < gn * Sw; k += blockDim.x) {
            const int j = k / Sw, w = k - j * Sw, e = e0 + j;
            if (skip(e)) continue;
            const uint32_t v = tile[k];
            ((uint32_t *)base0(e))[w] = v;
            if (dst1 && !term[e]) ((uint32_t *)(dst1 + (size_t)e * stride1))[w] = v;
        }
    } else {
        const uint8_t *bytes = (const uint8_t *)tile;
        for (int k = threadIdx.x; k < gn * S; k += blockDim.x) {
            const int j = k / S, w = k - j * S, e = e0 + j;
            if (skip(e)) continue;
            const int8_t v = (int8_t)bytes[(size_t)j * Sw * 4 + w];
            base0(e)[w] = v;
            if (dst1 && !term[e]) dst1[(size_t)e * stride1 + w] = v;
        }
    }
}

constexpr size_t kGlobalObsMaxBytes = 64 * 1024;  // one chip's state row must fit a workgroup's LDS tile

__global__ void k_set_word(int *dst, int v) { *dst = v; }  // DevPtrs::dflags, stream-ordered and graph-capturable

// python round(): half-to-even on the double value (dmfb.py:444-453)
int zoom_one(int d, int hf, int size) {
    if (std::abs(d) > hf) {
        const double scale = (double)(size - hf) / (double)(10 - hf);
        if (d > 0) return (int)std::nearbyint((double)(d - hf) / scale) + hf;
        return (int)std::nearbyint((double)(d + hf) / scale) - hf;
    }
    return d;
}

}  // namespace

struct dmfb_vec {
    dmfb_vec_config cfg;
    DevCfg dc;
    DevPtrs dp;
    int8_t zoom_host[2 * 511];
    int8_t *zoom_dev = nullptr;
    unsigned long long *band_dev = nullptr;  // DevPtrs::band
    int *dflags_dev = nullptr;               // DevPtrs::dflags
    int obs_per_cu = 0;                      // cap on k_observe's persistent workgroups per CU (0: as many as LDS admits)
    size_t bytes = 0;
    int T_fused = 16;    // chips per workgroup of the fused step+observe launch (<= 64)
    int T_obs = 16;      // chips per workgroup of k_observe
    int split_min = 0;   // batches of at least this many chips use the step-only + observe pair
    int T_min = 16;      // smallest tile pick_tile may choose (DMFB_VEC_MIN_TILE); smaller tiles do not pay off (measured)
    int n_cu = 256;      // compute units of the device (persistent grid of the observation kernel)
    mutable ObserveTiming timing;            // dmfb_vec_observe_timing
};

namespace {

// LDS of the usage histograms (one per wave) of a kernel that may fold usage logs into the maps
size_t hist_lds(const dmfb_vec *h) { return h->dp.health ? (size_t)(kBlock / kWave) * h->dc.hist_bytes : 0; }

// chips up to this many cells count a usage log through an LDS histogram; larger ones use global atomics
constexpr int kHistMaxCells = 4096;

// 8-byte words per band image: the fov*fov layer bytes, padded so that the kernel reads them in batches of 12
int band_words(int fov) { return ((fov * fov + 7) / 8 + 11) / 12 * 12; }

// Tile of the LDS-staged observation: at most 64 chips (wave 0 owns one chip per lane in the fused launch),
// obs block <= 40 KB so that >= 3-4 workgroups share a CU's 160 KiB, and halved while the grid would not
// cover the 256 CUs `min_groups`/256 times over (any tile size works: the tile is phase-aligned in LDS).
int pick_tile(const dmfb_vec *h, int min_groups) {
    const int row = h->cfg.n_agents * h->dc.obs_len;
    int T = 64;
    size_t cap = 40 * 1024;
    if (const char *v = getenv("DMFB_VEC_TILE_KB")) cap = (size_t)atoi(v) * 1024;  // tuning knob
    while (T > 1 && ((size_t)T * row > cap || tile_lds_bytes(T, h->cfg.n_agents, h->dc.obs_len, true, table_words(h->dc.hf, h->dc.nq)) + hist_lds(h) > 64 * 1024)) T >>= 1;
    while (T > h->T_min && (h->cfg.n_envs + T - 1) / T < min_groups) T >>= 1;
    return T;
}

constexpr int kStepOnlyTile = 256;  // step-only launch: every wave of the workgroup owns 64 chips


template <int N> int observe_n(const dmfb_vec *h, const uint8_t *mask, int8_t *obs, hipStream_t s) {
    const int T = h->T_obs;
    const size_t lds = tile_lds_bytes(T, N, h->dc.obs_len, true, table_words(h->dc.hf, h->dc.nq));
    const int grid = persistent_grid(lds, (h->cfg.n_envs + T - 1) / T, h->n_cu, h->obs_per_cu);
    hipEvent_t t0 = nullptr, t1 = nullptr;
    h->timing.slot(t0, t1);
    HIP_TRY(launch_observe_n<N>(h->dc, h->dp, mask, obs, grid, lds, s, t0, t1));
    return DMFB_OK;
}

// One fused launch for small batches (launch latency dominates); for large batches a step-only launch
// (all four waves stepping, no LDS tile, high occupancy) followed by the observation kernel.
// step-only launch (no observation tile): one lane per chip, 256 chips per workgroup
template <int N> int step_only_n(dmfb_vec *h, const StepArgs &b, hipStream_t s) {
    const int E = h->cfg.n_envs;
    DevCfg c = h->dc;
    c.T = kStepOnlyTile;
    HIP_TRY(launch_step_n<N>(c, h->dp, b, (E + c.T - 1) / c.T, tile_lds_bytes(c.T, N, c.obs_len, false, 0) + hist_lds(h), s));
    return DMFB_OK;
}

template <int N> int step_n(dmfb_vec *h, const StepArgs &a, hipStream_t s) {
    const int E = h->cfg.n_envs;
    if (a.out.d_obs_terminal && (!a.out.d_obs || E >= h->split_min || !(a.flags & DMFB_STEP_AUTORESET))) return DMFB_ERR_UNSUPPORTED;
    if (a.out.d_obs && E >= h->split_min) {
        StepArgs b = a;
        b.out.d_obs = nullptr;
        const int rc = step_only_n<N>(h, b, s);
        if (rc) return rc;
        return observe_n<N>(h, nullptr, a.out.d_obs, s);
    }
    if (!a.out.d_obs) return step_only_n<N>(h, a, s);
    DevCfg c = h->dc;
    const bool with_obs = a.out.d_obs != nullptr;
    c.T = with_obs ? h->T_fused : kStepOnlyTile;
    HIP_TRY(launch_step_n<N>(c, h->dp, a, (E + c.T - 1) / c.T,
                             tile_lds_bytes(c.T, N, c.obs_len, with_obs, table_words(c.hf, c.nq)) + hist_lds(h), s));
    return DMFB_OK;
}
template <int N> int reset_n(dmfb_vec *h, const uint8_t *mask, int mode, hipStream_t s) {
    HIP_TRY(launch_reset_n<N>(h->dc, h->dp, mask, mode, (h->cfg.n_envs + (kBlock / kWave) - 1) / (kBlock / kWave),
                              (size_t)(kBlock / kWave) * h->dc.hist_bytes, s));
    return DMFB_OK;
}

#define DISPATCH_N(n, FN, ...)                                  \
    switch (n) {                                                \
    case 1: return FN<1>(__VA_ARGS__);                          \
    case 2: return FN<2>(__VA_ARGS__);                          \
    case 3: return FN<3>(__VA_ARGS__);                          \
    case 4: return FN<4>(__VA_ARGS__);                          \
    case 5: return FN<5>(__VA_ARGS__);                          \
    case 6: return FN<6>(__VA_ARGS__);                          \
    case 7: return FN<7>(__VA_ARGS__);                          \
    case 8: return FN<8>(__VA_ARGS__);                          \
    case 9: return FN<9>(__VA_ARGS__);                          \
    case 10: return FN<10>(__VA_ARGS__);                        \
    case 11: return FN<11>(__VA_ARGS__);                        \
    case 12: return FN<12>(__VA_ARGS__);                        \
    case 13: return FN<13>(__VA_ARGS__);                        \
    case 14: return FN<14>(__VA_ARGS__);                        \
    case 15: return FN<15>(__VA_ARGS__);                        \
    case 16: return FN<16>(__VA_ARGS__);                        \
    default: return DMFB_ERR_UNSUPPORTED;                       \
    }

int launch_step(dmfb_vec *h, const StepArgs &a, hipStream_t s) { DISPATCH_N(h->cfg.n_agents, step_n, h, a, s) }
int launch_observe(const dmfb_vec *h, const uint8_t *mask, int8_t *obs, hipStream_t s) {
    DISPATCH_N(h->cfg.n_agents, observe_n, h, mask, obs, s)
}
int launch_reset(dmfb_vec *h, const uint8_t *mask, int mode, hipStream_t s) {
    DISPATCH_N(h->cfg.n_agents, reset_n, h, mask, mode, s)
}

// dmfb_vec_create past the argument checks, on the handle's device; the caller destroys the handle when this fails
int init(dmfb_vec *h, hipStream_t s) {
    const dmfb_vec_config *cfg = &h->cfg;
    {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && v > 0) h->n_cu = v;
    }
    DevCfg &d = h->dc;
    d.W = cfg->width; d.L = cfg->length; d.fov = cfg->fov; d.hf = cfg->fov / 2; d.ff = cfg->fov * cfg->fov;
    d.obs_len = 3 * d.ff + 2; d.max_step = 2 * (cfg->width + cfg->length);
    d.nq = band_words(cfg->fov);
    d.stall = cfg->stall != 0; d.b_degrade = cfg->b_degrade != 0; d.E = cfg->n_envs; d.n = cfg->n_agents;
    d.k0 = (uint32_t)cfg->seed; d.k1 = (uint32_t)(cfg->seed >> 32); d.env_id0 = cfg->env_id0;
    d.per_healthy = 1.0 - cfg->per_degrade;
    const int E = cfg->n_envs, n = cfg->n_agents;
    const size_t cells = (size_t)cfg->width * cfg->length;
    const size_t st_bytes = (size_t)rec_words(n) * E * 4, starts_bytes = (size_t)((n + 1) / 2) * E * 4;
    memset(&h->dp, 0, sizeof(h->dp));
    HIP_TRY(hipMalloc(&h->dp.st, st_bytes));
    HIP_TRY(hipMalloc(&h->dp.starts, starts_bytes));
    h->bytes = st_bytes + starts_bytes;
    if (cfg->b_degrade || cfg->with_maps) {
        HIP_TRY(hipMalloc(&h->dp.health, cells * E * 8));
        HIP_TRY(hipMalloc(&h->dp.degrade, cells * E * 8));
        HIP_TRY(hipMalloc(&h->dp.usage, cells * E * 2 + 4));  // + 4: the 32-bit atomics of the large-chip path stay in bounds
        d.ucap = d.max_step;
        HIP_TRY(hipMalloc(&h->dp.ulog, (size_t)E * d.ucap * kLogStride * 2));
        HIP_TRY(hipMalloc(&h->dp.kmap, kmap_bytes(cells) * E));
        HIP_TRY(hipMalloc(&h->dflags_dev, 4));
        h->dp.dflags = h->dflags_dev;
        LAUNCH(k_set_word, dim3(1), dim3(1), 0, s, h->dflags_dev, 1);  // until health or degrade is replaced (set_map)
        d.hist_bytes = (int)cells <= kHistMaxCells ? (int)((cells * 2 + 15) & ~(size_t)15) : 0;
        h->bytes += cells * E * 18 + kmap_bytes(cells) * E + (size_t)E * d.ucap * kLogStride * 2;
    }
    // GenRandomBlocks guards (dmfb.py:230-234): no blocks on tiny chips or above 20 % coverage
    d.nb = cfg->n_blocks;
    if (cfg->width < 5 || cfg->length < 5 || (double)(cfg->n_blocks * 4) / (double)(cfg->width * cfg->length) > 0.2) d.nb = 0;
    if (cfg->n_blocks > 0) {
        HIP_TRY(hipMalloc(&h->dp.blocks, (size_t)cfg->n_blocks * E * 4));
        HIP_TRY(hipMemsetAsync(h->dp.blocks, 0, (size_t)cfg->n_blocks * E * 4, s));
        h->bytes += (size_t)cfg->n_blocks * E * 4;
    }
    for (int dd = -255; dd <= 255; ++dd) {
        int zx = dd, zy = dd;
        if (d.hf != 10) { zx = zoom_one(dd, d.hf, d.W); zy = zoom_one(dd, d.hf, d.L); }
        h->zoom_host[dd + 255] = (int8_t)zx;
        h->zoom_host[511 + dd + 255] = (int8_t)zy;
    }
    HIP_TRY(hipMalloc(&h->zoom_dev, sizeof(h->zoom_host)));
    h->bytes += sizeof(h->zoom_host);
    HIP_TRY(hipMemcpyAsync(h->zoom_dev, h->zoom_host, sizeof(h->zoom_host), hipMemcpyHostToDevice, s));
    h->dp.zoom = h->zoom_dev;
    {   // observation tables (DevPtrs::band): band images [axis][pattern][nq], then the zoom table
        const int fov = d.fov, hf = d.hf, ff = d.ff, npat = 2 * hf + 1;
        const size_t words = (size_t)table_words(hf, d.nq);
        unsigned long long *img = new (std::nothrow) unsigned long long[words]();
        if (!img) return DMFB_ERR_BAD_ARG;
        for (int axis = 0; axis < 2; ++axis)
            for (int pat = 1; pat < npat; ++pat) {
                unsigned char *bytes = (unsigned char *)(img + ((size_t)axis * npat + pat) * d.nq);
                for (int b = 0; b < ff; ++b) {
                    const int v = axis == 0 ? b / fov : b % fov;  // window x (first axis) or y
                    // pattern p <= hf: the first p window rows/columns lie outside the chip (obs[2, 0:left, :] = 1,
                    // dmfb.py:430-431); p > hf: the last p - hf ones (obs[2, -right:, :] = 1, dmfb.py:432-433)
                    if (pat <= hf ? v < pat : v >= fov - (pat - hf)) bytes[b] = 1;
                }
            }
        memcpy(img + (size_t)2 * npat * d.nq, h->zoom_host, sizeof(h->zoom_host));
        hipError_t e1 = hipMalloc(&h->band_dev, words * 8);
        if (e1 == hipSuccess) e1 = hipMemcpy(h->band_dev, img, words * 8, hipMemcpyHostToDevice);
        delete[] img;
        if (e1 != hipSuccess) { hip_fail(e1, "observation table upload", __LINE__); return DMFB_ERR_HIP; }
        h->bytes += words * 8;
        h->dp.band = h->band_dev;
    }
    HIP_TRY(hipMemsetAsync(h->dp.st, 0, st_bytes, s));
    d.fov_magic = d.fov >= 2 ? (uint32_t)((0x100000000ull + (uint64_t)d.fov - 1) / (uint64_t)d.fov) : 0u;
    if (const char *v = getenv("DMFB_VEC_MIN_TILE")) h->T_min = atoi(v) > 0 ? atoi(v) : 1;  // tuning knob
    h->T_fused = pick_tile(h, 1024);
    h->T_obs = pick_tile(h, 2048);
    {   // observation kernel: at most 128 rows per tile, so that the two half-workgroups (layer 0 | layer 1, first | second half
        // of the band image) each cover every row in one pass
        int t = 128 / n;
        t = t < 1 ? 1 : (t > 64 ? 64 : t);
        while (t > 1 && tile_lds_bytes(t, n, d.obs_len, true, table_words(d.hf, d.nq)) > 64 * 1024) --t;
        while (t > h->T_min && (E + t - 1) / t < 1024) t = (t + 1) / 2;
        h->T_obs = t;
    }
    if (const char *v = getenv("DMFB_VEC_OBS_TILE")) {  // tuning knob: chips per workgroup of the observation kernel (1..64)
        const int t = atoi(v);
        if (t >= 1 && t <= 64 && tile_lds_bytes(t, n, d.obs_len, true, table_words(d.hf, d.nq)) <= 64 * 1024) h->T_obs = t;
    }
    d.T = h->T_fused; d.T_obs = h->T_obs;
    for (uint32_t k = 0; k < 64u * DMFB_MAX_AGENTS * (uint32_t)d.fov && d.fov >= 2; ++k)  // the magic must be exact on the range used
        if ((uint32_t)(((uint64_t)k * d.fov_magic) >> 32) != k / (uint32_t)d.fov) return DMFB_ERR_UNSUPPORTED;
    h->split_min = 32768;
    if (const char *v = getenv("DMFB_VEC_SPLIT_MIN_ENVS")) h->split_min = atoi(v);  // tuning / test knob
    if (const char *v = getenv("DMFB_VEC_OBS_PER_CU")) h->obs_per_cu = atoi(v);       // tuning knob: persistent workgroups per CU of k_observe
    const int rc = launch_reset(h, nullptr, 3, s);
    if (rc) return rc;
    // the zoom table upload reads host memory owned by the handle: make it safe to use right away
    HIP_TRY(hipStreamSynchronize(s));
    return DMFB_OK;
}

}  // namespace

extern "C" {

int dmfb_vec_check_config(const dmfb_vec_config *c) {
    if (!c) return DMFB_ERR_BAD_ARG;
    if (c->width < 5 || c->length < 5) return DMFB_ERR_CHIP_TOO_SMALL;
    if (c->n_agents <= 0) return DMFB_ERR_NO_AGENTS;
    if (c->fov > (c->width < c->length ? c->width : c->length)) return DMFB_ERR_FOV_TOO_LARGE;
    if (c->n_agents > (int)((c->width + 1) * (c->length + 1) / 9)) return DMFB_ERR_TOO_MANY_DROPLETS;
    if (c->n_agents > DMFB_MAX_AGENTS || c->width > DMFB_MAX_DIM || c->length > DMFB_MAX_DIM || c->fov < 1 ||
        c->n_blocks < 0 || c->n_blocks > DMFB_MAX_BLOCKS)
        return DMFB_ERR_UNSUPPORTED;
    if (c->n_envs <= 0) return DMFB_ERR_BAD_ARG;
    if (tile_lds_bytes(1, c->n_agents, 3 * c->fov * c->fov + 2, true, table_words(c->fov / 2, band_words(c->fov))) > 64 * 1024)
        return DMFB_ERR_UNSUPPORTED;
    return DMFB_OK;
}

int dmfb_vec_create(const dmfb_vec_config *cfg, void *stream, dmfb_vec **out) {
    if (!out) return DMFB_ERR_BAD_ARG;
    int rc = dmfb_vec_check_config(cfg);
    if (rc) return rc;
    DeviceGuard g(cfg->device);
    if (!g.ok) return DMFB_ERR_HIP;
    dmfb_vec *h = new (std::nothrow) dmfb_vec();
    if (!h) return DMFB_ERR_BAD_ARG;
    h->cfg = *cfg;
    rc = init(h, (hipStream_t)stream);
    if (rc) {
        dmfb_vec_destroy(h);
        return rc;
    }
    *out = h;
    return DMFB_OK;
}

int dmfb_vec_destroy(dmfb_vec *h) {
    if (h)
        destroy_handle(h, h->dp.st, h->dp.starts, h->dp.health, h->dp.degrade, h->dp.usage, h->dp.ulog, h->dp.kmap, h->zoom_dev,
                       h->dp.blocks, h->band_dev, h->dflags_dev);
    return DMFB_OK;
}

size_t dmfb_vec_state_bytes(const dmfb_vec *h) { return h ? h->bytes : 0; }
int dmfb_vec_obs_len(const dmfb_vec *h) { return h ? h->dc.obs_len : DMFB_ERR_BAD_ARG; }
int dmfb_vec_max_step(const dmfb_vec *h) { return h ? h->dc.max_step : DMFB_ERR_BAD_ARG; }
int dmfb_vec_n_envs(const dmfb_vec *h) { return h ? h->cfg.n_envs : DMFB_ERR_BAD_ARG; }
int dmfb_vec_n_agents(const dmfb_vec *h) { return h ? h->cfg.n_agents : DMFB_ERR_BAD_ARG; }

int dmfb_vec_reset(dmfb_vec *h, const uint8_t *d_mask, int new_flag, int8_t *d_obs, void *stream) {
    if (!h) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    int rc = launch_reset(h, d_mask, new_flag ? 1 : 0, (hipStream_t)stream);
    if (!rc && new_flag && !d_mask && h->dp.health) {  // every map is the generator's own again
        LAUNCH(k_set_word, dim3(1), dim3(1), 0, (hipStream_t)stream, h->dflags_dev, 1);
    }
    if (rc || !d_obs) return rc;
    return launch_observe(h, d_mask, d_obs, (hipStream_t)stream);
}

int dmfb_vec_restart(dmfb_vec *h, const uint8_t *d_mask, int8_t *d_obs, void *stream) {
    if (!h) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    int rc = launch_reset(h, d_mask, 2, (hipStream_t)stream);
    if (rc || !d_obs) return rc;
    return launch_observe(h, d_mask, d_obs, (hipStream_t)stream);
}

int dmfb_vec_set_task(dmfb_vec *h, const int32_t *d_starts, const int32_t *d_ends, void *stream) {
    if (!h || !d_starts || !d_ends) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    LAUNCH(k_set_task, dim3((h->cfg.n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->dc, h->dp,
           d_starts, d_ends);
    return DMFB_OK;
}

int dmfb_vec_get_task(const dmfb_vec *h, int32_t *d_starts, int32_t *d_ends, void *stream) {
    if (!h) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    LAUNCH(k_get_task, dim3((h->cfg.n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->dc, h->dp,
           d_starts, d_ends);
    return DMFB_OK;
}

int dmfb_vec_set_blocks(dmfb_vec *h, const int32_t *d_blocks, int nb, void *stream) {
    if (!h || nb < 0 || nb > h->cfg.n_blocks || (nb > 0 && !d_blocks)) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    h->dc.nb = nb;
    if (nb == 0) return DMFB_OK;
    LAUNCH(k_set_blocks, dim3((h->cfg.n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->dc, h->dp,
           d_blocks, nb);
    return DMFB_OK;
}

int dmfb_vec_get_blocks(const dmfb_vec *h, int32_t *d_blocks, int *nb_out, void *stream) {
    if (!h) return DMFB_ERR_BAD_ARG;
    if (nb_out) *nb_out = h->dc.nb;
    if (!d_blocks || h->dc.nb == 0) return DMFB_OK;
    DeviceGuard g(h->cfg.device);
    LAUNCH(k_get_blocks, dim3((h->cfg.n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->dc, h->dp,
           d_blocks, h->cfg.n_blocks);
    return DMFB_OK;
}

int dmfb_vec_step(dmfb_vec *h, const void *d_actions, const double *d_uniforms, const uint8_t *d_active,
                  uint32_t flags, const dmfb_vec_step_out *out, void *stream) {
    if (!h || !d_actions || !out) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    StepArgs a;
    a.actions = d_actions; a.uniforms = d_uniforms; a.active = d_active; a.flags = flags; a.out = *out;
    return launch_step(h, a, (hipStream_t)stream);
}

int dmfb_vec_observe(const dmfb_vec *h, const uint8_t *d_mask, int8_t *d_obs, void *stream) {
    if (!h || !d_obs) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    return launch_observe(h, d_mask, d_obs, (hipStream_t)stream);
}

int dmfb_vec_state_len(const dmfb_vec *h) { return h ? 3 * h->cfg.width * h->cfg.length : DMFB_ERR_BAD_ARG; }

}  // extern "C"

namespace {
int launch_global_obs(const dmfb_vec *h, const uint8_t *sel, const uint8_t *term, int8_t *dst0, size_t stride0, int8_t *dst1,
                      size_t stride1, hipStream_t s, const int32_t *t_row = nullptr, int T = 0) {
    const size_t S = 3 * (size_t)h->cfg.width * h->cfg.length, row = (S + 3) / 4 * 4;
    if (row > kGlobalObsMaxBytes) return DMFB_ERR_UNSUPPORTED;
    const int G = (int)std::max<size_t>(1, std::min<size_t>(64, 16384 / row));
    const int E = h->cfg.n_envs;
    const bool words = S % 4 == 0 && (uintptr_t)dst0 % 4 == 0 && (!dst1 || (uintptr_t)dst1 % 4 == 0) && stride0 % 4 == 0 &&
                       stride1 % 4 == 0;
    static LdsLimit lds;
    if (G * row > 64 * 1024) {
        int rc = lds.raise((const void *)k_global_obs, G * row);
        if (rc) return rc;
    }
    LAUNCH(k_global_obs, dim3((E + G - 1) / G), dim3(256), G * row, s, h->dc, h->dp, G, sel, term, dst0, stride0, dst1, stride1,
           (int)words, t_row, T);
    return DMFB_OK;
}
}  // namespace

extern "C" {

int dmfb_vec_global_obs(const dmfb_vec *h, const uint8_t *d_mask, int8_t *d_out, void *stream) {
    if (!h || !d_out) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    const size_t S = 3 * (size_t)h->cfg.width * h->cfg.length;
    return launch_global_obs(h, d_mask, nullptr, d_out, S, nullptr, 0, (hipStream_t)stream);
}

int dmfb_vec_global_obs_append(const dmfb_vec *h, const uint8_t *d_alive, const uint8_t *d_term, int32_t t, int32_t T, int8_t *d_s,
                               int8_t *d_s_next, void *stream) {
    if (!h || !d_alive || !d_term || !d_s || !d_s_next || t < 0 || t >= T) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    const size_t S = 3 * (size_t)h->cfg.width * h->cfg.length;
    int8_t *s1 = t + 1 < T ? d_s + (size_t)(t + 1) * S : nullptr;
    return launch_global_obs(h, d_alive, d_term, d_s_next + (size_t)t * S, (size_t)T * S, s1, (size_t)T * S, (hipStream_t)stream);
}

int dmfb_vec_global_obs_stage_first(const dmfb_vec *h, const uint8_t *d_mask, int32_t T, int8_t *d_stage, void *stream) {
    if (!h || !d_stage || T < 1) return DMFB_ERR_BAD_ARG;
    const size_t S = 3 * (size_t)h->cfg.width * h->cfg.length;
    if ((S + 3) / 4 * 4 > kGlobalObsMaxBytes) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    return launch_global_obs(h, d_mask, nullptr, d_stage, (size_t)(T + 1) * S, nullptr, 0, (hipStream_t)stream);
}

int dmfb_vec_global_obs_stage_close(const dmfb_vec *h, const int32_t *d_t_ep, const int32_t *d_close_slot, int32_t T,
                                    int8_t *d_stage, int8_t *d_ring_s, int32_t slots, void *stream) {
    if (!h || !d_t_ep || !d_close_slot || !d_stage || !d_ring_s || T < 1 || slots < h->cfg.n_envs) return DMFB_ERR_BAD_ARG;
    const size_t S = 3 * (size_t)h->cfg.width * h->cfg.length;
    if ((S + 3) / 4 * 4 > kGlobalObsMaxBytes) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    const hipStream_t s = (hipStream_t)stream;
    // stage[e][t + 1] = state(e) with t = d_t_ep[e] (k_global_obs with a per-chip destination row) ...
    int rc = launch_global_obs(h, nullptr, nullptr, d_stage, (size_t)(T + 1) * S, nullptr, 0, s, d_t_ep, T);
    if (rc) return rc;
    // ... then the rows of the closing chips into their ring slots, spread over the grid
    return launch_state_close(h->cfg.n_envs, T, S, slots, h->n_cu, d_t_ep, d_close_slot, d_stage, d_ring_s, s);
}

int dmfb_vec_get_state(const dmfb_vec *h, int32_t *d_pos, int32_t *d_dist, int32_t *d_step_count,
                       int64_t *d_constraints, void *stream) {
    if (!h) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    LAUNCH(k_get_state, dim3((h->cfg.n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->dc, h->dp,
           d_pos, d_dist, d_step_count, d_constraints);
    return DMFB_OK;
}

int dmfb_vec_route_append(const dmfb_vec *h, int32_t t, int32_t T, uint8_t *d_route, void *stream) {
    if (!h || !d_route || ((uintptr_t)d_route & 1) || T < 1 || t < -1 || t >= T) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    const long lanes = (long)h->cfg.n_envs * h->cfg.n_agents;
    LAUNCH(k_route_append, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->dc, h->dp, t + 1, T,
           (uint16_t *)d_route);
    return DMFB_OK;
}

int dmfb_vec_shield(const dmfb_vec *h, const float *d_q, const uint8_t *d_active, int32_t *d_actions, int8_t *d_last_onehot,
                    int8_t *d_ep_u, int8_t *d_ep_onehot, int32_t episode_limit, int32_t t, const int32_t *d_t_ep,
                    int32_t *d_overrides, uint8_t *d_unsafe, void *stream) {
    if (!h || !d_q || !d_actions || !d_last_onehot || (d_ep_u == nullptr) != (d_ep_onehot == nullptr)) return DMFB_ERR_BAD_ARG;
    if (d_ep_u && (episode_limit < 1 || (!d_t_ep && (t < 0 || t >= episode_limit)))) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    ShieldArgs a;
    a.q = d_q; a.active = d_active; a.actions = d_actions; a.last_onehot = d_last_onehot; a.ep_u = d_ep_u; a.ep_onehot = d_ep_onehot;
    a.T = episode_limit; a.t = t; a.t_ep = d_t_ep; a.overrides = d_overrides; a.unsafe = d_unsafe;
    const long lanes = (long)h->cfg.n_envs * kShieldLanes;
    LAUNCH(k_shield, dim3((unsigned)((lanes + kShieldBlock - 1) / kShieldBlock)), dim3(kShieldBlock), 0, (hipStream_t)stream, h->dc,
           h->dp, a);
    return DMFB_OK;
}

int dmfb_vec_get_map(const dmfb_vec *h, int which, double *d_buf, void *stream) {
    if (!h || !d_buf || which < 0 || which > 2) return DMFB_ERR_BAD_ARG;
    if (!h->dp.health) return DMFB_ERR_NO_MAPS;
    DeviceGuard g(h->cfg.device);
    const size_t total = (size_t)h->cfg.n_envs * h->cfg.width * h->cfg.length;
    if (which == DMFB_MAP_USAGE) {  // the steps since the last reset are still in the usage log
        LAUNCH(k_flush_usage, dim3((h->cfg.n_envs + (kBlock / kWave) - 1) / (kBlock / kWave)), dim3(kBlock), hist_lds(h),
               (hipStream_t)stream, h->dc, h->dp);
    }
    LAUNCH(k_get_map, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, total,
           h->dp.health, h->dp.degrade, h->dp.usage, which, d_buf);
    return DMFB_OK;
}

int dmfb_vec_set_map(dmfb_vec *h, int which, const double *d_buf, void *stream) {
    if (!h || !d_buf || which < 0 || which > 2) return DMFB_ERR_BAD_ARG;
    if (!h->dp.health) return DMFB_ERR_NO_MAPS;
    DeviceGuard g(h->cfg.device);
    const size_t total = (size_t)h->cfg.n_envs * h->cfg.width * h->cfg.length;
    if (which != DMFB_MAP_USAGE) {  // health / degrade no longer follow from the generator: gather the float64 map
        LAUNCH(k_set_word, dim3(1), dim3(1), 0, (hipStream_t)stream, h->dflags_dev, 0);
    }
    if (which == DMFB_MAP_USAGE) {  // pending log entries belong to the map that is being replaced: fold them in first
        LAUNCH(k_flush_usage, dim3((h->cfg.n_envs + (kBlock / kWave) - 1) / (kBlock / kWave)), dim3(kBlock), hist_lds(h),
               (hipStream_t)stream, h->dc, h->dp);
    }
    LAUNCH(k_set_map, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, total,
           h->dp.health, h->dp.degrade, h->dp.usage, which, d_buf);
    return DMFB_OK;
}

int dmfb_vec_launch_shape(const dmfb_vec *h, int32_t out[6]) {
    if (!h || !out) return DMFB_ERR_BAD_ARG;
    out[0] = h->T_fused; out[1] = h->T_obs; out[2] = h->split_min; out[3] = kStepOnlyTile;
    const size_t lds = tile_lds_bytes(h->T_obs, h->cfg.n_agents, h->dc.obs_len, true, table_words(h->dc.hf, h->dc.nq));
    out[4] = persistent_grid(lds, (h->cfg.n_envs + h->T_obs - 1) / h->T_obs, h->n_cu, h->obs_per_cu);
    out[5] = kObsBlock;
    return DMFB_OK;
}

int dmfb_vec_observe_timing(dmfb_vec *h, int enable) {
    if (!h) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    return h->timing.enable(enable);
}

int dmfb_vec_observe_timing_read(dmfb_vec *h, double *total_us, int *launches) {
    if (!h || !total_us || !launches) return DMFB_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    return h->timing.read(total_us, launches);
}

int dmfb_vec_zoom_lut(const dmfb_vec *h, int8_t *host_out) {
    if (!h || !host_out) return DMFB_ERR_BAD_ARG;
    memcpy(host_out, h->zoom_host, sizeof(h->zoom_host));
    return DMFB_OK;
}

const char *dmfb_vec_strerror(int code) {
    switch (code) {
    case DMFB_OK: return "ok";
    case DMFB_ERR_BAD_ARG: return "bad argument";
    case DMFB_ERR_FOV_TOO_LARGE: return "Fov is too large";
    case DMFB_ERR_TOO_MANY_DROPLETS: return "Too many droplets for DMFB";
    case DMFB_ERR_CHIP_TOO_SMALL: return "width >= 5 and length >= 5 required";
    case DMFB_ERR_NO_AGENTS: return "n_agents > 0 required";
    case DMFB_ERR_UNSUPPORTED: return "configuration outside the build limits";
    case DMFB_ERR_BAD_ACTION: return "action is illegal";
    case DMFB_ERR_NO_MAPS: return "handle was created without health/usage/degrade maps";
    case DMFB_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}

int dmfb_vec_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
