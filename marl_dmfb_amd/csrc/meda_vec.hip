// meda_vec.hip -- C ABI (include/meda_vec.h) of the vectorised MEDA environment, the LDS-staged
// observation kernel, map/task/state accessors and the dispatch to the per-N kernels built from
// meda_vec_n.hip.  Device code of the transition: meda_kernels.h.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "meda_kernels.h"
#include "meda_shield.h"

#define HIP_ABI_TAG "meda_vec"
#define HIP_ABI_ERR MEDA_ERR_HIP
#include "hip_abi.h"
#include "vec_env.h"

static_assert(MEDA_MAP_HEALTH == kMapHealth && MEDA_MAP_USAGE == kMapUsage && MEDA_MAP_DEGRADE == kMapDegrade, "map selectors");

using namespace medak;

namespace {

// ---- MEDAEnv.getOneObs (meda.py:613-674) and MEDAEnv_v0_2.getOneObs (meda.py:850-897), LDS-staged ----------
// Persistent workgroups (the grid covers the CUs a few times over; a workgroup walks tiles blockIdx.x,
// blockIdx.x + gridDim.x, ...).  A tile is T consecutive chips = T*n rows of obs_len bytes, built in LDS at the
// same 16-byte phase as its destination in HBM (shift = global offset & 15), so its body streams out with
// aligned 16-byte stores whatever T, n and fov are.
// Roles, as in dmfbk::k_observe: the LAST wave is the loader -- it alone reads global memory (droplet words, one
// chip per lane; the refresh mask) and never stores; the other waves stream finished tiles out and never load
// (gfx950 counts a wave's loads and stores in one in-order counter).  The droplet words run two tiles ahead:
// while tile k is filled, those of tile k+1 sit in the loader's registers; while tile k streams out they are
// written to the second word buffer and tile k+2 is requested.
// Rows are filled by waves, two rows per wave pass (lanes 0-24 and 32-56 each own one cell of a 5x5 footprint);
// a row is always written by ONE wave, and LDS operations of one wave complete in order, so for overlapping
// footprints the higher droplet index wins exactly as in the reference's sequential loops.
constexpr int kObsBlock = 256;
constexpr int kObsWork = kObsBlock - kWave;  // threads that stream tiles out

__host__ __device__ inline size_t obs_tile_area(int T, int row_bytes) { return ((size_t)T * row_bytes + 16 + 15) & ~(size_t)15; }
__host__ __device__ inline size_t obs_lds_bytes(int T, int n, int row_bytes) {
    return obs_tile_area(T, row_bytes) + 2 * (size_t)T * n * 4 + 2 * (((size_t)T + 15) & ~(size_t)15) + 512;
}

// One 5x5 footprint (value val, centre (x0, y0) in window coordinates) into a window layer [y][x]: every cell is
// clamped into the window.  For a footprint that touches the window this writes exactly its in-window cells (a cell
// outside lands on the window edge, which the footprint then covers); for a goal it is np.clip's smear (meda.py:665,
// 872).  The caller predicates footprints that miss the window entirely.
__device__ __forceinline__ void put5x5(int8_t *layer, int fov, int x0, int y0, int8_t val) {
    int xs[2 * kR + 1], ys[2 * kR + 1];
#pragma unroll
    for (int k = 0; k <= 2 * kR; ++k) {
        xs[k] = min(max(x0 + k - kR, 0), fov - 1);
        ys[k] = min(max(y0 + k - kR, 0), fov - 1) * fov;
    }
#pragma unroll
    for (int ky = 0; ky <= 2 * kR; ++ky)
#pragma unroll
        for (int kx = 0; kx <= 2 * kR; ++kx) layer[ys[ky] + xs[kx]] = val;
}
__device__ __forceinline__ bool touches(int x0, int y0, int fov) {  // some footprint cell inside the window
    return x0 + kR >= 0 && x0 - kR <= fov - 1 && y0 + kR >= 0 && y0 - kR <= fov - 1;
}

// Fill of one zeroed LDS tile (all waves of the workgroup): words = [tv*n] droplet words.  An item is one LAYER of
// one observation row and belongs to one lane, which writes that layer's droplets in the reference's order (later
// writes win, as in its sequential loops); waves are layer-uniform.  The v0_2 boundary bands are a phase of their
// own, one lane per window line, before a barrier.
__device__ __forceinline__ void fill_rows(const MCfg &c, int8_t *tile, const uint32_t *words, const int8_t *zoom, int tv, int tid) {
    const int n = c.n, fov = c.fov, ff = c.ff, hf = fov / 2;
    const int wave = tid / kWave, lane = tid % kWave;
    const int rows = tv * n;
    constexpr int kWaves = kObsBlock / kWave;
    if (c.version == 2) {
        // ---- MEDAEnv_v0_2.getOneObs (meda.py:850-897)
        // layer 2: boundary bands with the reference's axis mix-up (meda.py:880-890).  A bit per column, spread to one
        // byte per bit four columns at a time and OR-ed into the zeroed tile (lines are fov bytes long, so neighbouring
        // lanes share words: atomic OR)
        for (int it = tid; it < rows * fov; it += kObsBlock) {
            const int r = it / fov, wr = it - r * fov;
            const uint32_t wa = words[r];
            const int cx = wa & 0xff, cy = (wa >> 8) & 0xff;
            const int left = hf - cx, right = hf - (c.W - 1 - cx);
            const int up = hf - cy, down = hf - (c.L - 1 - cy);
            int c0 = 0, c1 = 0;
            if (up > 0) { c0 = 0; c1 = up < fov ? up : fov; }
            else if (down > 0) { c0 = fov - down < 0 ? 0 : fov - down; c1 = fov; }
            const bool full = left > 0 ? (wr < left) : (right > 0 ? (wr >= fov - right) : false);
            int8_t *dst = tile + (size_t)r * c.obs_len + 2 * ff + wr * fov;
            if (fov > 28) {  // wide windows: plain byte stores
                const int b0 = full ? 0 : c0, b1 = full ? fov : c1;
                for (int cc = b0; cc < b1; ++cc) dst[cc] = 1;
                continue;
            }
            const uint32_t colbits = full ? ((1u << fov) - 1u) : ((1u << c1) - (1u << c0));
            if (colbits) {
                const int ph = (int)((uintptr_t)dst & 3);
                uint32_t *w = (uint32_t *)(dst - ph);
                const unsigned long long bits = (unsigned long long)colbits << ph;
                for (int q = 0; q * 4 < fov + 3; ++q) {
                    const uint32_t v = ((uint32_t)((bits >> (4 * q)) & 15u) * 0x00204081u) & 0x01010101u;
                    if (v) atomicOr(w + q, v);
                }
            }
        }
        __syncthreads();  // the byte stores below may share a word with a band's atomic
        // waves 0,2: layer 0 + direction bytes; waves 1,3: layer 1
        const int layer = wave & 1;
        for (int r = (wave >> 1) * kWave + lane; r < rows; r += (kWaves / 2) * kWave) {
            const int s = r / n, a = r - s * n;
            const uint32_t wa = words[r];
            const int cx = wa & 0xff, cy = (wa >> 8) & 0xff, gxa = (wa >> 16) & 0xff, gya = wa >> 24;
            const int ox = cx - hf, oy = cy - hf;
            int8_t *row = tile + (size_t)r * c.obs_len;
            if (layer == 0) {
                for (int j = 0; j < n; ++j) {  // every droplet, ascending index
                    const uint32_t wj = words[s * n + j];
                    const int x0 = (int)(wj & 0xff) - ox, y0 = (int)((wj >> 8) & 0xff) - oy;
                    if (touches(x0, y0, fov)) put5x5(row, fov, x0, y0, (int8_t)(j + 1));
                }
                row[3 * ff] = zoom[gya - cy + 128];
                row[3 * ff + 1] = zoom[256 + gxa - cx + 128];
                continue;
            }
            // members of the `observed` set: droplets with at least one footprint cell inside the window
            uint32_t obs_mask = 0;
            for (int j = 0; j < n; ++j) {
                const uint32_t wj = words[s * n + j];
                obs_mask |= (uint32_t)touches((int)(wj & 0xff) - ox, (int)((wj >> 8) & 0xff) - oy, fov) << j;
            }
            // iteration order of the CPython set (see oracle/meda_oracle.c): ascending once it has had 5
            // members (table resized to 32 slots), else slot order of the 8-slot table
            unsigned long long order = 0;  // 4-bit entries
            int cnt = 0;
            if (__popc(obs_mask) >= 5) {
                for (int j = 0; j < n; ++j)
                    if ((obs_mask >> j) & 1) { order |= (unsigned long long)j << (4 * cnt); ++cnt; }
            } else {
                unsigned long long slots = 0;  // 8 x (valid bit | 4-bit value)
                for (int j = 0; j < n; ++j)
                    if ((obs_mask >> j) & 1) {
                        int i = j & 7;
                        while ((slots >> (5 * i)) & 16) i = (i * 5 + 1) & 7;
                        slots |= (unsigned long long)(16 | j) << (5 * i);
                    }
                for (int i = 0; i < 8; ++i)
                    if ((slots >> (5 * i)) & 16) { order |= ((slots >> (5 * i)) & 15) << (4 * cnt); ++cnt; }
            }
            for (int tt = 0; tt < cnt; ++tt) {  // clipped goals of the observed OTHER droplets, in set order
                const int j = (int)((order >> (4 * tt)) & 15);
                if (j == a) continue;
                const uint32_t wj = words[s * n + j];
                put5x5(row + ff, fov, (int)((wj >> 16) & 0xff) - ox, (int)(wj >> 24) - oy, (int8_t)(j + 1));
            }
        }
        return;
    }
    // ---- MEDAEnv.getOneObs (meda.py:613-674): wave = layer
    const int layer = wave;
    for (int r = lane; r < rows; r += kWave) {
        const int s = r / n, a = r - s * n;
        const uint32_t wa = words[r];
        const int cx = wa & 0xff, cy = (wa >> 8) & 0xff, gxa = (wa >> 16) & 0xff, gya = wa >> 24;
        const int ox = cx - hf, oy = cy - hf;
        int8_t *row = tile + (size_t)r * c.obs_len;
        if (layer == 0) {  // own footprint, direction
            put5x5(row, fov, hf, hf, (int8_t)(a + 1));
            row[4 * ff] = (int8_t)(gxa - cx);
            row[4 * ff + 1] = (int8_t)(gya - cy);
        } else if (layer == 1) {  // own goal, in-window cells only
            if (touches(gxa - ox, gya - oy, fov)) put5x5(row + ff, fov, gxa - ox, gya - oy, (int8_t)(a + 1));
        } else {  // 2: the OTHER droplets (in-window cells); 3: their goals, smeared onto the window edge; ascending index
            for (int j = 0; j < n; ++j) {
                if (j == a) continue;
                const uint32_t wj = words[s * n + j];
                if (layer == 2) {
                    const int x0 = (int)(wj & 0xff) - ox, y0 = (int)((wj >> 8) & 0xff) - oy;
                    if (touches(x0, y0, fov)) put5x5(row + 2 * ff, fov, x0, y0, (int8_t)(j + 1));
                } else {
                    put5x5(row + 3 * ff, fov, (int)((wj >> 16) & 0xff) - ox, (int)(wj >> 24) - oy, (int8_t)(j + 1));
                }
            }
        }
    }
}

template <int NW>  // droplet words the loader keeps per chip: n <= NW
__global__ __launch_bounds__(kObsBlock) void k_meda_observe(MCfg c, MPtrs p, const uint8_t *mask, int8_t *gobs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int T = c.T, E = c.E, n = c.n;
    const int tid = threadIdx.x;
    const bool loader = tid >= kObsWork;
    const int ltid = tid - kObsWork;
    const int ntiles = (E + T - 1) / T;
    const int row_bytes = n * c.obs_len;
    uint32_t *const wbuf = (uint32_t *)(smem + obs_tile_area(T, row_bytes));  // [2][T*n] droplet words
    uint8_t *const fbuf = (uint8_t *)(wbuf + 2 * (size_t)T * n);               // [2][align16(T)] refresh flags
    const int fstride = (T + 15) & ~15;
    const int8_t *const zoom = (const int8_t *)(fbuf + 2 * fstride);           // LDS copy of MPtrs::zoom (v0_2 only)
    uint32_t rec[NW];
    auto prefetch = [&](int tile) {  // unconditional loads from clamped (always valid) addresses: nothing to wait for here
        const int base = tile < ntiles ? tile * T : 0;
        const int chip = min(base + ltid, E - 1);
#pragma unroll
        for (int w = 0; w < NW; ++w) rec[w] = p.st[(size_t)min(w, n - 1) * E + chip];
    };
    auto unpack = [&](int tile, uint32_t *dst) {
        if (tile >= ntiles || ltid >= min(T, E - tile * T)) return;
#pragma unroll
        for (int w = 0; w < NW; ++w)
            if (w < n) dst[ltid * n + w] = rec[w];
    };
    int tile = blockIdx.x, buf = 0;
    if (loader) {
        prefetch(tile);
        if (c.version == 2)
            for (int i = ltid; i < 128; i += kWave) ((uint32_t *)zoom)[i] = ((const uint32_t *)p.zoom)[i];
        unpack(tile, wbuf);
        prefetch(tile + gridDim.x);
    }
    for (; tile < ntiles; tile += gridDim.x, buf ^= 1) {
        const int tile_base = tile * T;
        const int tv = min(T, E - tile_base);
        const size_t g0 = (size_t)tile_base * row_bytes;
        const int shift = (int)(((uintptr_t)gobs + g0) & 15);
        const int bytes = tv * row_bytes;
        int8_t *const tile_lds = (int8_t *)smem + shift;
        const uint32_t *const words = wbuf + (size_t)buf * T * n;
        uint8_t *const flag = fbuf + buf * fstride;
        // this barrier publishes the words written during the previous tile's stream-out and separates that
        // stream-out (LDS reads) from the zero fill below; the loader's lanes flag and count the chips to refresh
        bool refresh = false;
        if (loader && ltid < tv) {
            refresh = !mask || mask[tile_base + ltid] != 0;
            flag[ltid] = (uint8_t)refresh;
        }
        const int cnt = __syncthreads_count(refresh);
        if (cnt != 0) {  // (uniform) something to refresh in this tile
            uint4 *z = (uint4 *)smem;
            const uint4 zero = make_uint4(0, 0, 0, 0);
            for (int i = tid; i < (shift + bytes + 15) / 16; i += kObsBlock) z[i] = zero;
            __syncthreads();
            fill_rows(c, tile_lds, words, zoom, tv, tid);
            __syncthreads();
        }
        if (loader) {
            unpack(tile + gridDim.x, wbuf + (size_t)(buf ^ 1) * T * n);
            prefetch(tile + 2 * gridDim.x);
        } else if (cnt == tv) {
            // head (< 16 bytes) and tail by bytes, body 16 bytes per lane: four LDS reads in flight, then four stores
            const int head = (16 - shift) & 15;
            const int hb = head < bytes ? head : bytes;
            for (int b = tid; b < hb; b += kObsWork) gobs[g0 + b] = tile_lds[b];
            const int n16 = (bytes - hb) >> 4;
            const uint4 *src = (const uint4 *)(tile_lds + hb);
            uint4 *dst = (uint4 *)(gobs + g0 + hb);
            int i = tid;
            for (; i + 3 * kObsWork < n16; i += 4 * kObsWork) {
                const uint4 v0 = src[i], v1 = src[i + kObsWork], v2 = src[i + 2 * kObsWork], v3 = src[i + 3 * kObsWork];
                dst[i] = v0; dst[i + kObsWork] = v1; dst[i + 2 * kObsWork] = v2; dst[i + 3 * kObsWork] = v3;
            }
            for (; i < n16; i += kObsWork) dst[i] = src[i];
            for (int b = hb + (n16 << 4) + tid; b < bytes; b += kObsWork) gobs[g0 + b] = tile_lds[b];
        } else if (cnt != 0) {
            for (int s = 0; s < tv; ++s)
                if (flag[s])
                    for (int b = tid; b < row_bytes; b += kObsWork) gobs[g0 + (size_t)s * row_bytes + b] = tile_lds[(size_t)s * row_bytes + b];
        }
    }
}

// MEDAEnv.updateHealth (meda.py:600-605) for the chips flagged by the last reset / auto-reset
__global__ __launch_bounds__(kBlock) void k_meda_update_health(MCfg c, MPtrs p) {
    const int e = blockIdx.x * (kBlock / kWave) + (int)(threadIdx.x / kWave);
    if (e >= c.E || !p.reset_flag[e]) return;
    const int lane = threadIdx.x % kWave;
    const int cells = c.W * c.L;
    const size_t base = (size_t)e * cells;
    for (int i = lane; i < cells; i += kWave)
        if (p.usage[base + i] > 50) { p.health[base + i] = p.health[base + i] * p.degrade[base + i]; p.usage[base + i] = 0; }
    __builtin_amdgcn_s_waitcnt(0);
    if (lane == 0) p.reset_flag[e] = 0;
}

// MEDAEnv.__init__ maps (meda.py:494-504)
__global__ void k_meda_init_maps(MCfg c, MPtrs p) {
    const size_t total = (size_t)c.E * c.W * c.L;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int cells = c.W * c.L;
    const int e = (int)(i / cells), cell = (int)(i % cells);
    p.health[i] = 1.0;
    p.usage[i] = 0;
    double v = 1.0;
    if (c.b_degrade) {
        uint32_t w[4];
        philox(c.k0, c.k1, c.env_id0 + (uint32_t)e, 0u, (uint32_t)cell, STREAM_DEGRADE << 8, w);
        const double d = u53(w[0], w[1]) * 0.4 + 0.6;
        v = (u53(w[2], w[3]) < c.per_healthy) ? 1.0 : d;
    }
    p.degrade[i] = v;
}

__global__ void k_meda_set_task(MCfg c, MPtrs p, const int32_t *starts, const int32_t *ends) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.E) return;
    const int n = c.n, E = c.E;
    for (int i = 0; i < n; ++i) {
        const size_t k = ((size_t)e * n + i) * 2;
        const uint32_t s = (uint32_t)(starts[k] & 0xff) | ((uint32_t)(starts[k + 1] & 0xff) << 8);
        const uint32_t g = (uint32_t)(ends[k] & 0xff) | ((uint32_t)(ends[k + 1] & 0xff) << 8);
        p.starts[(size_t)i * E + e] = s;
        p.st[(size_t)i * E + e] = s | (g << 16);
    }
    p.st[(size_t)n * E + e] = 0;
    p.st[(size_t)(n + 1) * E + e] = 0;
}
__global__ void k_meda_get_task(MCfg c, MPtrs p, int32_t *starts, int32_t *ends) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.E) return;
    const int n = c.n, E = c.E;
    for (int i = 0; i < n; ++i) {
        const size_t k = ((size_t)e * n + i) * 2;
        const uint32_t s = p.starts[(size_t)i * E + e], w = p.st[(size_t)i * E + e];
        if (starts) { starts[k] = s & 0xff; starts[k + 1] = (s >> 8) & 0xff; }
        if (ends) { ends[k] = (w >> 16) & 0xff; ends[k + 1] = w >> 24; }
    }
}
__global__ void k_meda_get_state(MCfg c, MPtrs p, int32_t *pos, uint8_t *status, int32_t *step_count, uint8_t *failed) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= c.E) return;
    const int n = c.n, E = c.E;
    const uint32_t st = p.st[(size_t)n * E + e], sw = p.st[(size_t)(n + 1) * E + e];
    for (int i = 0; i < n; ++i) {
        const uint32_t w = p.st[(size_t)i * E + e];
        if (pos) { pos[((size_t)e * n + i) * 2] = w & 0xff; pos[((size_t)e * n + i) * 2 + 1] = (w >> 8) & 0xff; }
        if (status) status[(size_t)e * n + i] = (st >> i) & 1;
    }
    if (step_count) step_count[e] = sw & 0xffff;
    if (failed) failed[e] = (sw >> 16) != 0;
}

// meda_vec_route_append: lane k = e * n + i writes droplet i's centre (x, y) byte pair to route[e][slot][i]
__global__ void k_meda_route_append(MCfg c, MPtrs p, int slot, int T, uint16_t *route) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int n = c.n, E = c.E;
    if (k >= (long)E * n) return;
    const int e = (int)(k / n), i = (int)(k - (long)e * n);
    const uint32_t w = p.st[(size_t)i * E + e];   // cx | cy << 8 | gx << 16 | gy << 24
    route[((size_t)e * (T + 1) + slot) * n + i] = (uint16_t)(w & 0xffff);
}

// ---- the global state QMIX mixes on (meda_vec_global_obs*) ---------------------------------------------------------------
// int8[2][W][L] per chip: layer 0 = i + 1 on droplet i's 5x5 box, layer 1 = i + 1 on destination i's box, clipped to the chip,
// the highest i winning a shared cell (the last writer of an ascending scatter).  No LDS row tile: work item = (destination,
// chip, 16 bytes of the row at a 16-byte aligned address), v fastest, so that a wave writes ~1 KiB of one row with
// global_store_dwordx4; the bytes of a row's misaligned head and tail item go one by one.  The workgroup's chips are prepared
// once in LDS: their 2n boxes clipped to the chip, and per linear row (layer * W + y) a bit mask of the boxes that reach it.  An
// item ORs the masks of the one or two rows it spans, turns each of those boxes into a 16-bit byte mask and merges value i + 1
// into its four words in box order.
// Chip e's row goes to dst0 + e * stride0 when sel[e] != 0 (sel NULL = all) and, when dst1 is set, also to dst1 + e * stride1
// when in addition term[e] == 0.  With t_row set (the stage of the continuous rollout) chip e's row goes to row t_row[e] + 1 of
// its T + 1 rows instead, dst0 + e * stride0 + (t_row[e] + 1) * S, and a chip whose t_row is outside [0, T) is skipped.
constexpr int kStateChips = 64;       // most chips per workgroup
constexpr int kStateVec = 16;         // row bytes per work item
constexpr int kStateRowMasks = 2048;  // most linear rows per workgroup (chips x 2W)

// a / d for 0 <= a < 2^24 through the float reciprocal (one correction step) instead of the integer division sequence
__device__ __forceinline__ int div_small(int a, int d, float inv) {
    int q = (int)((float)a * inv);
    if (q * d > a) --q;
    else if ((q + 1) * d <= a) ++q;
    return q;
}

__global__ __launch_bounds__(256) void k_meda_global_obs(MCfg c, MPtrs p, int G, const uint8_t *sel, const uint8_t *term,
                                                         int8_t *dst0, size_t stride0, int8_t *dst1, size_t stride1,
                                                         const int32_t *t_row, int T) {
    // per chip, box 2i = droplet i (layer 0) and box 2i + 1 = destination i (layer 1): linear rows r0 | r1 << 16 and columns
    // x0 | x1 << 16, inclusive and clipped to the chip (r0 > r1 or x0 > x1: nothing on the chip)
    __shared__ uint2 box[kStateChips * 2 * MEDA_MAX_AGENTS];
    __shared__ uint32_t rows[kStateRowMasks];   // chip j, linear row r: bit b set when box b reaches the row
    __shared__ int8_t *base[2][kStateChips];   // the chip's row per destination, nullptr = not written
    const int W = c.W, L = c.L, n = c.n, E = c.E, S = 2 * W * L, R = 2 * W;
    const int e0 = blockIdx.x * G, gn = min(G, E - e0);
    for (int k = threadIdx.x; k < gn * R; k += blockDim.x) rows[k] = 0u;
    if ((int)threadIdx.x < gn) {
        const int j = threadIdx.x, e = e0 + j;
        const bool skip = (sel && !sel[e]) || (t_row && (unsigned)t_row[e] >= (unsigned)T);
        base[0][j] = skip ? nullptr : dst0 + (size_t)e * stride0 + (t_row ? (size_t)(t_row[e] + 1) * S : 0);
        base[1][j] = skip || !dst1 || term[e] ? nullptr : dst1 + (size_t)e * stride1;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < gn * n; k += blockDim.x) {
        const int i = k / gn, j = k - i * gn;   // consecutive lanes read consecutive chips of droplet i
        const uint32_t w = p.st[(size_t)i * E + e0 + j];   // cx | cy << 8 | gx << 16 | gy << 24
#pragma unroll
        for (int layer = 0; layer < 2; ++layer) {
            const int bx = (int)((w >> (16 * layer)) & 0xff), by = (int)((w >> (16 * layer + 8)) & 0xff);
            const int r0 = layer * W + max(by - kR, 0), r1 = layer * W + min(by + kR, W - 1);
            const int x0 = max(bx - kR, 0), x1 = min(bx + kR, L - 1);
            box[(j * n + i) * 2 + layer] = make_uint2((uint32_t)r0 | ((uint32_t)r1 << 16), (uint32_t)x0 | ((uint32_t)x1 << 16));
            for (int r = r0; r <= r1; ++r) atomicOr(&rows[j * R + r], 1u << (2 * i + layer));
        }
    }
    __syncthreads();
    const int nv = S / kStateVec + 2;   // items per row: a row that starts off a 16-byte boundary spans one more line
    const int items = (dst1 ? 2 : 1) * gn * nv;
    const int adv = (int)blockDim.x / nv, rem = (int)blockDim.x - adv * nv;
    const float inv_L = 1.0f / (float)L;
    int dj = div_small((int)threadIdx.x, nv, 1.0f / (float)nv), v = (int)threadIdx.x - dj * nv;   // item k = dj * nv + v
    for (int k = threadIdx.x; k < items; k += blockDim.x, v += rem, dj += adv + (v >= nv ? 1 : 0), v -= (v >= nv ? nv : 0)) {
        const int d = dj >= gn ? 1 : 0, j = dj - d * gn;
        int8_t *row = base[d][j];
        if (!row) continue;
        const int k0 = v * kStateVec - (int)((uintptr_t)row & (kStateVec - 1));   // row byte at the item's first address
        if (k0 >= S || k0 + kStateVec <= 0) continue;
        const int lo = max(k0, 0), hi = min(k0 + kStateVec, S);                    // the item's bytes of the row: [lo, hi)
        const int ly0 = div_small(lo, L, inv_L);
        int ly1 = ly0;
        for (int x = lo - ly0 * L + (hi - 1 - lo); x >= L; x -= L) ++ly1;
        uint32_t cand = 0;
        for (int ly = ly0; ly <= ly1; ++ly) cand |= rows[j * R + ly];
        uint32_t q[4] = {0u, 0u, 0u, 0u};
        const uint2 *bj = box + j * 2 * n;
        while (cand) {   // ascending box order: the last writer wins
            const int b = __ffs(cand) - 1;
            cand &= cand - 1;
            const uint2 bb = bj[b];
            const int r0 = max((int)(bb.x & 0xffff), ly0), r1 = min((int)(bb.x >> 16), ly1);
            const int x0 = (int)(bb.y & 0xffff), x1 = (int)(bb.y >> 16);
            uint32_t m = 0;   // bit t: byte k0 + t of the item lies in the box
            for (int ly = r0; ly <= r1; ++ly) {
                const int f = max(ly * L + x0 - k0, 0), z = min(ly * L + x1 - k0, kStateVec - 1);
                if (f <= z) m |= (2u << z) - (1u << f);
            }
            const uint32_t val = (uint32_t)(b >> 1) + 1u;
#pragma unroll
            for (int u = 0; u < 4; ++u) {   // 4 mask bits -> 4 byte masks (shifted copies 7 bits apart: no carries)
                const uint32_t bm = ((((m >> (4 * u)) & 0xfu) * 0x00204081u) & 0x01010101u) * 0xffu;
                q[u] = (q[u] & ~bm) | (val * 0x01010101u & bm);
            }
        }
        if (lo == k0 && hi == k0 + kStateVec) {
            *(uint4 *)(row + k0) = make_uint4(q[0], q[1], q[2], q[3]);
        } else {
#pragma unroll
            for (int t = 0; t < kStateVec; ++t)
                if (k0 + t >= lo && k0 + t < hi) row[k0 + t] = (int8_t)(q[t >> 2] >> (8 * (t & 3)));
        }
    }
}
}  // namespace

struct meda_vec {
    meda_vec_config cfg;
    MCfg dc;
    MPtrs dp;
    size_t bytes = 0;
    size_t obs_lds = 0;
    int obs_grid = 1;    // persistent grid of the observation kernel
    int n_cu = 256;
    int8_t zoom_host[512];
    int8_t *zoom_dev = nullptr;
    mutable ObserveTiming timing;  // meda_vec_observe_timing
};

namespace {

template <int N> int step_n(meda_vec *h, const MStepArgs &a, hipStream_t s) { HIP_TRY(launch_meda_step_n<N>(h->dc, h->dp, a, s)); return MEDA_OK; }
template <int N> int reset_n(meda_vec *h, const uint8_t *m, int mode, hipStream_t s) { HIP_TRY(launch_meda_reset_n<N>(h->dc, h->dp, m, mode, s)); return MEDA_OK; }

#define DISPATCH_N(n, FN, ...)                                  \
    switch (n) {                                                \
    case 1: return FN<1>(__VA_ARGS__);  case 2: return FN<2>(__VA_ARGS__);   \
    case 3: return FN<3>(__VA_ARGS__);  case 4: return FN<4>(__VA_ARGS__);   \
    case 5: return FN<5>(__VA_ARGS__);  case 6: return FN<6>(__VA_ARGS__);   \
    case 7: return FN<7>(__VA_ARGS__);  case 8: return FN<8>(__VA_ARGS__);   \
    case 9: return FN<9>(__VA_ARGS__);  case 10: return FN<10>(__VA_ARGS__); \
    case 11: return FN<11>(__VA_ARGS__); case 12: return FN<12>(__VA_ARGS__); \
    case 13: return FN<13>(__VA_ARGS__); case 14: return FN<14>(__VA_ARGS__); \
    case 15: return FN<15>(__VA_ARGS__); case 16: return FN<16>(__VA_ARGS__); \
    default: return MEDA_ERR_UNSUPPORTED;                       \
    }
int launch_step(meda_vec *h, const MStepArgs &a, hipStream_t s) { DISPATCH_N(h->cfg.n_agents, step_n, h, a, s) }
int launch_reset(meda_vec *h, const uint8_t *m, int mode, hipStream_t s) { DISPATCH_N(h->cfg.n_agents, reset_n, h, m, mode, s) }

int launch_observe(const meda_vec *h, const uint8_t *mask, int8_t *obs, hipStream_t s) {
    const dim3 grid(h->obs_grid), block(kObsBlock);
    hipEvent_t t0 = nullptr, t1 = nullptr;
    h->timing.slot(t0, t1);
    // hipExtLaunchKernelGGL: the events receive the dispatch's own start/end time stamps (nullptr = plain launch)
    HIP_TRY(launch_status([&] {
        if (h->dc.n <= 4) hipExtLaunchKernelGGL(k_meda_observe<4>, grid, block, h->obs_lds, s, t0, t1, 0, h->dc, h->dp, mask, obs);
        else if (h->dc.n <= 8) hipExtLaunchKernelGGL(k_meda_observe<8>, grid, block, h->obs_lds, s, t0, t1, 0, h->dc, h->dp, mask, obs);
        else hipExtLaunchKernelGGL(k_meda_observe<MEDA_MAX_AGENTS>, grid, block, h->obs_lds, s, t0, t1, 0, h->dc, h->dp, mask, obs);
    }));
    return MEDA_OK;
}
int launch_update_health(const meda_vec *h, hipStream_t s) {
    if (!h->dp.health) return MEDA_OK;
    if (!h->cfg.b_degrade) {  // updateHealth returns early (meda.py:601-602): just clear the flags
        HIP_TRY(hipMemsetAsync(h->dp.reset_flag, 0, (size_t)h->cfg.n_envs, s));
        return MEDA_OK;
    }
    const int per = kBlock / kWave;
    LAUNCH(k_meda_update_health, dim3((h->cfg.n_envs + per - 1) / per), dim3(kBlock), 0, s, h->dc, h->dp);
    return MEDA_OK;
}

// meda_vec_create past the argument checks, on the handle's device; the caller destroys the handle when this fails
int init(meda_vec *h, hipStream_t s) {
    const meda_vec_config *cfg = &h->cfg;
    MCfg &d = h->dc;
    d.W = cfg->width; d.L = cfg->length; d.fov = cfg->fov; d.ff = cfg->fov * cfg->fov;
    d.version = cfg->obs_version; d.obs_len = (cfg->obs_version == 2 ? 3 : 4) * d.ff + 2;
    d.max_step = cfg->width + cfg->length; d.b_degrade = cfg->b_degrade != 0; d.E = cfg->n_envs; d.n = cfg->n_agents;
    d.k0 = (uint32_t)cfg->seed; d.k1 = (uint32_t)(cfg->seed >> 32); d.env_id0 = cfg->env_id0;
    d.per_healthy = 1.0 - cfg->per_degrade;
    const int E = cfg->n_envs, n = cfg->n_agents;
    const size_t row = (size_t)n * d.obs_len;
    {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && v > 0) h->n_cu = v;
    }
    // observation tile, at most 64 chips (the loader wave keeps one chip per lane).  Measured on MI355X at 30x30, 4
    // droplets, fov 19 (tools/probe/meda_tile_sweep.sh, profiles/r02/meda_tile_sweep.txt): the base observation is
    // fastest with the largest tile (64 KB of LDS, two workgroups per CU: its fill is light, fewer barriers per
    // byte), the v0_2 one with ~40 KB (four per CU: bands and the set order make its fill heavier, more overlap)
    size_t cap = (cfg->obs_version == 2 ? 40 : 64) * 1024;
    if (const char *v = getenv("MEDA_VEC_TILE_KB")) cap = (size_t)atoi(v) * 1024;  // tuning knob
    int T = 1;
    while (T < 64 && obs_lds_bytes(T + 1, n, (int)row) <= cap) ++T;
    while (T > 1 && (E + T - 1) / T < 2 * h->n_cu) --T;  // keep the grid wide for small batches
    if (const char *v = getenv("MEDA_VEC_OBS_TILE")) {  // tuning knob: chips per tile
        const int t = atoi(v);
        if (t >= 1 && t <= 64 && obs_lds_bytes(t, n, (int)row) <= 64 * 1024) T = t;
    }
    d.T = T;
    h->obs_lds = obs_lds_bytes(T, n, (int)row);
    h->obs_grid = persistent_grid(h->obs_lds, (E + T - 1) / T, h->n_cu);
    memset(&h->dp, 0, sizeof(h->dp));
    const size_t st_bytes = (size_t)(n + 4) * E * 4, starts_bytes = (size_t)n * E * 4, cells = (size_t)cfg->width * cfg->length;
    HIP_TRY(hipMalloc(&h->dp.st, st_bytes));
    HIP_TRY(hipMalloc(&h->dp.starts, starts_bytes));
    HIP_TRY(hipMalloc(&h->dp.reset_flag, (size_t)E));
    h->bytes = st_bytes + starts_bytes + E;
    HIP_TRY(hipMemsetAsync(h->dp.st, 0, st_bytes, s));
    HIP_TRY(hipMemsetAsync(h->dp.reset_flag, 0, (size_t)E, s));
    for (int dd = -128; dd <= 127; ++dd) {  // python round() = half to even on the double quotient (meda.py:894)
        h->zoom_host[dd + 128] = (int8_t)(int)std::nearbyint((double)dd / ((double)cfg->width / 30.0));
        h->zoom_host[256 + dd + 128] = (int8_t)(int)std::nearbyint((double)dd / ((double)cfg->length / 30.0));
    }
    HIP_TRY(hipMalloc(&h->zoom_dev, sizeof(h->zoom_host)));
    HIP_TRY(hipMemcpyAsync(h->zoom_dev, h->zoom_host, sizeof(h->zoom_host), hipMemcpyHostToDevice, s));
    h->dp.zoom = h->zoom_dev;
    if (cfg->b_degrade || cfg->with_maps) {
        HIP_TRY(hipMalloc(&h->dp.health, cells * E * 8));
        HIP_TRY(hipMalloc(&h->dp.degrade, cells * E * 8));
        HIP_TRY(hipMalloc(&h->dp.usage, cells * E * 2));
        h->bytes += cells * E * 18;
        const size_t total = cells * E;
        LAUNCH(k_meda_init_maps, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, h->dc, h->dp);
    }
    const int rc = launch_reset(h, nullptr, 3, s);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(h->dp.reset_flag, 0, (size_t)E, s));  // construction does not run updateHealth
    HIP_TRY(hipStreamSynchronize(s));  // the zoom table upload reads host memory owned by the handle
    return MEDA_OK;
}

}  // namespace

extern "C" {

int meda_vec_check_config(const meda_vec_config *c) {
    if (!c) return MEDA_ERR_BAD_ARG;
    if (c->width <= 0 || c->length <= 0) return MEDA_ERR_BAD_SIZE;
    if (c->n_agents <= 0) return MEDA_ERR_NO_AGENTS;
    if (c->n_agents > (c->width / 15) * (c->length / 15)) return MEDA_ERR_TOO_MANY_DROPLETS;
    if (c->n_agents > MEDA_MAX_AGENTS || c->width > MEDA_MAX_DIM || c->length > MEDA_MAX_DIM || c->fov < 1) return MEDA_ERR_UNSUPPORTED;
    if (obs_lds_bytes(1, c->n_agents, c->n_agents * (4 * c->fov * c->fov + 2)) > 60 * 1024) return MEDA_ERR_UNSUPPORTED;  // one chip's rows must fit the LDS tile
    if (c->obs_version != 0 && c->obs_version != 2) return MEDA_ERR_UNSUPPORTED;
    if (c->n_envs <= 0) return MEDA_ERR_BAD_ARG;
    return MEDA_OK;
}

int meda_vec_create(const meda_vec_config *cfg, void *stream, meda_vec **out) {
    if (!out) return MEDA_ERR_BAD_ARG;
    int rc = meda_vec_check_config(cfg);
    if (rc) return rc;
    DeviceGuard g(cfg->device);
    if (!g.ok) return MEDA_ERR_HIP;
    meda_vec *h = new (std::nothrow) meda_vec();
    if (!h) return MEDA_ERR_BAD_ARG;
    h->cfg = *cfg;
    rc = init(h, (hipStream_t)stream);
    if (rc) {
        meda_vec_destroy(h);
        return rc;
    }
    *out = h;
    return MEDA_OK;
}

int meda_vec_destroy(meda_vec *h) {
    if (h) destroy_handle(h, h->dp.st, h->dp.starts, h->dp.reset_flag, h->dp.health, h->dp.degrade, h->dp.usage, h->zoom_dev);
    return MEDA_OK;
}

size_t meda_vec_state_bytes(const meda_vec *h) { return h ? h->bytes : 0; }
int meda_vec_obs_len(const meda_vec *h) { return h ? h->dc.obs_len : MEDA_ERR_BAD_ARG; }
int meda_vec_max_step(const meda_vec *h) { return h ? h->dc.max_step : MEDA_ERR_BAD_ARG; }
int meda_vec_n_envs(const meda_vec *h) { return h ? h->cfg.n_envs : MEDA_ERR_BAD_ARG; }
int meda_vec_n_agents(const meda_vec *h) { return h ? h->cfg.n_agents : MEDA_ERR_BAD_ARG; }

int meda_vec_reset(meda_vec *h, const uint8_t *d_mask, int8_t *d_obs, void *stream) {
    if (!h) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    hipStream_t s = (hipStream_t)stream;
    int rc = launch_reset(h, d_mask, 0, s);
    if (rc) return rc;
    rc = launch_update_health(h, s);
    if (rc || !d_obs) return rc;
    return launch_observe(h, d_mask, d_obs, s);
}

int meda_vec_restart(meda_vec *h, const uint8_t *d_mask, int8_t *d_obs, void *stream) {
    if (!h) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    int rc = launch_reset(h, d_mask, 2, (hipStream_t)stream);
    if (rc || !d_obs) return rc;
    return launch_observe(h, d_mask, d_obs, (hipStream_t)stream);
}

int meda_vec_set_task(meda_vec *h, const int32_t *d_starts, const int32_t *d_ends, void *stream) {
    if (!h || !d_starts || !d_ends) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    LAUNCH(k_meda_set_task, dim3((h->cfg.n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->dc, h->dp, d_starts, d_ends);
    return MEDA_OK;
}
int meda_vec_get_task(const meda_vec *h, int32_t *d_starts, int32_t *d_ends, void *stream) {
    if (!h) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    LAUNCH(k_meda_get_task, dim3((h->cfg.n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->dc, h->dp, d_starts, d_ends);
    return MEDA_OK;
}

int meda_vec_step(meda_vec *h, const void *d_actions, const double *d_uniforms, const uint8_t *d_active, uint32_t flags,
                  const meda_vec_step_out *out, void *stream) {
    if (!h || !d_actions || !out) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    hipStream_t s = (hipStream_t)stream;
    MStepArgs a;
    a.actions = d_actions; a.uniforms = d_uniforms; a.active = d_active; a.flags = flags; a.out = *out;
    int rc = launch_step(h, a, s);
    if (rc) return rc;
    if (flags & MEDA_STEP_AUTORESET) {
        rc = launch_update_health(h, s);
        if (rc) return rc;
    }
    if (out->d_obs) return launch_observe(h, nullptr, out->d_obs, s);
    return MEDA_OK;
}

int meda_vec_observe(const meda_vec *h, const uint8_t *d_mask, int8_t *d_obs, void *stream) {
    if (!h || !d_obs) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    return launch_observe(h, d_mask, d_obs, (hipStream_t)stream);
}

int meda_vec_get_state(const meda_vec *h, int32_t *d_pos, uint8_t *d_status, int32_t *d_step_count, uint8_t *d_failed,
                       void *stream) {
    if (!h) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    LAUNCH(k_meda_get_state, dim3((h->cfg.n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->dc, h->dp, d_pos,
           d_status, d_step_count, d_failed);
    return MEDA_OK;
}

int meda_vec_route_append(const meda_vec *h, int32_t t, int32_t T, uint8_t *d_route, void *stream) {
    if (!h || !d_route || ((uintptr_t)d_route & 1) || T < 1 || t < -1 || t >= T) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    const long lanes = (long)h->cfg.n_envs * h->cfg.n_agents;
    LAUNCH(k_meda_route_append, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->dc, h->dp, t + 1, T,
           (uint16_t *)d_route);
    return MEDA_OK;
}

int meda_vec_shield(const meda_vec *h, const float *d_q, const uint8_t *d_active, int32_t *d_actions, int8_t *d_last_onehot,
                    int8_t *d_ep_u, int8_t *d_ep_onehot, int32_t episode_limit, int32_t t, const int32_t *d_t_ep,
                    int32_t *d_overrides, uint8_t *d_unsafe, void *stream) {
    if (!h || !d_q || !d_actions || !d_last_onehot || (d_ep_u == nullptr) != (d_ep_onehot == nullptr)) return MEDA_ERR_BAD_ARG;
    if (d_ep_u && (episode_limit < 1 || (!d_t_ep && (t < 0 || t >= episode_limit)))) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    ShieldArgs a;
    a.q = d_q; a.active = d_active; a.actions = d_actions; a.last_onehot = d_last_onehot; a.ep_u = d_ep_u; a.ep_onehot = d_ep_onehot;
    a.T = episode_limit; a.t = t; a.t_ep = d_t_ep; a.overrides = d_overrides; a.unsafe = d_unsafe;
    const long lanes = (long)h->cfg.n_envs * kShieldLanes;
    LAUNCH(k_meda_shield, dim3((unsigned)((lanes + kShieldBlock - 1) / kShieldBlock)), dim3(kShieldBlock), 0, (hipStream_t)stream,
           h->dc, h->dp, a);
    return MEDA_OK;
}

int meda_vec_state_len(const meda_vec *h) { return h ? 2 * h->cfg.width * h->cfg.length : MEDA_ERR_BAD_ARG; }

}  // extern "C"

namespace {
int launch_global_obs(const meda_vec *h, const uint8_t *sel, const uint8_t *term, int8_t *dst0, size_t stride0, int8_t *dst1,
                      size_t stride1, hipStream_t s, const int32_t *t_row = nullptr, int T = 0) {
    const int E = h->cfg.n_envs, nv = 2 * h->cfg.width * h->cfg.length / kStateVec + 2;
    // about sixteen items per lane (the chips' setup -- loads, LDS masks, two barriers -- is paid once per workgroup), the grid
    // kept at four workgroups per CU or more for small batches
    int G = std::max(1, std::min(kStateChips, 4096 / nv));
    while (G > 1 && (E + G - 1) / G < 4 * h->n_cu) --G;
    while (G > 1 && G * 2 * h->cfg.width > kStateRowMasks) --G;   // the per-row box masks of the workgroup's chips fit LDS
    LAUNCH(k_meda_global_obs, dim3((E + G - 1) / G), dim3(256), 0, s, h->dc, h->dp, G, sel, term, dst0, stride0, dst1, stride1,
           t_row, T);
    return MEDA_OK;
}
}  // namespace

extern "C" {

int meda_vec_global_obs(const meda_vec *h, const uint8_t *d_mask, int8_t *d_out, void *stream) {
    if (!h || !d_out) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    const size_t S = 2 * (size_t)h->cfg.width * h->cfg.length;
    return launch_global_obs(h, d_mask, nullptr, d_out, S, nullptr, 0, (hipStream_t)stream);
}

int meda_vec_global_obs_append(const meda_vec *h, const uint8_t *d_alive, const uint8_t *d_term, int32_t t, int32_t T, int8_t *d_s,
                               int8_t *d_s_next, void *stream) {
    if (!h || !d_alive || !d_term || !d_s || !d_s_next || t < 0 || t >= T) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    const size_t S = 2 * (size_t)h->cfg.width * h->cfg.length;
    int8_t *s1 = t + 1 < T ? d_s + (size_t)(t + 1) * S : nullptr;
    return launch_global_obs(h, d_alive, d_term, d_s_next + (size_t)t * S, (size_t)T * S, s1, (size_t)T * S, (hipStream_t)stream);
}

int meda_vec_global_obs_stage_first(const meda_vec *h, const uint8_t *d_mask, int32_t T, int8_t *d_stage, void *stream) {
    if (!h || !d_stage || T < 1) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    const size_t S = 2 * (size_t)h->cfg.width * h->cfg.length;
    return launch_global_obs(h, d_mask, nullptr, d_stage, (size_t)(T + 1) * S, nullptr, 0, (hipStream_t)stream);
}

int meda_vec_global_obs_stage_close(const meda_vec *h, const int32_t *d_t_ep, const int32_t *d_close_slot, int32_t T,
                                    int8_t *d_stage, int8_t *d_ring_s, int32_t slots, void *stream) {
    if (!h || !d_t_ep || !d_close_slot || !d_stage || !d_ring_s || T < 1 || slots < h->cfg.n_envs) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    const hipStream_t s = (hipStream_t)stream;
    const size_t S = 2 * (size_t)h->cfg.width * h->cfg.length;
    // stage[e][t + 1] = state(e) with t = d_t_ep[e] (k_meda_global_obs with a per-chip destination row) ...
    int rc = launch_global_obs(h, nullptr, nullptr, d_stage, (size_t)(T + 1) * S, nullptr, 0, s, d_t_ep, T);
    if (rc) return rc;
    // ... then the rows of the closing chips into their ring slots (k_state_close, vec_env.h)
    return launch_state_close(h->cfg.n_envs, T, S, slots, h->n_cu, d_t_ep, d_close_slot, d_stage, d_ring_s, s);
}

int meda_vec_get_map(const meda_vec *h, int which, double *d_buf, void *stream) {
    if (!h || !d_buf || which < 0 || which > 2) return MEDA_ERR_BAD_ARG;
    if (!h->dp.health) return MEDA_ERR_NO_MAPS;
    DeviceGuard g(h->cfg.device);
    const size_t total = (size_t)h->cfg.n_envs * h->cfg.width * h->cfg.length;
    LAUNCH(k_get_map, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, total, h->dp.health,
           h->dp.degrade, h->dp.usage, which, d_buf);
    return MEDA_OK;
}
int meda_vec_set_map(meda_vec *h, int which, const double *d_buf, void *stream) {
    if (!h || !d_buf || which < 0 || which > 2) return MEDA_ERR_BAD_ARG;
    if (!h->dp.health) return MEDA_ERR_NO_MAPS;
    DeviceGuard g(h->cfg.device);
    const size_t total = (size_t)h->cfg.n_envs * h->cfg.width * h->cfg.length;
    LAUNCH(k_set_map, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, total, h->dp.health,
           h->dp.degrade, h->dp.usage, which, d_buf);
    return MEDA_OK;
}

int meda_vec_launch_shape(const meda_vec *h, int32_t out[4]) {
    if (!h || !out) return MEDA_ERR_BAD_ARG;
    out[0] = kBlock; out[1] = h->dc.T; out[2] = kObsBlock; out[3] = h->obs_grid;
    return MEDA_OK;
}

int meda_vec_observe_timing(meda_vec *h, int enable) {
    if (!h) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    return h->timing.enable(enable);
}

int meda_vec_observe_timing_read(meda_vec *h, double *total_us, int *launches) {
    if (!h || !total_us || !launches) return MEDA_ERR_BAD_ARG;
    DeviceGuard g(h->cfg.device);
    return h->timing.read(total_us, launches);
}

const char *meda_vec_strerror(int code) {
    switch (code) {
    case MEDA_OK: return "ok";
    case MEDA_ERR_BAD_ARG: return "bad argument";
    case MEDA_ERR_TOO_MANY_DROPLETS: return "Too many droplets in the MEDA array";
    case MEDA_ERR_BAD_SIZE: return "w > 0 and l > 0 required";
    case MEDA_ERR_NO_AGENTS: return "n_agents > 0 required";
    case MEDA_ERR_UNSUPPORTED: return "configuration outside the build limits";
    case MEDA_ERR_NO_MAPS: return "handle was created without health/usage/degrade maps";
    case MEDA_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
    }
}
int meda_vec_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
