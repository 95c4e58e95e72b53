// qmix_lambda_kernels.h -- the walk kernels of include/qmix_lambda.h: the TD rule of the QMIX learn on lambda-returns.  Included by
// qmix_ops.hip, whose k_mix_forward<H, Index, true> has left e[t] (the eval mixer's q_tot, NaN for a bad-action row) and Q'[t] (the
// target mixer's) of every row in two float32 arrays before these run.
//
// Layout, that of vdn_lambda_kernels.h: one wave per episode, four episodes per workgroup.  Phase A: the lanes stride over the
// episode's steps and leave Q'[t], r[t], e[t] and the step's flags in LDS.  Phase B: lane 0 of the wave walks t backwards (the
// recurrence of the header, one float operation after the other: a parallel scan would round differently) and overwrites Q'[t] by
// G[t].  Phase C: the lanes write mtd, mask and the targets.  No sums, no atomics.  LDS per workgroup: 4 x (3 x 512 floats + 512
// bytes) = 26 624 bytes, + 2 052 bytes of unit offsets in the packed form.  LambdaOff, the packed preamble and phase B come from
// td_rules.h, which vdn_lambda_kernels.h shares; phases A and C differ: here they read the totals, there they run the row rule.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/qmix_lambda.h"

namespace {

struct WalkIn {
    const float *tot_e, *tot_t, *r;
    const uint8_t *term, *padded;
    float gamma, lam;
};

struct WalkOut {
    float *mtd, *maskf, *targets;   // targets may be NULL
};

// Where step t of episode ep lives: row = its element of tot_e / tot_t and of the outputs, step = its element of the replay tensors.
struct PaddedWalk {   // include/qmix_ops.h: row b * T + t, replay step b * t_limit + t
    int T, Tl;
    __device__ __forceinline__ size_t row(int ep, int t) const { return (size_t)ep * T + t; }
    __device__ __forceinline__ size_t step(int ep, int t, size_t) const { return (size_t)ep * Tl + t; }
};

struct PackedWalk {   // include/qmix_packed.h: unit off[t] + ep, replay step units[unit]
    const int32_t *units, *off;
    __device__ __forceinline__ size_t row(int ep, int t) const { return (size_t)off[t] + ep; }
    __device__ __forceinline__ size_t step(int, int, size_t row) const { return (size_t)units[row]; }
};

// ep: this wave's episode, T: its steps (0 for a wave behind the last episode: it only takes part in the barriers)
template <class Walk>
__device__ __forceinline__ void mix_lambda_episode(const Walk &ix, int ep, int T, const WalkIn &in, const WalkOut &out) {
    __shared__ float s_g[kLamEp][kLamT], s_r[kLamEp][kLamT], s_e[kLamEp][kLamT];
    __shared__ uint8_t s_f[kLamEp][kLamT];   // bit 0 terminated, bit 1 padded
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;

    // ---- phase A: Q', e, r and the flags of every step
    int first_pad = T;
    for (int t = lane; t < T; t += 64) {
        const size_t row = ix.row(ep, t), st = ix.step(ep, t, row);
        const bool pad = in.padded[st] != 0;
        s_g[w][t] = in.tot_t[row];
        s_r[w][t] = in.r[st];
        s_e[w][t] = in.tot_e[row];
        s_f[w][t] = (uint8_t)((in.term[st] ? 1 : 0) | (pad ? 2 : 0));
        if (pad && t < first_pad) first_pad = t;
    }
    for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(first_pad, o); first_pad = other < first_pad ? other : first_pad; }
    const int L = first_pad;   // the leading steps with padded == 0
    __syncthreads();

    // ---- phase B: the backward walk, one lane per episode
    if (lane == 0) lambda_walk_back(s_g[w], s_r[w], s_f[w], L, T, in.gamma, in.lam);
    __syncthreads();

    // ---- phase C: the outputs (e is NaN in a bad-action row, so mtd is NaN there whatever the mask)
    for (int t = lane; t < T; t += 64) {
        const size_t o = ix.row(ep, t);
        const float g = s_g[w][t];
        const float mk = 1.0f - ((s_f[w][t] & 2) ? 1.0f : 0.0f);
        out.mtd[o] = mk * (s_e[w][t] - g);
        out.maskf[o] = mk;
        if (out.targets) out.targets[o] = g;
    }
}

__global__ __launch_bounds__(256) void k_mix_lambda_walk(const PaddedWalk ix, int B, const WalkIn in, const WalkOut out) {
    const int ep = blockIdx.x * kLamEp + (threadIdx.x >> 6);
    mix_lambda_episode(ix, ep, ep < B ? ix.T : 0, in, out);
}

// E episodes (= the units of step 0), n_steps steps in the longest; ix.off comes in NULL and becomes the LDS copy of lo
__global__ __launch_bounds__(256) void k_mix_lambda_walk_packed(PackedWalk ix, int E, int n_steps, const WalkIn in, const WalkOut out,
                                                                const LambdaOff lo) {
    int T;
    ix.off = lambda_packed_episode(lo, E, n_steps, T);
    mix_lambda_episode(ix, blockIdx.x * kLamEp + (threadIdx.x >> 6), T, in, out);
}

}  // namespace
