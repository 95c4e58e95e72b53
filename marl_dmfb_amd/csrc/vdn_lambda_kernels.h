// vdn_lambda_kernels.h -- the kernels of include/vdn_lambda.h: the TD block of the VDN learn on lambda-returns.  Included by
// vdn_ops.hip behind td_block_sums (whose fixed-order sums and ticket word the kernels here share), the operand structs, the index
// rules and td_row, the row rule of the one-step kernel.  LambdaOff, the packed preamble and phase B come from td_rules.h, which
// qmix_lambda_kernels.h shares.
//
// Layout: one wave per episode, four episodes per workgroup.  Phase A: the lanes stride over the episode's steps and leave Q'[t],
// r[t], e[t] and the step's flags in LDS.  Phase B: lane 0 of the wave walks t backwards (the recurrence of the header, one float
// operation after the other: a parallel scan would round differently) and overwrites Q'[t] by G[t].  Phase C: the lanes write mtd,
// mask and the targets and add their slots' squares in a fixed order.  LDS per workgroup: 4 x (3 x 512 floats + 512 bytes) = 26 624
// bytes, + 2 052 bytes of unit offsets in the packed form, + the 36 bytes of td_block_sums.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vdn_lambda.h"

namespace {

// ep: this wave's episode, T: its steps (0 for a wave behind the last episode: it only takes part in the barriers and the sums)
template <class Index, class Sel>
__device__ __forceinline__ void td_lambda_episode(const Index &ix, int ep, int T, const TdIn &in, float lam, const TdOut &out, const Sel &sel) {
    __shared__ float s_g[kLamEp][kLamT], s_r[kLamEp][kLamT], s_e[kLamEp][kLamT];
    __shared__ uint8_t s_f[kLamEp][kLamT];   // bit 0 terminated, bit 1 padded, bit 2 an action outside [0, A)
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;

    // ---- phase A: Q', e and the flags of every step, by the row rule of the one-step kernel (td_row)
    int first_pad = T;
    for (int t = lane; t < T; t += 64) {
        const int row = ix.row(ep, t);
        const At at = ix.at(row, in.n, in.A);
        const TdRow q = td_row(in, at, sel, row);
        const bool pad = in.padded[at.ep] != 0;
        s_g[w][t] = q.qt_tot;
        s_r[w][t] = in.r[at.ep];
        s_e[w][t] = q.qe_tot;
        s_f[w][t] = (uint8_t)((in.term[at.ep] ? 1 : 0) | (pad ? 2 : 0) | (q.ok ? 0 : 4));
        if (pad && t < first_pad) first_pad = t;
    }
    for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(first_pad, o); first_pad = other < first_pad ? other : first_pad; }
    const int L = first_pad;   // the leading steps with padded == 0
    __syncthreads();

    // ---- phase B: the backward walk, one lane per episode
    if (lane == 0) lambda_walk_back(s_g[w], s_r[w], s_f[w], L, T, in.gamma, lam);
    __syncthreads();

    // ---- phase C: the outputs; every lane adds its slots in step order
    float sq = 0.0f, mks = 0.0f;
    for (int t = lane; t < T; t += 64) {
        const int o = ix.row(ep, t);
        const int f = s_f[w][t];
        const float g = s_g[w][t];
        const float mk = 1.0f - ((f & 2) ? 1.0f : 0.0f);
        const float m = (f & 4) ? __builtin_nanf("") : mk * (g - s_e[w][t]);
        out.mtd[o] = m;
        out.maskf[o] = mk;
        if (out.targets) out.targets[o] = g;
        if ((f & 4) && out.bad) atomicAdd(out.bad, 1);
        sq = sq + m * m;
        mks = mks + mk;
    }
    if (out.sums) td_block_sums(sq, mks, out.part, out.sums);
}

__global__ __launch_bounds__(256) void k_td_lambda_forward(const PaddedIndex ix, const TdIn in, float lam, const TdOut out) {
    const int ep = blockIdx.x * kLamEp + (threadIdx.x >> 6);
    td_lambda_episode(ix, ep, ep < ix.B ? ix.T : 0, in, lam, out, NoSel{});
}

// E episodes (= the units of step 0), n_steps steps in the longest; ix.off comes in NULL and becomes the LDS copy of lo
template <class Sel>
__device__ __forceinline__ void td_lambda_packed(PackedIndex ix, int E, int n_steps, const TdIn &in, float lam, const TdOut &out,
                                                 const LambdaOff &lo, const Sel &sel) {
    int T;
    ix.off = lambda_packed_episode(lo, E, n_steps, T);
    td_lambda_episode(ix, blockIdx.x * kLamEp + (threadIdx.x >> 6), T, in, lam, out, sel);
}
__global__ __launch_bounds__(256) void k_td_lambda_forward_packed(PackedIndex ix, int E, int n_steps, const TdIn in, float lam, const TdOut out,
                                                                  const LambdaOff lo) {
    td_lambda_packed(ix, E, n_steps, in, lam, out, lo, NoSel{});
}

}  // namespace
