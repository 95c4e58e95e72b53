// vdn_lambda_kernels.h -- the kernels of include/vdn_lambda.h: the TD block of the VDN learn on lambda-returns.  Included by
// vdn_ops.hip behind td_block_sums, whose fixed-order sums and ticket word the kernels here share.
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

constexpr int kLamT = VDN_LAMBDA_MAX_T;
constexpr int kLamEp = VDN_LAMBDA_WG_EPISODES;

// packed form: the first unit of step t (prefix sums of the host's counts), off[n_steps] = n_units
struct LambdaOff {
    int32_t off[kLamT + 1];
};

// where step t of episode b lies: the padded form (time-major Q tensors, chip-major episode tensors, outputs [B][T]) ...
struct LamPadded {
    int B, T, Tl;
    __device__ __forceinline__ size_t slot(int b, int t) const { return (size_t)b * Tl + t; }
    __device__ __forceinline__ size_t qrow(int b, int t, int n, int A) const { return ((size_t)t * B + b) * n * A; }
    __device__ __forceinline__ size_t out(int b, int t) const { return (size_t)b * T + t; }
};
// ... and the packed form: unit j = off[t] + rank, the replay tensors indexed through units[j]
struct LamPacked {
    const int32_t *off;     // LDS copy of LambdaOff
    const int32_t *units;
    __device__ __forceinline__ size_t slot(int b, int t) const { return (size_t)units[off[t] + b]; }
    __device__ __forceinline__ size_t qrow(int b, int t, int n, int A) const { return (size_t)(off[t] + b) * n * A; }
    __device__ __forceinline__ size_t out(int b, int t) const { return (size_t)(off[t] + b); }
};

// ep: this wave's episode, T: its steps (0 for a wave behind the last episode: it only takes part in the barriers and the sums)
template <class IX>
__device__ __forceinline__ void td_lambda_episode(const IX &ix, int ep, int T, const float *__restrict__ qe, const float *__restrict__ qt,
                                                  const int8_t *__restrict__ u, const float *__restrict__ r,
                                                  const int8_t *__restrict__ avail, const uint8_t *__restrict__ term,
                                                  const uint8_t *__restrict__ padded, int n, int A, float gamma, float lam,
                                                  float *__restrict__ mtd, float *__restrict__ maskf, float *__restrict__ targets,
                                                  int32_t *__restrict__ bad, float *part, float *__restrict__ sums) {
    __shared__ float s_g[kLamEp][kLamT], s_r[kLamEp][kLamT], s_e[kLamEp][kLamT];
    __shared__ uint8_t s_f[kLamEp][kLamT];   // bit 0 terminated, bit 1 padded, bit 2 an action outside [0, A)
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;

    // ---- phase A: Q', e and the flags of every step, exactly as k_td_forward forms them
    int first_pad = T;
    for (int t = lane; t < T; t += 64) {
        const size_t s = ix.slot(ep, t), q0 = ix.qrow(ep, t, n, A);
        float qe_tot = 0.0f, qt_tot = 0.0f;
        bool ok = true;
        for (int i = 0; i < n; ++i) {
            int a_taken = (int)u[s * n + i];
            if ((unsigned)a_taken >= (unsigned)A) { ok = false; a_taken = 0; }   // never used as an index
            qe_tot = qe_tot + qe[q0 + (size_t)i * A + a_taken];
            float m = -3.4e38f;
            for (int a = 0; a < A; ++a) {
                const float v = avail[(s * n + i) * A + a] == 0 ? -9999999.0f : qt[q0 + (size_t)i * A + a];
                m = v > m ? v : m;
            }
            qt_tot = qt_tot + m;
        }
        const bool pad = padded[s] != 0;
        s_g[w][t] = qt_tot;
        s_r[w][t] = r[s];
        s_e[w][t] = qe_tot;
        s_f[w][t] = (uint8_t)((term[s] ? 1 : 0) | (pad ? 2 : 0) | (ok ? 0 : 4));
        if (pad && t < first_pad) first_pad = t;
    }
    for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(first_pad, o); first_pad = other < first_pad ? other : first_pad; }
    const int L = first_pad;   // the leading steps with padded == 0
    __syncthreads();

    // ---- phase B: the backward walk, one lane per episode
    if (lane == 0) {
        const float om = 1.0f - lam;
        float g_next = 0.0f;
        for (int t = T - 1; t >= 0; --t) {
            const float q = s_g[w][t];
            const float y = t >= L - 1 ? q : (om * q) + (lam * g_next);
            const float nt = 1.0f - ((s_f[w][t] & 1) ? 1.0f : 0.0f);
            const float g = s_r[w][t] + (gamma * y) * nt;
            s_g[w][t] = g;
            g_next = g;
        }
    }
    __syncthreads();

    // ---- phase C: the outputs; every lane adds its slots in step order
    float sq = 0.0f, mks = 0.0f;
    for (int t = lane; t < T; t += 64) {
        const size_t o = ix.out(ep, t);
        const int f = s_f[w][t];
        const float g = s_g[w][t];
        const float mk = 1.0f - ((f & 2) ? 1.0f : 0.0f);
        const float m = (f & 4) ? __builtin_nanf("") : mk * (g - s_e[w][t]);
        mtd[o] = m;
        maskf[o] = mk;
        if (targets) targets[o] = g;
        if ((f & 4) && bad) atomicAdd(bad, 1);
        sq = sq + m * m;
        mks = mks + mk;
    }
    if (sums) td_block_sums(sq, mks, part, sums);
}

__global__ __launch_bounds__(256) void k_td_lambda_forward(const float *__restrict__ qe, const float *__restrict__ qt, const int8_t *__restrict__ u,
                                                           const float *__restrict__ r, const int8_t *__restrict__ avail,
                                                           const uint8_t *__restrict__ term, const uint8_t *__restrict__ padded, int B,
                                                           int T, int Tl, int n, int A, float gamma, float lam, float *__restrict__ mtd,
                                                           float *__restrict__ maskf, float *__restrict__ targets,
                                                           int32_t *__restrict__ bad, float *part, float *__restrict__ sums) {
    const int ep = blockIdx.x * kLamEp + (threadIdx.x >> 6);
    const LamPadded ix{B, T, Tl};
    td_lambda_episode(ix, ep, ep < B ? T : 0, qe, qt, u, r, avail, term, padded, n, A, gamma, lam, mtd, maskf, targets, bad, part, sums);
}

// E episodes (= the units of step 0), n_steps steps in the longest
__global__ __launch_bounds__(256) void k_td_lambda_forward_packed(const float *__restrict__ qe, const float *__restrict__ qt,
                                                                  const int32_t *__restrict__ units, const int8_t *__restrict__ u,
                                                                  const float *__restrict__ r, const int8_t *__restrict__ avail,
                                                                  const uint8_t *__restrict__ term, const uint8_t *__restrict__ padded,
                                                                  int E, int n_steps, int n, int A, float gamma, float lam,
                                                                  float *__restrict__ mtd, float *__restrict__ maskf,
                                                                  float *__restrict__ targets, int32_t *__restrict__ bad, float *part,
                                                                  float *__restrict__ sums, LambdaOff lo) {
    __shared__ int32_t s_off[kLamT + 1];
    for (int t = threadIdx.x; t <= n_steps; t += 256) s_off[t] = lo.off[t];
    __syncthreads();
    const int ep = blockIdx.x * kLamEp + (threadIdx.x >> 6);
    int T = 0;   // this episode's length: the steps with more than `ep` units
    if (ep < E) {
        for (int t = threadIdx.x & 63; t < n_steps; t += 64) T += (s_off[t + 1] - s_off[t] > ep) ? 1 : 0;
        for (int o = 32; o > 0; o >>= 1) T += __shfl_xor(T, o);
    }
    const LamPacked ix{s_off, units};
    td_lambda_episode(ix, ep, T, qe, qt, u, r, avail, term, padded, n, A, gamma, lam, mtd, maskf, targets, bad, part, sums);
}

}  // namespace
