// td_rules.h -- what the TD block of the VDN learn (vdn_ops.hip) and the mixing + TD block of the QMIX learn (qmix_ops.hip) both
// use, each written once: the double-Q selector operand, and the pieces of the lambda walk that do not depend on where a learner
// keeps its rows.  Both learners promise the bits of the float32 numpy rule of policy/td_lambda.py: the float operations of phase B
// and their order are that contract.
//
// Not here: the index rules (PaddedIndex / PackedIndex of either file: QMIX's carry the P-row layout, VDN's the unit mapping of the
// backward), phases A and C of the walk, and the per-agent pick itself: td_row of vdn_ops.hip and k_mix_forward of qmix_ops.hip each
// keep their copy (profiles/mix_block/NOTES.md: a shared function cost a QMIX kernel a wave).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/qmix_lambda.h"
#include "../../include/vdn_lambda.h"

namespace {

static_assert(VDN_LAMBDA_MAX_T == QMIX_LAMBDA_MAX_T && VDN_LAMBDA_WG_EPISODES == QMIX_LAMBDA_WG_EPISODES,
              "the two learners share LambdaOff and the layout of the walk");
constexpr int kLamT = VDN_LAMBDA_MAX_T;
constexpr int kLamEp = VDN_LAMBDA_WG_EPISODES;   // one wave per episode

// ---- the target side of the pick, a compile-time variant: NoSel, the maximum over the target network's own row, or QSel
// (include/vdn_double.h, include/qmix_double.h), where the first maximum of a selector's row picks the action that the target
// network values.  qs: [T][B][n][A] beside the padded Q tensors, [n_sel][n][A] in the packed form, where sel_units[row] names the
// selector unit of output row `row` (NULL: the row's own block, the one of q_target, which the host has checked to exist).
struct NoSel {
    static constexpr bool on = false;
};
struct QSel {
    static constexpr bool on = true;
    const float *qs;
    const int32_t *sel_units;
    int n_sel;
    int8_t *picks;   // [rows][n] or NULL
    // false: sel_units[row] lies outside [0, n_sel) and is not used as an index; the row then reads no selector at all
    __device__ __forceinline__ bool place(long row, int n, int A, size_t &s0) const {
        if (!sel_units) return true;
        const int32_t k = sel_units[row];
        if ((uint32_t)k >= (uint32_t)n_sel) return false;
        s0 = (size_t)k * n * A;
        return true;
    }
};

// ---- the lambda walk (include/vdn_lambda.h, include/qmix_lambda.h): one wave per episode, kLamEp episodes per workgroup
inline bool lambda_ok(float lam) { return lam >= 0.0f && lam <= 1.0f; }   // false for NaN

// packed form: the first unit of step t (prefix sums of the host's counts), off[n_steps] = n_units
struct LambdaOff {
    int32_t off[kLamT + 1];
};
// counts[t] = the episodes longer than t: never negative, never growing, summing to n_units -> lo.off.  n_steps in [0, kLamT].
inline bool lambda_offsets(int n_units, int n_steps, const int32_t *counts, LambdaOff &lo) {
    if (n_steps > 0 && !counts) return false;
    long off = 0, prev = 0x7fffffffL;
    for (int t = 0; t < n_steps; ++t) {
        if (counts[t] < 0 || counts[t] > prev) return false;
        lo.off[t] = (int32_t)off;
        off += counts[t];
        prev = counts[t];
        if (off > n_units) return false;
    }
    if (off != n_units) return false;
    for (int t = n_steps; t <= kLamT; ++t) lo.off[t] = (int32_t)off;
    return true;
}

// The packed walk's preamble, run by the whole workgroup: lo.off -> LDS (the return value), and T, the length of this wave's episode
// blockIdx.x * kLamEp + wave: the steps with more than that many units (0 behind the last of the E episodes).
__device__ __forceinline__ const int32_t *lambda_packed_episode(const LambdaOff &lo, int E, int n_steps, int &T) {
    __shared__ int32_t s_off[kLamT + 1];
    for (int t = threadIdx.x; t <= n_steps; t += 256) s_off[t] = lo.off[t];
    __syncthreads();
    const int ep = blockIdx.x * kLamEp + (threadIdx.x >> 6);
    T = 0;
    if (ep < E) {
        for (int t = threadIdx.x & 63; t < n_steps; t += 64) T += (s_off[t + 1] - s_off[t] > ep) ? 1 : 0;
        for (int o = 32; o > 0; o >>= 1) T += __shfl_xor(T, o);
    }
    return s_off;
}

// Phase B, one lane per episode, on the episode's LDS rows: s_g holds Q'[t] and leaves as G[t]; bit 0 of s_f[t] is `terminated`;
// L = the leading steps with padded == 0.  One float operation after the other, t backwards: a parallel scan would round differently.
__device__ __forceinline__ void lambda_walk_back(float *s_g, const float *s_r, const uint8_t *s_f, int L, int T, float gamma, float lam) {
    const float om = 1.0f - lam;
    float g_next = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
        const float q = s_g[t];
        const float y = t >= L - 1 ? q : (om * q) + (lam * g_next);
        const float nt = 1.0f - ((s_f[t] & 1) ? 1.0f : 0.0f);
        const float g = s_r[t] + (gamma * y) * nt;
        s_g[t] = g;
        g_next = g;
    }
}

}  // namespace
