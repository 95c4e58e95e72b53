// qmix_ops.hip -- the mixing + TD block of QMIX.learn (policy/qmix.py:104-122, network/qmix_net.py) after the hypernetworks'
// first-layer GEMM, one kernel each way.  See include/qmix_ops.h.
//
// Eight lanes share one (episode, step) row: lane `slot` owns the mixer columns j = slot, slot + 8, ... (M / 8 of them), so that
// the n x M hypernetwork outputs of a row are spread over the lanes; the row's sums over j are butterfly reductions inside the
// group of eight.  Every row is computed and written by its own group: no atomics besides the bad-action counter.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/qmix_ops.h"

#define HIP_ABI_TAG "qmix_ops"
#define HIP_ABI_ERR QMIX_ERR_HIP
#include "hip_abi.h"

namespace {

constexpr int kM = 32;            // qmix_hidden_dim of every TrainParas table
constexpr int kLanes = 8;         // lanes per row
constexpr int kJ = kM / kLanes;   // mixer columns per lane
constexpr int kMaxN = 16;         // droplets (DMFB_MAX_AGENTS)
constexpr int kMaxA = 16;
constexpr int kBlock = 256;

struct Dims {
    int B, T, Tl, n, A;
    int p_rows, p_off;    // eval P layout
    int pt_rows, pt_off;  // target P layout
};

__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = 1; m < kLanes; m <<= 1) v += __shfl_xor(v, m, kLanes);
    return v;
}

template <int H> __device__ __forceinline__ float dot(const float *__restrict__ w, const float (&h)[H]) {
    const float4 *w4 = reinterpret_cast<const float4 *>(w);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < H / 4; ++k) {
        const float4 v = w4[k];
        acc = fmaf(v.x, h[4 * k], acc);
        acc = fmaf(v.y, h[4 * k + 1], acc);
        acc = fmaf(v.z, h[4 * k + 2], acc);
        acc = fmaf(v.w, h[4 * k + 3], acc);
    }
    return acc;
}

__device__ __forceinline__ float elu(float x) { return x > 0.f ? x : expm1f(x); }
__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// q_tot of one row (every lane of the group returns it)
template <int H>
__device__ float mix_row(const float *__restrict__ P, const qmix_mixer &w, const float (&q)[kMaxN], int n, int slot) {
    float h1[H], h2[H];
#pragma unroll
    for (int h = 0; h < H; ++h) { h1[h] = fmaxf(P[h], 0.f); h2[h] = fmaxf(P[H + h], 0.f); }
    float acc = 0.f, accb = 0.f;
#pragma unroll
    for (int jj = 0; jj < kJ; ++jj) {
        const int j = slot + kLanes * jj;
        float pre = 0.f;
#pragma unroll
        for (int i = 0; i < kMaxN; ++i)
            if (i < n) pre = fmaf(q[i], fabsf(w.b1[i * kM + j] + dot<H>(w.w1 + (size_t)(i * kM + j) * H, h1)), pre);
        pre += P[2 * H + j];
        acc = fmaf(elu(pre), fabsf(w.b2[j] + dot<H>(w.w2 + (size_t)j * H, h2)), acc);
        accb = fmaf(w.wb[j], fmaxf(P[2 * H + kM + j], 0.f), accb);
    }
    return group_sum(acc) + (group_sum(accb) + w.bb[0]);
}

template <int H>
__global__ __launch_bounds__(kBlock) void k_mix_forward(Dims d, const float *__restrict__ qe, const float *__restrict__ qt,
                                                        const int8_t *__restrict__ u, const float *__restrict__ r,
                                                        const int8_t *__restrict__ avail, const uint8_t *__restrict__ term,
                                                        const uint8_t *__restrict__ padded, const float *__restrict__ pe,
                                                        const float *__restrict__ pt, qmix_mixer we, qmix_mixer wt, float gamma,
                                                        float *__restrict__ mtd, float *__restrict__ maskf, int32_t *__restrict__ bad) {
    const long gid = (long)blockIdx.x * kBlock + threadIdx.x;
    const long rows = (long)d.B * d.T;
    const bool valid = gid / kLanes < rows;
    const long row = valid ? gid / kLanes : 0;   // idle lanes of the last group follow row 0 (the shuffles need every lane)
    const int slot = (int)(gid % kLanes);
    const int b = (int)(row / d.T), t = (int)(row - (long)b * d.T);
    const size_t ep = (size_t)b * d.Tl + t;
    const size_t q0 = ((size_t)t * d.B + b) * d.n * d.A;
    const int A = d.A;
    float q_e[kMaxN], q_t[kMaxN];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < kMaxN; ++i) {
        q_e[i] = 0.f; q_t[i] = 0.f;
        if (i < d.n) {
            int a_taken = (int)u[ep * d.n + i];
            if ((unsigned)a_taken >= (unsigned)A) { ok = false; a_taken = 0; }   // torch.gather raises; never read out of bounds
            q_e[i] = qe[q0 + (size_t)i * A + a_taken];
            float m = -3.4e38f;
            for (int a = 0; a < A; ++a) {
                const float v = avail[(ep * d.n + i) * A + a] == 0 ? -9999999.0f : qt[q0 + (size_t)i * A + a];
                m = v > m ? v : m;
            }
            q_t[i] = m;
        }
    }
    const float tot_e = mix_row<H>(pe + ((size_t)b * d.p_rows + t + d.p_off) * (2 * H + 2 * kM), we, q_e, d.n, slot);
    const float tot_t = mix_row<H>(pt + ((size_t)b * d.pt_rows + t + d.pt_off) * (2 * H + 2 * kM), wt, q_t, d.n, slot);
    if (valid && slot == 0) {
        const float not_term = 1.0f - (term[ep] ? 1.0f : 0.0f);
        const float target = r[ep] + (gamma * tot_t) * not_term;
        const float mk = 1.0f - (padded[ep] ? 1.0f : 0.0f);
        mtd[row] = ok ? mk * (tot_e - target) : __builtin_nanf("");
        maskf[row] = mk;
        if (!ok && bad) atomicAdd(bad, 1);
    }
}

template <int H>
__global__ __launch_bounds__(kBlock) void k_mix_backward(Dims d, const float *__restrict__ mtd, const float *__restrict__ maskf,
                                                         const float *__restrict__ qe, const int8_t *__restrict__ u,
                                                         const float *__restrict__ pe, qmix_mixer w, const float *__restrict__ g0,
                                                         float *__restrict__ gq, float *__restrict__ gp, float *__restrict__ z,
                                                         float *__restrict__ x) {
    constexpr int F = 2 * H + 2 * kM, XW = 2 * H + kM + 3;
    const long gid = (long)blockIdx.x * kBlock + threadIdx.x;
    const long rows = (long)d.B * d.T;
    const bool valid = gid / kLanes < rows;
    const long row = valid ? gid / kLanes : 0;
    const int slot = (int)(gid % kLanes);
    const int b = (int)(row / d.T), t = (int)(row - (long)b * d.T);
    const int n = d.n, A = d.A, ZW = n * kM + kM + 1;
    const size_t ep = (size_t)b * d.Tl + t;
    const size_t q0 = ((size_t)t * d.B + b) * n * A;
    const float g = ((2.0f * mtd[row]) * maskf[row]) * g0[0];   // d num / d q_tot_eval of this row
    float q[kMaxN], dq[kMaxN];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < kMaxN; ++i) {
        q[i] = 0.f; dq[i] = 0.f;
        if (i < n) {
            int a_taken = (int)u[ep * n + i];
            if ((unsigned)a_taken >= (unsigned)A) { ok = false; a_taken = 0; }   // mtd is NaN for the row: every gradient below is NaN
            q[i] = qe[q0 + (size_t)i * A + a_taken];
        }
    }
    const float *P = pe + ((size_t)b * d.p_rows + t + d.p_off) * F;
    float *dP = gp + ((size_t)b * d.p_rows + t + d.p_off) * F;
    float *Z = z + (size_t)row * ZW;
    float *X = x + (size_t)row * XW;
    float h1[H], h2[H], dh1[H], dh2[H];
#pragma unroll
    for (int h = 0; h < H; ++h) { h1[h] = fmaxf(P[h], 0.f); h2[h] = fmaxf(P[H + h], 0.f); dh1[h] = 0.f; dh2[h] = 0.f; }
#pragma unroll
    for (int jj = 0; jj < kJ; ++jj) {
        const int j = slot + kLanes * jj;
        float zi[kMaxN];
        float pre = 0.f;
#pragma unroll
        for (int i = 0; i < kMaxN; ++i) {
            zi[i] = 0.f;
            if (i < n) {
                zi[i] = w.b1[i * kM + j] + dot<H>(w.w1 + (size_t)(i * kM + j) * H, h1);
                pre = fmaf(q[i], fabsf(zi[i]), pre);
            }
        }
        pre += P[2 * H + j];
        const float hid = elu(pre);
        const float z2 = w.b2[j] + dot<H>(w.w2 + (size_t)j * H, h2);
        const float dpre = (g * fabsf(z2)) * (pre > 0.f ? 1.f : expf(pre));
        const float dz2 = sgn(z2) * (g * hid);
        const float hbp = P[2 * H + kM + j];
        if (valid) {
            Z[n * kM + j] = dz2;
            dP[2 * H + j] = dpre;
            dP[2 * H + kM + j] = hbp > 0.f ? g * w.wb[j] : 0.f;
            X[2 * H + 2 + j] = fmaxf(hbp, 0.f);
        }
        const float *w2r = w.w2 + (size_t)j * H;
#pragma unroll
        for (int h = 0; h < H; ++h) dh2[h] = fmaf(w2r[h], dz2, dh2[h]);
#pragma unroll
        for (int i = 0; i < kMaxN; ++i) {
            if (i < n) {
                const float dz1 = sgn(zi[i]) * (q[i] * dpre);
                if (valid) Z[i * kM + j] = dz1;
                const float *w1r = w.w1 + (size_t)(i * kM + j) * H;
#pragma unroll
                for (int h = 0; h < H; ++h) dh1[h] = fmaf(w1r[h], dz1, dh1[h]);
                dq[i] = fmaf(fabsf(zi[i]), dpre, dq[i]);
            }
        }
    }
#pragma unroll
    for (int h = 0; h < H; ++h) { dh1[h] = group_sum(dh1[h]); dh2[h] = group_sum(dh2[h]); }
#pragma unroll
    for (int i = 0; i < kMaxN; ++i) dq[i] = group_sum(dq[i]);
    if (!valid) return;
#pragma unroll
    for (int h = 0; h < H; ++h) {
        if (h % kLanes == slot) {
            dP[h] = P[h] > 0.f ? dh1[h] : 0.f;
            dP[H + h] = P[H + h] > 0.f ? dh2[h] : 0.f;
            X[h] = h1[h];
            X[H + 1 + h] = h2[h];
        }
    }
    if (slot == 0) {
        X[H] = 1.f; X[2 * H + 1] = 1.f; X[2 * H + 2 + kM] = 1.f;
        Z[n * kM + kM] = g;
    }
#pragma unroll
    for (int i = 0; i < kMaxN; ++i) {
        if (i < n) {
            const int a_taken = (int)u[ep * n + i];
            float *out = gq + q0 + (size_t)i * A;
            // a bad action anywhere in the row: the whole row of grad_q is NaN, every agent's entries
            for (int a = slot; a < A; a += kLanes) out[a] = (!ok || a == a_taken) ? dq[i] : 0.f;
        }
    }
}

int check(int B, int T, int t_limit, int n, int A, int H, int M, const qmix_mixer *m) {
    if (B <= 0 || T <= 0 || t_limit < T || n <= 0 || A <= 0 || !m) return QMIX_ERR_BAD_ARG;
    if (M != kM || (H != 24 && H != 32) || n > kMaxN || A > kMaxA) return QMIX_ERR_UNSUPPORTED;
    const uintptr_t al = (uintptr_t)m->w1 | (uintptr_t)m->w2;   // rows are read as float4
    if (!m->w1 || !m->b1 || !m->w2 || !m->b2 || !m->wb || !m->bb || (al & 15)) return QMIX_ERR_BAD_ARG;
    return QMIX_OK;
}

dim3 grid(int B, int T) { return dim3((unsigned)(((long)B * T * kLanes + kBlock - 1) / kBlock)); }

}  // namespace

extern "C" {

int qmix_mix_td_forward(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r, const int8_t *d_avail_next,
                        const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T, int32_t t_limit, int32_t n_agents,
                        int32_t n_actions, const float *d_p_eval, int32_t p_eval_rows, int32_t p_eval_off, const float *d_p_target,
                        int32_t p_target_rows, int32_t p_target_off, int32_t hyper_hidden, int32_t qmix_hidden, const qmix_mixer *eval,
                        const qmix_mixer *target, float gamma, float *d_mtd, float *d_mask, int32_t *d_bad_actions, void *stream) {
    int rc = check(B, T, t_limit, n_agents, n_actions, hyper_hidden, qmix_hidden, eval);
    if (!rc) rc = check(B, T, t_limit, n_agents, n_actions, hyper_hidden, qmix_hidden, target);
    if (rc) return rc;
    if (!d_q_eval || !d_q_target || !d_u || !d_r || !d_avail_next || !d_terminated || !d_padded || !d_p_eval || !d_p_target || !d_mtd ||
        !d_mask || p_eval_off < 0 || p_target_off < 0 || p_eval_rows < T + p_eval_off || p_target_rows < T + p_target_off)
        return QMIX_ERR_BAD_ARG;
    const Dims d{B, T, t_limit, n_agents, n_actions, p_eval_rows, p_eval_off, p_target_rows, p_target_off};
    hipStream_t s = (hipStream_t)stream;
    if (hyper_hidden == 24)
        LAUNCH(k_mix_forward<24>, grid(B, T), dim3(kBlock), 0, s, d, d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded,
               d_p_eval, d_p_target, *eval, *target, gamma, d_mtd, d_mask, d_bad_actions);
    else
        LAUNCH(k_mix_forward<32>, grid(B, T), dim3(kBlock), 0, s, d, d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded,
               d_p_eval, d_p_target, *eval, *target, gamma, d_mtd, d_mask, d_bad_actions);
    return QMIX_OK;
}

int qmix_mix_td_backward(const float *d_mtd, const float *d_mask, const float *d_q_eval, const int8_t *d_u, int32_t B, int32_t T,
                         int32_t t_limit, int32_t n_agents, int32_t n_actions, const float *d_p_eval, int32_t p_eval_rows,
                         int32_t p_eval_off, int32_t hyper_hidden, int32_t qmix_hidden, const qmix_mixer *eval,
                         const float *d_grad_num, float *d_grad_q, float *d_grad_p, float *d_z, float *d_x, void *stream) {
    int rc = check(B, T, t_limit, n_agents, n_actions, hyper_hidden, qmix_hidden, eval);
    if (rc) return rc;
    if (!d_mtd || !d_mask || !d_q_eval || !d_u || !d_p_eval || !d_grad_num || !d_grad_q || !d_grad_p || !d_z || !d_x || p_eval_off < 0 ||
        p_eval_rows < T + p_eval_off)
        return QMIX_ERR_BAD_ARG;
    const Dims d{B, T, t_limit, n_agents, n_actions, p_eval_rows, p_eval_off, 0, 0};
    hipStream_t s = (hipStream_t)stream;
    if (hyper_hidden == 24)
        LAUNCH(k_mix_backward<24>, grid(B, T), dim3(kBlock), 0, s, d, d_mtd, d_mask, d_q_eval, d_u, d_p_eval, *eval, d_grad_num,
               d_grad_q, d_grad_p, d_z, d_x);
    else
        LAUNCH(k_mix_backward<32>, grid(B, T), dim3(kBlock), 0, s, d, d_mtd, d_mask, d_q_eval, d_u, d_p_eval, *eval, d_grad_num,
               d_grad_q, d_grad_p, d_z, d_x);
    return QMIX_OK;
}

int qmix_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
