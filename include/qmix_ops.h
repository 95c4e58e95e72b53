/*
 * qmix_ops.h -- C ABI of the mixing + TD block of QMIX.learn (reference policy/qmix.py:104-122 and network/qmix_net.py), fused.
 *
 * QMixNet's hypernetworks read the global state s.  Their FIRST layers (hyper_w1[0], hyper_w2[0], hyper_b1, hyper_b2[0]) are
 * one BLAS GEMM against the concatenated weight: P = s W^T + b, P float32 [rows][F], F = 2 * H + 2 * M (H = hyper_hidden_dim,
 * M = qmix_hidden_dim), columns [hyper_w1[0] (H) | hyper_w2[0] (H) | hyper_b1 (M) | hyper_b2[0] (M)].  Everything after that
 * GEMM runs here, one launch each way, per (episode b, step t):
 *   h1 = relu(P[0:H]), h2 = relu(P[H:2H]), hb = relu(P[2H+M:2H+2M])
 *   w1 = |hyper_w1[2](h1)| (n x M), b1 = P[2H:2H+M], w2 = |hyper_w2[2](h2)| (M), b2 = hyper_b2[2](hb) (scalar)
 *   q_tot = elu(q . w1 + b1) . w2 + b2
 * for the eval network (q = q_eval gathered by u) and the target network (q = max over available actions of q_target, the
 * unavailable ones set to -9999999), then  target = r + gamma * q_tot_target * (1 - terminated),  mtd = mask * (q_tot_eval -
 * target), mask = 1 - padded.  Loss = sum(mtd^2) / sum(mask) stays with the caller.
 *
 * Conventions as vdn_ops.h: plain C types, caller-owned DEVICE buffers, `stream` = hipStream_t as void*, asynchronous, negative
 * error codes.  Q tensors are TIME-MAJOR float32 [T][B][n][A]; the episode tensors are the replay buffer's with `t_limit` slots
 * per episode (u int8[B][t_limit][n][1], r float32, avail_u_next int8[B][t_limit][n][A], terminated / padded uint8).  Row (b, t)
 * of a P tensor is row b * p_rows + t + p_off (p_rows = T + 1, p_off = 0 / 1 for the eval / target P of a state tensor holding
 * s[0..T], as the replay ring stores it).  Build limits: M == 32, H in {24, 32}, n <= 16, A <= 16 (QMIX_ERR_UNSUPPORTED otherwise).
 * No float atomics: two launches on the same inputs give identical bits.
 */
#ifndef QMIX_OPS_H
#define QMIX_OPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QMIX_OK 0
#define QMIX_ERR_BAD_ARG (-1)
#define QMIX_ERR_UNSUPPORTED (-6)
#define QMIX_ERR_HIP (-100)

/* The second hypernetwork layers of one QMixNet (DEVICE pointers, contiguous float32): hyper_w1[2] weight [n*M][H] and bias [n*M],
 * hyper_w2[2] weight [M][H] and bias [M], hyper_b2[2] weight [1][M] and bias [1]. */
typedef struct {
    const float *w1, *b1, *w2, *b2, *wb, *bb;
} qmix_mixer;

/* d_mtd / d_mask float32[B*T], row b * T + t.  An action outside [0, n_actions) is never used as an index: the row's mtd becomes NaN
 * and *d_bad_actions (int32 device counter, may be NULL) is incremented once per such row, as vdn_td_forward does. */
int qmix_mix_td_forward(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r, const int8_t *d_avail_next,
                        const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T, int32_t t_limit, int32_t n_agents,
                        int32_t n_actions, const float *d_p_eval, int32_t p_eval_rows, int32_t p_eval_off, const float *d_p_target,
                        int32_t p_target_rows, int32_t p_target_off, int32_t hyper_hidden, int32_t qmix_hidden, const qmix_mixer *eval,
                        const qmix_mixer *target, float gamma, float *d_mtd, float *d_mask, int32_t *d_bad_actions, void *stream);

/* Gradient of  num = sum(mtd^2), scaled by *d_grad_num (device scalar), w.r.t. the eval side:
 *   d_grad_q float32[T][B][n][A]: every element written (the taken action's entry, zeros elsewhere; a row with an action outside
 *            [0, n_actions), whose mtd is NaN, is NaN in every entry of every agent);
 *   d_grad_p float32, rows of d_p_eval's layout: the rows of steps t < T are written (others untouched), for the weight GEMM
 *            dW = dP^T s and the bias column sums of the first layers;
 *   d_z float32[B*T][n*M + M + 1] and d_x float32[B*T][2H + M + 3]: per-row factors of the second-layer gradients, which are the
 *            GEMMs  Z[:, 0:nM]^T X[:, 0:H+1] -> [hyper_w1[2].weight | .bias],  Z[:, nM:nM+M]^T X[:, H+1:2H+2] -> hyper_w2[2],
 *            Z[:, nM+M:]^T X[:, 2H+2:] -> hyper_b2[2]  (X carries a column of ones behind each factor for the bias). */
int qmix_mix_td_backward(const float *d_mtd, const float *d_mask, const float *d_q_eval, const int8_t *d_u, int32_t B, int32_t T,
                         int32_t t_limit, int32_t n_agents, int32_t n_actions, const float *d_p_eval, int32_t p_eval_rows,
                         int32_t p_eval_off, int32_t hyper_hidden, int32_t qmix_hidden, const qmix_mixer *eval,
                         const float *d_grad_num, float *d_grad_q, float *d_grad_p, float *d_z, float *d_x, void *stream);

int qmix_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif /* QMIX_OPS_H */
