/*
 * qmix_lambda.h -- C ABI of the lambda-return targets of the QMIX learn (built into libqmix_ops.so beside qmix_ops.h and
 * qmix_packed.h, whose conventions, error codes, qmix_mixer and build limits apply): qmix_mix_td_forward /
 * qmix_mix_td_forward_packed with the one-step target replaced by the lambda-return of the episode.  The backward entry points are
 * those of the one-step block (qmix_mix_td_backward, qmix_mix_td_backward_packed): they read only d_mtd, d_mask, d_q_eval, d_u and
 * the eval P.
 *
 * The rule is that of vdn_lambda.h with the mixers in the place of the sums.  Per episode: T = the steps the call covers, L = the
 * count of leading steps with padded == 0, Q'[t] = the target mixer's q_tot of step t and e[t] = the eval mixer's q_tot, both the
 * very values qmix_mix_td_forward forms for the row.  With nt[t] = 1 - terminated[t] and om = 1.0f - lam formed once, every operation
 * a float32 operation in this order, for t = T-1 down to 0:
 *     y[t]   = Q'[t]                              if t >= L-1  (a padded slot, or the episode's last valid step: the one-step target)
 *     y[t]   = (om * Q'[t]) + (lam * G[t+1])      otherwise
 *     G[t]   = r[t] + (gamma * y[t]) * nt[t]
 *     mtd[t] = mask[t] * (e[t] - G[t]),  mask[t] = 1 - padded[t]       (QMIX's sign, which its backward depends on)
 * lam == 0 gives the bits of the one-step entry points.
 *
 * TWO launches on the caller's stream.  The first is the row-parallel kernel of qmix_mix_td_forward, writing each row's two q_tot
 * into d_q_tot_eval / d_q_tot_target instead of forming mtd; the second walks every episode backwards, one lane per episode (the
 * result is that of the loop above bit for bit; a parallel scan would round differently), and writes d_mtd, d_mask and d_targets.
 * d_q_tot_eval and d_q_tot_target are therefore outputs AND the hand-off between the launches: required, float32 with one element
 * per row, distinct from every other buffer of the call.  A row with an action outside [0, n_actions) has d_q_tot_eval = NaN, so
 * its d_mtd is NaN; G does not read e, so no other slot changes.  The row is counted once in *d_bad_actions (may be NULL).
 * No float atomics, no sums: two calls on the same inputs give identical bits.
 *
 * QMIX_ERR_BAD_ARG, before anything is launched and with every output untouched: lam outside [0, 1] or NaN, T or n_steps above
 * QMIX_LAMBDA_MAX_T, counts that grow, are negative or do not sum to n_units, a NULL required pointer (only d_bad_actions,
 * d_targets and d_p_target_row may be NULL), and what the one-step entry points refuse (QMIX_ERR_UNSUPPORTED outside the build
 * limits, as there).
 */
#ifndef QMIX_LAMBDA_H
#define QMIX_LAMBDA_H

#include <stdint.h>

#include "qmix_ops.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QMIX_LAMBDA_MAX_T 512        /* steps per episode: 2 * (128 + 128), the longest episode limit of the environments */
#define QMIX_LAMBDA_WG_EPISODES 4    /* the walk: one wave per episode, four waves per workgroup */

/* qmix_mix_td_forward (qmix_ops.h) on lambda-returns.  d_q_tot_eval / d_q_tot_target float32[B*T], row b * T + t: e and Q'.
 * d_targets float32[B*T] receives G (may be NULL); the episode lengths L come from d_padded on the device. */
int qmix_mix_td_lambda_forward(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r,
                               const int8_t *d_avail_next, const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T,
                               int32_t t_limit, int32_t n_agents, int32_t n_actions, const float *d_p_eval, int32_t p_eval_rows,
                               int32_t p_eval_off, const float *d_p_target, int32_t p_target_rows, int32_t p_target_off,
                               int32_t hyper_hidden, int32_t qmix_hidden, const qmix_mixer *eval, const qmix_mixer *target, float gamma,
                               float *d_mtd, float *d_mask, int32_t *d_bad_actions, float lam, float *d_q_tot_eval,
                               float *d_q_tot_target, float *d_targets, void *stream);

/* qmix_mix_td_forward_packed (qmix_packed.h) on lambda-returns.  counts: HOST int32[n_steps], non-increasing, summing to n_units;
 * counts[t] = the episodes longer than t (as vdn_td_lambda_forward_packed_sums, vdn_lambda.h).  Step t of the episode of rank e is
 * unit sum(counts[0..t)) + e; its length T is the number of t with counts[t] > e, and L is counted over those steps.
 * d_q_tot_eval / d_q_tot_target / d_targets float32[n_units], one element per unit.  n_units == 0 launches nothing. */
int qmix_mix_td_lambda_forward_packed(const float *d_q_eval, const float *d_q_target, const int32_t *d_units, int32_t n_units,
                                      const int8_t *d_u, const float *d_r, const int8_t *d_avail_next, const uint8_t *d_terminated,
                                      const uint8_t *d_padded, int32_t n_agents, int32_t n_actions, const float *d_p_eval,
                                      const float *d_p_target, const int32_t *d_p_target_row, int32_t hyper_hidden,
                                      int32_t qmix_hidden, const qmix_mixer *eval, const qmix_mixer *target, float gamma, float *d_mtd,
                                      float *d_mask, int32_t *d_bad_actions, float lam, float *d_q_tot_eval, float *d_q_tot_target,
                                      float *d_targets, int32_t n_steps, const int32_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QMIX_LAMBDA_H */
