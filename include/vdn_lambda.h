/*
 * vdn_lambda.h -- C ABI of the TD(lambda) targets of the VDN learn (built into libvdn_ops.so beside vdn_ops.h and vdn_tail.h, whose
 * conventions and error codes apply): vdn_td_forward_sums / vdn_td_forward_packed_sums with the one-step target replaced by the
 * lambda-return of the episode, one launch per learn.  The backward entry points are those of the one-step block (vdn_td_backward,
 * vdn_td_backward_packed_pad): they read only d_mtd, d_mask and d_u.
 *
 * The rule, per episode: T = the steps the call covers, L = the count of leading steps with padded == 0.  Q'[t] (the sum over the
 * agents of the best available target Q, unavailable actions at -9999999) and e[t] (the sum of the taken actions' eval Q) are those
 * of vdn_td_forward, agents summed in index order.  With nt[t] = 1 - terminated[t] and om = 1.0f - lam formed once, every operation a
 * float32 operation in this order, for t = T-1 down to 0:
 *     y[t]   = Q'[t]                              if t >= L-1  (a padded slot, or the episode's last valid step: the one-step target)
 *     y[t]   = (om * Q'[t]) + (lam * G[t+1])      otherwise
 *     G[t]   = r[t] + (gamma * y[t]) * nt[t]
 *     mtd[t] = mask[t] * (G[t] - e[t]),  mask[t] = 1 - padded[t]
 * The walk over t is serial (one lane per episode): the result is that of the loop above bit for bit.  A terminated step cuts the
 * return through nt wherever it stands.  An action outside [0, n_actions) makes that slot's d_mtd NaN and is counted in
 * *d_bad_actions as in vdn_td_forward; G does not read u, so no other slot changes.  lam == 0 gives the one-step target.
 *
 * The two sums (d_sums, d_part) are formed as in vdn_tail.h: fixed order, no float atomics, two launches on the same inputs give
 * the same bits; the hand-off goes through the SAME device word as the other *_sums entry points, so launches of all of them on one
 * device must be ordered on one stream.  One workgroup serves VDN_LAMBDA_WG_EPISODES episodes, so d_part is
 * float32[vdn_td_lambda_sum_parts(number of episodes)] here (not vdn_td_sum_parts of the slot count).
 *
 * VDN_ERR_BAD_ARG, before anything is launched and with every output untouched: lam outside [0, 1] or NaN, T or n_steps above
 * VDN_LAMBDA_MAX_T, counts that grow, are negative or do not sum to n_units, a NULL required pointer, and what vdn_td_forward_sums
 * refuses.
 */
#ifndef VDN_LAMBDA_H
#define VDN_LAMBDA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDN_LAMBDA_MAX_T 512        /* steps per episode: 2 * (128 + 128), the longest episode limit of the environments */
#define VDN_LAMBDA_WG_EPISODES 4    /* one wave per episode, four waves per workgroup */

/* floats of d_part for n_episodes episodes (B, or counts[0] of the packed form) */
int vdn_td_lambda_sum_parts(int64_t n_episodes);

/* vdn_td_forward_sums (vdn_tail.h) on lambda-returns.  d_targets float32[B*T] receives G (may be NULL); the episode lengths L come
 * from d_padded on the device.  d_sums may be NULL (then d_part is not used). */
int vdn_td_lambda_forward_sums(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r,
                               const int8_t *d_avail_next, const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T,
                               int32_t t_limit, int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd, float *d_mask,
                               int32_t *d_bad_actions, float *d_part, float *d_sums, float lam, float *d_targets, void *stream);

/* vdn_td_forward_packed_sums (vdn_tail.h) on lambda-returns.  counts: HOST int32[n_steps], non-increasing, summing to n_units;
 * counts[t] = the episodes longer than t (the role step_rows plays for gru_seq_forward_packed, per episode instead of per row).
 * Step t of the episode of rank e is unit sum(counts[0..t)) + e; its length T is the number of t with counts[t] > e, and L is counted
 * over those steps.  d_targets float32[n_units] receives G (may be NULL). */
int vdn_td_lambda_forward_packed_sums(const float *d_q_eval, const float *d_q_target, const int32_t *d_units, int32_t n_units,
                                      const int8_t *d_u, const float *d_r, const int8_t *d_avail_next, const uint8_t *d_terminated,
                                      const uint8_t *d_padded, int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd,
                                      float *d_mask, int32_t *d_bad_actions, float *d_part, float *d_sums, float lam, float *d_targets,
                                      int32_t n_steps, const int32_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VDN_LAMBDA_H */
