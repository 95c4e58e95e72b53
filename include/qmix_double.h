/*
 * qmix_double.h -- C ABI of the double-Q targets of the QMIX learn (built into libqmix_ops.so beside qmix_ops.h, qmix_packed.h and
 * qmix_lambda.h, whose conventions, error codes, qmix_mixer and build limits apply): the forward entry points of qmix_lambda.h with
 * the per-agent values that go into the TARGET mixer formed by double Q-learning: a SELECTOR (the eval network one step ahead,
 * detached) chooses each agent's next action and the target network values it.  Everything behind those values is the existing row
 * body: the two mixers, the one-step target r + (gamma * q_tot_target) * nt at lam == 0, the totals and the walk of qmix_lambda.h at
 * lam > 0, mask, QMIX's sign.  The backward entry points are those of the one-step block (qmix_mix_td_backward,
 * qmix_mix_td_backward_packed): they read only d_mtd, d_mask, d_q_eval, d_u and the eval P.
 *
 * The rule (that of vdn_double.h), per (episode, step) row and agent i, A = n_actions:
 *     s(a)   = avail_next[i][a] == 0 ? -9999999.0f : q_sel[i][a]
 *     a* = 0; m = s(0); for a = 1 .. A-1: if (s(a) > m) { m = s(a); a* = a; }
 *     q_t[i] = avail_next[i][a*] == 0 ? -9999999.0f : q_target[i][a*]
 * and q_t[i] goes into the target mixer where qmix_mix_td_forward puts the maximum of the target row.  The first maximum wins; a NaN
 * never displaces an earlier value; a row with no available action picks 0.  With d_q_sel == d_q_target, d_sel_units == NULL and
 * finite Q values, d_mtd and d_mask have the bits of the existing one-step and lambda entry points (the value at a row's own first
 * maximum is its maximum).
 *
 * d_picks (int8, one row of n_agents per output row, may be NULL) receives a* of every output row, padded slots included.
 *
 * lam == 0: ONE launch, the row kernel of qmix_mix_td_forward with the selector.  d_q_tot_eval, d_q_tot_target, n_steps and counts are
 * not read and may be NULL / 0; d_targets (may be NULL) receives r + (gamma * q_tot_target) * nt of every row.
 * lam > 0: TWO launches as in qmix_lambda.h: the rows' totals with the selector, then the unchanged walk.  d_q_tot_eval and
 * d_q_tot_target are then required outputs and the hand-off between the launches.
 *
 * Packed form: the selector has units of its own.  The selector of unit j is unit d_sel_units[j] of d_q_sel (d_sel_units == NULL:
 * unit j, and then n_sel_units >= n_units is required).  A d_sel_units[j] outside [0, n_sel_units) is never used as an index: that
 * row's picks are -1, its d_mtd is NaN (under lambda its d_q_tot_eval too) and it is counted once in *d_bad_actions (once, too, if its
 * action is outside [0, n_actions) as well).  Its target q_tot is formed with the row's own target rows as the selector, so at
 * lam == 0 no other row changes and at lam > 0 the earlier slots of its episode see that finite value.  An action outside
 * [0, n_actions) behaves as in qmix_mix_td_forward.
 *
 * No LDS in the row kernel, no atomics besides the bad-action counter, no sums: two calls on the same inputs give identical bits.
 *
 * QMIX_ERR_BAD_ARG, before anything is launched and with every output untouched: whatever the entry point of the same form and
 * lambda refuses (qmix_mix_td_forward / qmix_mix_td_forward_packed at lam == 0, those of qmix_lambda.h at lam > 0), d_q_sel == NULL,
 * n_sel_units < 1, d_sel_units == NULL with n_sel_units < n_units, lam outside [0, 1] or NaN.  QMIX_ERR_UNSUPPORTED outside the
 * build limits, as there.
 */
#ifndef QMIX_DOUBLE_H
#define QMIX_DOUBLE_H

#include <stdint.h>

#include "qmix_ops.h"

#ifdef __cplusplus
extern "C" {
#endif

/* qmix_mix_td_lambda_forward (qmix_lambda.h) with double-Q targets.  d_q_sel float32[T][B][n_agents][n_actions], the layout of
 * d_q_target; d_picks int8[B*T][n_agents] (may be NULL). */
int qmix_mix_td_double_forward(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r,
                               const int8_t *d_avail_next, const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T,
                               int32_t t_limit, int32_t n_agents, int32_t n_actions, const float *d_p_eval, int32_t p_eval_rows,
                               int32_t p_eval_off, const float *d_p_target, int32_t p_target_rows, int32_t p_target_off,
                               int32_t hyper_hidden, int32_t qmix_hidden, const qmix_mixer *eval, const qmix_mixer *target, float gamma,
                               float *d_mtd, float *d_mask, int32_t *d_bad_actions, float lam, float *d_q_tot_eval,
                               float *d_q_tot_target, float *d_targets, const float *d_q_sel, int8_t *d_picks, void *stream);

/* qmix_mix_td_lambda_forward_packed (qmix_lambda.h) with double-Q targets.  d_q_sel float32[n_sel_units][n_agents][n_actions];
 * d_sel_units int32[n_units] (may be NULL); d_picks int8[n_units][n_agents] (may be NULL).  counts / n_steps: read when lam > 0. */
int qmix_mix_td_double_forward_packed(const float *d_q_eval, const float *d_q_target, const int32_t *d_units, int32_t n_units,
                                      const int8_t *d_u, const float *d_r, const int8_t *d_avail_next, const uint8_t *d_terminated,
                                      const uint8_t *d_padded, int32_t n_agents, int32_t n_actions, const float *d_p_eval,
                                      const float *d_p_target, const int32_t *d_p_target_row, int32_t hyper_hidden,
                                      int32_t qmix_hidden, const qmix_mixer *eval, const qmix_mixer *target, float gamma, float *d_mtd,
                                      float *d_mask, int32_t *d_bad_actions, float lam, float *d_q_tot_eval, float *d_q_tot_target,
                                      float *d_targets, int32_t n_steps, const int32_t *counts, const float *d_q_sel,
                                      int32_t n_sel_units, const int32_t *d_sel_units, int8_t *d_picks, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QMIX_DOUBLE_H */
