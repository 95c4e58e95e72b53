/*
 * vdn_double.h -- C ABI of the double-Q targets of the VDN learn (built into libvdn_ops.so beside vdn_ops.h, vdn_tail.h and
 * vdn_lambda.h, whose conventions and error codes apply): the forward entry points of vdn_lambda.h with Q'[t], the target side's
 * contribution at step t, formed by double Q-learning: a SELECTOR (the eval network one step ahead, detached) chooses each
 * agent's next action and the target network values it.  Everything behind Q'[t] is what vdn_lambda.h states: the one-step target
 * r + (gamma * Q') * nt at lam == 0, the lambda walk at lam > 0, mask, sums.  The backward entry points are those of the one-step
 * block (vdn_td_backward, vdn_td_backward_packed_pad): they read only d_mtd, d_mask and d_u.
 *
 * The rule, per (episode, step) slot and agent i, A = n_actions:
 *     s(a)   = avail_next[i][a] == 0 ? -9999999.0f : q_sel[i][a]
 *     a* = 0; m = s(0); for a = 1 .. A-1: if (s(a) > m) { m = s(a); a* = a; }
 *     v_i    = avail_next[i][a*] == 0 ? -9999999.0f : q_target[i][a*]
 *     Q'     = the sum of v_i over i in index order, float32 (as vdn_td_forward adds)
 * The first maximum wins; a NaN never displaces an earlier value; a row with no available action picks 0.  With q_sel == q_target Q'
 * is the value of vdn_td_forward bit for bit (the value at a row's own first maximum is its maximum).  A lane walks a row of at most
 * 127 actions twice: once over the selector, then one read of the target.
 *
 * d_picks (int8, one row of n_agents per output slot, may be NULL) receives a* of every slot, padded ones included.
 *
 * lam == 0 runs the row-parallel kernel of vdn_td_forward_sums: d_part is float32[vdn_td_sum_parts(number of slots)] and the sums
 * have the bits of vdn_td_forward_sums / vdn_td_forward_packed_sums when q_sel == q_target.  lam > 0 runs the walk of vdn_lambda.h:
 * d_part is float32[vdn_td_lambda_sum_parts(number of episodes)].  Either way the hand-off goes through the SAME device word as the
 * other *_sums entry points: launches of all of them on one device must be ordered on one stream.
 *
 * Packed form: the selector has units of its own.  The selector of unit j is unit d_sel_units[j] of d_q_sel (d_sel_units == NULL: unit
 * j, and then n_sel_units >= n_units is required).  A d_sel_units[j] outside [0, n_sel_units) is never used as an index: that slot's
 * d_mtd is NaN, its picks are -1 and it is counted once in *d_bad_actions (once, too, if its action is outside [0, n_actions) as
 * well).  Its Q' is formed with the slot's own target rows as the selector, so at lam == 0 no other slot changes and at lam > 0 the
 * earlier slots of its episode see that finite Q'.  An action outside [0, n_actions) behaves as in vdn_td_forward.
 *
 * VDN_ERR_BAD_ARG, before anything is launched and with every output untouched: whatever the entry points of vdn_lambda.h refuse
 * (at lam == 0 as well: T or n_steps above VDN_LAMBDA_MAX_T; the packed form reads counts only when lam > 0), d_q_sel == NULL,
 * n_sel_units < 1, d_sel_units == NULL with n_sel_units < n_units.
 */
#ifndef VDN_DOUBLE_H
#define VDN_DOUBLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* vdn_td_lambda_forward_sums (vdn_lambda.h) with double-Q targets.  d_q_sel float32[T][B][n_agents][n_actions], the layout of
 * d_q_target; d_picks int8[B*T][n_agents] (may be NULL). */
int vdn_td_double_forward_sums(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r,
                               const int8_t *d_avail_next, const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T,
                               int32_t t_limit, int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd, float *d_mask,
                               int32_t *d_bad_actions, float *d_part, float *d_sums, float lam, float *d_targets, const float *d_q_sel,
                               int8_t *d_picks, void *stream);

/* vdn_td_lambda_forward_packed_sums (vdn_lambda.h) with double-Q targets.  d_q_sel float32[n_sel_units][n_agents][n_actions];
 * d_sel_units int32[n_units] (may be NULL); d_picks int8[n_units][n_agents] (may be NULL).  counts / n_steps: required when lam > 0. */
int vdn_td_double_forward_packed_sums(const float *d_q_eval, const float *d_q_target, const int32_t *d_units, int32_t n_units,
                                      const int8_t *d_u, const float *d_r, const int8_t *d_avail_next, const uint8_t *d_terminated,
                                      const uint8_t *d_padded, int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd,
                                      float *d_mask, int32_t *d_bad_actions, float *d_part, float *d_sums, float lam, float *d_targets,
                                      int32_t n_steps, const int32_t *counts, const float *d_q_sel, int32_t n_sel_units,
                                      const int32_t *d_sel_units, int8_t *d_picks, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VDN_DOUBLE_H */
