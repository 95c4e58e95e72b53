/*
 * qmix_packed.h -- C ABI of the packed QMIX learn (built into libqmix_ops.so): the mixing + TD block of qmix_ops.h on packed
 * (episode, step) UNITS, i.e. on the valid steps of a length-sorted batch only, and the gather of their global-state rows.
 *
 * The arithmetic of a unit is that of a (b, t) row of qmix_mix_td_forward / _backward: the kernels are the same per-row code
 * instantiated with another index rule, so a unit's outputs have the bits of the padded entry points' row.  What differs is
 * where a row's operands live:
 *   replay tensors   unit j is the step d_units[j] = slot * t_limit + t, indexed in place (as vdn_td_forward_packed, vdn_ops.h)
 *   Q values         rows j*n .. j*n+n-1 of the packed tensors (the layout gru_seq_forward_packed leaves, crnn_ops.h)
 *   P                eval row j; target row d_p_target_row[j] (on a valid step s_next[t] == s[t + 1], so the target rows of
 *                    most units are the eval state rows of the next step's units: one gathered state tensor serves both)
 *
 * Conventions, error codes, qmix_mixer and the build limits (M == 32, H in {24, 32}, n <= 16, A <= 16) are those of qmix_ops.h.
 * A count of 0 (n_units, n_rows) returns QMIX_OK and launches nothing.  QMIX_ERR_BAD_ARG: a negative count, a NULL required
 * pointer (only d_bad_actions and d_p_target_row may be NULL), rows_pad < n_units * n, state_len < 1, n_state_rows < 1.
 * No float atomics: two launches on the same inputs give identical bits.
 */
#ifndef QMIX_PACKED_H
#define QMIX_PACKED_H

#include <stdint.h>

#include "qmix_ops.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Unit j is the step d_units[j] = slot * t_limit + t of the replay tensors, which are indexed in place exactly as
 * vdn_td_forward_packed does (include/vdn_ops.h).  Rows j*n .. j*n+n-1 of d_q_eval / d_q_target (float32[>= n_units*n][A],
 * the layout gru_seq_forward_packed leaves) belong to unit j.  Row j of d_p_eval (float32[n_units][F], F = 2H + 2M) is the
 * eval mixer's first-layer output for the state of unit j.  The target mixer's row for unit j is row d_p_target_row[j]
 * of d_p_target (row j when d_p_target_row is NULL).  d_mtd / d_mask float32[n_units].
 * Arithmetic per unit, bad-action rule and counter: qmix_mix_td_forward. */
int qmix_mix_td_forward_packed(const float *d_q_eval, const float *d_q_target, const int32_t *d_units, int32_t n_units,
                               const int8_t *d_u, const float *d_r, const int8_t *d_avail_next, const uint8_t *d_terminated,
                               const uint8_t *d_padded, int32_t n_agents, int32_t n_actions, const float *d_p_eval,
                               const float *d_p_target, const int32_t *d_p_target_row, int32_t hyper_hidden, int32_t qmix_hidden,
                               const qmix_mixer *eval, const qmix_mixer *target, float gamma, float *d_mtd, float *d_mask,
                               int32_t *d_bad_actions, void *stream);

/* d_grad_q float32[rows_pad][A], rows_pad >= n_units*n: every element written, rows from n_units*n on as zeros (the
 * GEMM padding rows of the packed learn, as vdn_td_backward_packed_pad).  d_grad_p float32[n_units][F], d_z
 * float32[n_units][n*M+M+1], d_x float32[n_units][2H+M+3]: per unit what qmix_mix_td_backward writes per (b, t) row. */
int qmix_mix_td_backward_packed(const float *d_mtd, const float *d_mask, const float *d_q_eval, const int32_t *d_units,
                                int32_t n_units, const int8_t *d_u, int32_t n_agents, int32_t n_actions, int32_t rows_pad,
                                const float *d_p_eval, int32_t hyper_hidden, int32_t qmix_hidden, const qmix_mixer *eval,
                                const float *d_grad_num, float *d_grad_q, float *d_grad_p, float *d_z, float *d_x, void *stream);

/* d_out float32[n_rows][state_len]: row i = float(d_states row d_rows[i]), d_states int8[n_state_rows][state_len] (the
 * ring's (slots, T + 1, S) tensor seen as rows; any base alignment, any state_len >= 1).  A row id outside
 * [0, n_state_rows) is never dereferenced: its output row is NaN. */
int qmix_gather_states(const int8_t *d_states, int64_t n_state_rows, int32_t state_len, const int32_t *d_rows, int32_t n_rows,
                       float *d_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QMIX_PACKED_H */
