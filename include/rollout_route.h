/*
 * rollout_route.h -- C ABI of the best-of-K route pick of marl_dmfb_amd.route.Router (built into the rollout_ops library,
 * conventions of rollout_ops.h: plain C types, caller-owned DEVICE buffers, `stream` = hipStream_t as void*, asynchronous,
 * negative int error codes ROLLOUT_ERR_*).
 *
 * Every task is played K times side by side in one lock-step batch, task-major: chip = task * K + try.  The recorded episodes
 * are those of an Evaluator in route mode: d_route uint8[B*K][T+1][n][2] (dmfb_vec_route_append / meda_vec_route_append) and
 * d_u int8[B*K][T][n] (the actions, slot t written by rollout_select_actions / rollout_gru_head_select).
 */
#ifndef ROLLOUT_ROUTE_H
#define ROLLOUT_ROUTE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* For every task b, the winning try k* among its K tries, by this exact, deterministic order:
 *   a successful try (d_success[chip] > 0) beats a failed one;
 *   then fewer steps wins (d_steps: the raw played steps, before failed episodes are set to episode_limit);
 *   then fewer constraints wins (d_constraints int32[B*K] when constraints_f64 == 0, float64[B*K] when == 1);
 *   then the lower try index wins.
 * d_choice[b] = k*; the rows of chip b * K + k* are copied to d_route_out uint8[B][T+1][n][2] and d_u_out int8[B][T][n]
 * (each pair may be NULL together).  One wave per task: the pick is a wave reduction, then the wave copies the rows.
 * ROLLOUT_ERR_BAD_ARG, before anything is launched, for n_tasks < 0, tries < 1, n_agents < 1, T < 1, a NULL d_steps /
 * d_success / d_constraints / d_choice, or only one pointer of a pair. */
int rollout_route_select(int32_t n_tasks, int32_t tries, int32_t n_agents, int32_t T, const int64_t *d_steps,
                         const int64_t *d_success, const void *d_constraints, int32_t constraints_f64, const uint8_t *d_route,
                         const int8_t *d_u, uint8_t *d_route_out, int8_t *d_u_out, int32_t *d_choice, void *stream);

#ifdef __cplusplus
}
#endif
#endif
