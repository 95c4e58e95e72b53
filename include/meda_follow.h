/*
 * meda_follow.h -- C ABI of closed-loop planner routing for MEDA (marl_dmfb_amd.plan.MedaFollower, MedaPlanner.follow and
 * MedaPlanner.plan(safe=True); libmeda_follow.so).  Conventions of the other headers: plain C types, caller-owned DEVICE buffers,
 * `stream` = hipStream_t as void*, asynchronous, negative int error codes before anything is launched.
 *
 * The failure-safe rule is stated in DESIGN.md (section 10) and, executable, in marl_dmfb_amd.plan.plan_reference_meda(safe=True);
 * the closed loop in marl_dmfb_amd.plan.follow_reference_meda.  It is the rule of include/meda_plan.h with two guards, so that a
 * move that fails (a MEDA move succeeds with the mean health of the 25 cells under the droplet) cannot bring two centres closer
 * than d2 < 36: against the planned positions pos_q[t], with N[t] = the union of the discs d2 < 36 around them, t = 0 .. T,
 *     src[t]     = reach[t] & ~G & ~N[t+1]                                  (this droplet stays, the planned one moves)
 *     reach[t+1] = (the nine moves of src[t]) & ~blocked & ~N[t+1] & ~N[t]  (the planned one stays, this droplet moves)
 * and the arrival at level t needs the goal outside N[t] .. N[T].  The kernels must equal the numpy statements bit for bit.
 *
 * One workgroup of one wave per task; lane y owns chip row y as a 64-bit word (bit x); the LDS of include/meda_plan.h and no global
 * scratch.
 */
#ifndef MEDA_FOLLOW_H
#define MEDA_FOLLOW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MEDA_FOLLOW_ERR_BAD_ARG (-1)
#define MEDA_FOLLOW_ERR_UNSUPPORTED (-6)
#define MEDA_FOLLOW_ERR_HIP (-100)

/* The limits of include/meda_plan.h. */
#define MEDA_FOLLOW_MAX_DIM 64
#define MEDA_FOLLOW_MIN_DIM 5
#define MEDA_FOLLOW_MAX_AGENTS 16

/* The safe rule, open loop: the contract, arrays and error codes of meda_plan_route (include/meda_plan.h). */
int meda_follow_plan(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, const int32_t *d_starts,
                     const int32_t *d_goals, const uint8_t *d_avoid, uint8_t *d_route, int8_t *d_u, int32_t *d_steps,
                     uint8_t *d_success, int32_t *d_attempt, int32_t *d_lower_bound, void *stream);

/* Lock-step t of the closed loop: one launch per lock-step between meda_vec_route_append and meda_vec_step.  The contract of
 * route_follow_dmfb (include/route_plan.h) in layout, caller initialisation and error codes; a chip whose d_active byte is 0 is
 * left alone.  What differs:
 *   - the end of an episode is taken from d_terminated, the byte meda_vec_step wrote in the previous lock-step (all droplets done,
 *     the step limit, or a frozen chip): at t > 0 a set byte clears d_active; at t == 0 the byte is not read.  Standing on the goal
 *     centre is not being done: the env sets a droplet's status in the step after it entered the disc d2 < 16;
 *   - a chip off its plan (or with a partial plan) is replanned with the safe rule, with the goals of the k droplets nearest their
 *     goals among those with d2(position, goal) >= 16 (ascending d2, ties by descending index) replaced by their positions, for
 *     k = 0, 1, .. below the count of such droplets; a droplet inside its goal disc is never parked, the env snaps it;
 *   - a missing action is 8 (STALL).
 *   d_goals        int32[B][n][2]       as meda_plan_route; d_avoid uint8[B][width][length] ([y][x]) or NULL
 *   d_positions    uint8[B][T+1][n][2]  the record meda_vec_route_append writes; slot t is read, 2-byte aligned (T = width + length)
 *   d_terminated   uint8[B]             meda_vec_step_out.d_terminated of the previous lock-step
 *   d_route        uint8[B][T+1][n][2]  the kept plan from the centres it was made at, 2-byte aligned;  d_route_u int8[B][T][n]
 *   d_cursor       int32[B]             the level of the kept plan the chip should stand at, -1: no plan yet
 *   d_partial, d_gave_up, d_active      uint8[B]
 *   d_replans, d_steps                  int32[B]   plans made, lock-steps played (+1 whenever actions are emitted)
 *   d_lower_bound  int32[B]             written at t == 0 only: the bound of the first plan
 *   d_actions      int32[B][n]          this lock-step's actions for meda_vec_step; rows of chips left alone are not written
 *   d_u            int8[B][T][n]        row t = the same actions
 * The caller starts an episode with d_cursor -1, d_partial / d_gave_up / d_replans / d_steps 0 and d_u -1.
 * MEDA_FOLLOW_ERR_BAD_ARG for n_tasks < 0, a width or length below MEDA_FOLLOW_MIN_DIM, n_agents <= 0, t outside [0, T), a NULL
 * pointer (d_avoid excepted) or an odd d_positions / d_route; MEDA_FOLLOW_ERR_UNSUPPORTED for a width or length above
 * MEDA_FOLLOW_MAX_DIM or n_agents above MEDA_FOLLOW_MAX_AGENTS; n_tasks == 0 returns 0 and launches nothing. */
int meda_follow_step(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t t, const int32_t *d_goals,
                     const uint8_t *d_avoid, const uint8_t *d_positions, const uint8_t *d_terminated, uint8_t *d_route,
                     int8_t *d_route_u, int32_t *d_cursor, uint8_t *d_partial, int32_t *d_replans, uint8_t *d_gave_up,
                     uint8_t *d_active, int32_t *d_steps, int32_t *d_lower_bound, int32_t *d_actions, int8_t *d_u, void *stream);

/* MEDA_FOLLOW_MAX_DIM of the library that was built. */
int meda_follow_max_dim(void);

/* Dynamic LDS bytes one task takes, (T - 1) * width * 8 + ((T + 1) * n_agents * 2 rounded up to 16), or a negative error code as
 * meda_follow_plan. */
int meda_follow_lds_bytes(int32_t width, int32_t length, int32_t n_agents);

int meda_follow_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif
