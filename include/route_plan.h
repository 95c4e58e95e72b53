/*
 * route_plan.h -- C ABI of the deterministic space-time planner for DMFB (marl_dmfb_amd.plan.Planner; libroute_plan.so).
 * Conventions of the other headers: plain C types, caller-owned DEVICE buffers, `stream` = hipStream_t as void*, asynchronous,
 * negative int error codes before anything is launched.
 *
 * The rule is stated in DESIGN.md ("Space-time planner") and, executable, in marl_dmfb_amd.plan.plan_reference: prioritized
 * planning (droplets by descending Manhattan distance, ties by index; attempt k plans them in that order rotated left by k), each
 * droplet by a breadth-first search over (cell, time) against the 3x3 neighbourhoods of the droplets planned before it, walked
 * back with the lowest action number at every level.  The kernel must equal plan_reference bit for bit.
 *
 * One workgroup of one wave per task; lane x owns chip row x as a 64-bit word (bit y).  Everything of a task lives in LDS:
 *   the filtered reach levels of the droplet in flight   (T - 1) * width * 8 bytes   (T = 2 * (width + length))
 *   the planned paths                                    (T + 1) * n_agents * 2 bytes
 * so the walk back needs no parent table and there is no global scratch.  At the limit (64 x 64, 16 droplets) that is
 * 130,560 + 8,224 bytes of the 163,840 a workgroup may hold on gfx950; 50 x 50 with 10 droplets takes 83,620.
 */
#ifndef ROUTE_PLAN_H
#define ROUTE_PLAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ROUTE_PLAN_ERR_BAD_ARG (-1)
#define ROUTE_PLAN_ERR_UNSUPPORTED (-6)
#define ROUTE_PLAN_ERR_HIP (-100)

/* The largest width and the largest length: one lane per row, one bit per column of a 64-bit row word. */
#define ROUTE_PLAN_MAX_DIM 64
#define ROUTE_PLAN_MAX_AGENTS 16
/* The largest `reserve` and `retries` of the _opt entry points. */
#define ROUTE_PLAN_MAX_RESERVE 255
#define ROUTE_PLAN_MAX_RETRIES 255

/* Plans n_tasks independent tasks on a width x length chip (cells (x, y), x < width, y < length).
 *   d_starts, d_goals  int32[B][n][2]   (x, y) per droplet; on the chip, starts distinct, goals distinct (the caller checks)
 *   d_blocks           int32[B][nb][4]  x0, x1, y0, y1 inclusive, or NULL when n_blocks == 0
 *   d_avoid            uint8[B][width][length], non-zero = a cell no droplet may enter, or NULL
 *   d_route            uint8[B][T+1][n][2]  positions after t steps, the last one repeated; all equal to the starts on failure
 *   d_u                int8[B][T][n]    the planned action (0 STALL 1 RIGHT 2 LEFT 3 DOWN 4 UP) for t < steps, -1 from steps on
 *   d_steps            int32[B]         the largest arrival time, 0 on failure
 *   d_success          uint8[B]
 *   d_attempt          int32[B]         the rotation that was kept, -1 on failure
 *   d_lower_bound      int32[B]         the largest arrival of the droplets planned alone; -1 if some goal cannot be reached
 * ROUTE_PLAN_ERR_BAD_ARG for n_tasks < 0, a non-positive width / length / n_agents, n_agents > ROUTE_PLAN_MAX_AGENTS,
 * n_blocks < 0, a NULL required pointer, n_blocks > 0 with d_blocks NULL; ROUTE_PLAN_ERR_UNSUPPORTED for a width or length above
 * ROUTE_PLAN_MAX_DIM; n_tasks == 0 returns 0 and launches nothing. */
int route_plan_dmfb(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t n_blocks,
                    const int32_t *d_starts, const int32_t *d_goals, const int32_t *d_blocks, const uint8_t *d_avoid,
                    uint8_t *d_route, int8_t *d_u, int32_t *d_steps, uint8_t *d_success, int32_t *d_attempt,
                    int32_t *d_lower_bound, void *stream);

/* route_plan_dmfb with the two opt-in parameters of the rule (plan_reference(reserve=, retries=)); 0 / 0 is
 * route_plan_dmfb bit for bit.
 *   reserve  R: while a droplet is searched, every droplet not yet planned in the attempt forbids near(its start) at the levels
 *            1 .. min(R, T), so that no earlier droplet's first steps corner it; what later droplets see are true paths only.
 *   retries  Q: when all n rotations fail, up to Q further attempts.  Attempt n plans the base order with the first droplet that
 *            got no path in attempt 0 moved to the front; attempt n + r + 1 plans the order of attempt n + r with the first droplet
 *            that got no path in it moved to the front, and the retries end when that droplet is at the front already.
 *   d_attempt   the attempt that was kept: a rotation 0 .. n-1 or a retry n .. n+Q-1, -1 on failure
 * d_lower_bound is the bound of the droplets alone, without reservations.  ROUTE_PLAN_ERR_BAD_ARG also for a reserve outside
 * 0 .. ROUTE_PLAN_MAX_RESERVE or retries outside 0 .. ROUTE_PLAN_MAX_RETRIES. */
int route_plan_dmfb_opt(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t n_blocks,
                        const int32_t *d_starts, const int32_t *d_goals, const int32_t *d_blocks, const uint8_t *d_avoid,
                        uint8_t *d_route, int8_t *d_u, int32_t *d_steps, uint8_t *d_success, int32_t *d_attempt,
                        int32_t *d_lower_bound, int32_t reserve, int32_t retries, void *stream);

/* Lock-step t of closed-loop routing (marl_dmfb_amd.plan.Follower; the rule: plan.follow_reference and DESIGN.md, "Closed-loop
 * routing"): one launch per lock-step between dmfb_vec_route_append and dmfb_vec_step, one workgroup of one wave per chip, the
 * LDS of route_plan_dmfb and no global scratch.  A chip whose d_active byte is 0 is left alone.  A chip whose droplets are all on
 * their goals at t > 0 has ended: its d_active byte is cleared.  A chip that has a complete plan (d_cursor >= 0, d_partial 0) and
 * stands where that plan says at d_cursor plays the plan's next actions and advances the cursor.  Any other chip is replanned
 * from where it stands, with the goals of the k droplets nearest their goals (ascending Manhattan distance > 0, ties by
 * descending index) replaced by their positions, for k = 0, 1, .. below the count of droplets off their goals, until the rule of
 * route_plan_dmfb routes it: the plan, d_cursor = 1, d_partial = (k > 0) and d_replans + 1 are written and the plan's first
 * actions played.  If no k does, d_gave_up is set and d_active cleared.
 *   d_goals        int32[B][n][2]       as route_plan_dmfb; d_blocks, d_avoid likewise
 *   d_positions    uint8[B][T+1][n][2]  the record dmfb_vec_route_append writes; slot t is read, 2-byte aligned
 *   d_route        uint8[B][T+1][n][2]  the kept plan from the positions it was made at, 2-byte aligned;  d_route_u int8[B][T][n]
 *   d_cursor       int32[B]             the level of the kept plan the chip should stand at, -1: no plan yet
 *   d_partial, d_gave_up, d_active      uint8[B]
 *   d_replans, d_steps                  int32[B]   plans made, lock-steps played (+1 whenever actions are emitted)
 *   d_lower_bound  int32[B]             written at t == 0 only: the bound of the first plan
 *   d_actions      int32[B][n]          this lock-step's actions for dmfb_vec_step; rows of chips left alone are not written
 *   d_u            int8[B][T][n]        row t = the same actions
 * The caller starts an episode with d_cursor -1, d_partial / d_gave_up / d_replans / d_steps 0 and d_u -1.
 * ROUTE_PLAN_ERR_BAD_ARG as route_plan_dmfb and for t outside [0, T), a NULL pointer (d_blocks with n_blocks == 0 and d_avoid
 * excepted) or an odd d_positions / d_route; ROUTE_PLAN_ERR_UNSUPPORTED as route_plan_dmfb; n_tasks == 0 launches nothing. */
int route_follow_dmfb(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t n_blocks, int32_t t,
                      const int32_t *d_goals, const int32_t *d_blocks, const uint8_t *d_avoid, const uint8_t *d_positions,
                      uint8_t *d_route, int8_t *d_route_u, int32_t *d_cursor, uint8_t *d_partial, int32_t *d_replans,
                      uint8_t *d_gave_up, uint8_t *d_active, int32_t *d_steps, int32_t *d_lower_bound, int32_t *d_actions, int8_t *d_u,
                      void *stream);

/* route_follow_dmfb with every replan made by the rule of route_plan_dmfb_opt: a droplet's start is where it stands at the replan,
 * a parked droplet's goal is its position.  0 / 0 is route_follow_dmfb bit for bit; the same reserve / retries are expected at
 * every lock-step of an episode.  ROUTE_PLAN_ERR_BAD_ARG also as route_plan_dmfb_opt. */
int route_follow_dmfb_opt(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t n_blocks, int32_t t,
                          const int32_t *d_goals, const int32_t *d_blocks, const uint8_t *d_avoid, const uint8_t *d_positions,
                          uint8_t *d_route, int8_t *d_route_u, int32_t *d_cursor, uint8_t *d_partial, int32_t *d_replans,
                          uint8_t *d_gave_up, uint8_t *d_active, int32_t *d_steps, int32_t *d_lower_bound, int32_t *d_actions,
                          int8_t *d_u, int32_t reserve, int32_t retries, void *stream);

/* ROUTE_PLAN_MAX_DIM of the library that was built. */
int route_plan_max_dim(void);

/* Dynamic LDS bytes one task takes, or a negative error code as route_plan_dmfb. */
int route_plan_lds_bytes(int32_t width, int32_t length, int32_t n_agents);

int route_plan_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif
