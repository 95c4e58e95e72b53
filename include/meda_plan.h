/*
 * meda_plan.h -- C ABI of the deterministic space-time planner for MEDA (marl_dmfb_amd.plan.MedaPlanner; libmeda_plan.so).
 * Conventions of the other headers: plain C types, caller-owned DEVICE buffers, `stream` = hipStream_t as void*, asynchronous,
 * negative int error codes before anything is launched.
 *
 * The rule is stated in DESIGN.md ("Space-time planner", MEDA) and, executable, in marl_dmfb_amd.plan.plan_reference_meda:
 * prioritized planning (droplets by descending squared distance start -> goal, ties by index; attempt k plans them in that order
 * rotated left by k), each droplet by a breadth-first search over (centre, time) with the nine moves of include/meda_vec.h and
 * their clamps, against the discs d2 < 36 around the droplets planned before it, up to the first level that touches the disc
 * d2 < 16 around its goal, walked back with the lowest action number and then the lowest (y, x) source at every level.  The kernel
 * must equal plan_reference_meda bit for bit.
 *
 * One workgroup of one wave per task; lane y owns chip row y as a 64-bit word (bit x).  Everything of a task lives in LDS:
 *   the avoided cells widened in x (the rows `blocked` is made of)      width * 8 bytes
 *   the `src` levels of the droplet in flight                          (T - 2) * width * 8 bytes   (T = width + length)
 *   the planned paths                                                  (T + 1) * n_agents * 2 bytes, rounded up to 16
 * so the walk back needs no parent table and there is no global scratch.  At the limit (64 x 64, 16 droplets) that is
 * 65,024 + 4,128 = 69,152 bytes of the 163,840 a workgroup may hold on gfx950; 30 x 30 with 4 droplets takes 14,160 + 496.
 */
#ifndef MEDA_PLAN_H
#define MEDA_PLAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MEDA_PLAN_ERR_BAD_ARG (-1)
#define MEDA_PLAN_ERR_UNSUPPORTED (-6)
#define MEDA_PLAN_ERR_HIP (-100)

/* The largest width and the largest length: one lane per row, one bit per column of a 64-bit row word. */
#define MEDA_PLAN_MAX_DIM 64
/* The smallest: a 5x5 droplet has to fit. */
#define MEDA_PLAN_MIN_DIM 5
#define MEDA_PLAN_MAX_AGENTS 16

/* Plans n_tasks independent tasks on a chip of `width` rows (y) and `length` columns (x); centres (x, y) with
 * 2 <= x <= length-3 and 2 <= y <= width-3, as meda_vec_set_task takes them.
 *   d_starts, d_goals  int32[B][n][2]   (x, y) per droplet; in range, starts distinct, goals distinct (the caller checks)
 *   d_avoid            uint8[B][width][length] ([y][x]), non-zero = a cell no droplet's 5x5 box may touch after a move, or NULL
 *   d_route            uint8[B][T+1][n][2]  centres after t steps, the goal from the snap step on; all equal to the starts on failure
 *   d_u                int8[B][T][n]    the planned action (0 N 1 E 2 S 3 W 4 NE 5 SE 6 SW 7 NW 8 STALL) for t < steps, 8 for a
 *                                       droplet inside its goal disc or done, -1 from steps on
 *   d_steps            int32[B]         the largest (arrival + 1): the step at which the env reports success; 0 on failure
 *   d_success          uint8[B]
 *   d_attempt          int32[B]         the rotation that was kept, -1 on failure
 *   d_lower_bound      int32[B]         the largest (arrival + 1) of the droplets planned alone; -1 if some goal cannot be reached
 * MEDA_PLAN_ERR_BAD_ARG for n_tasks < 0, a width or length below MEDA_PLAN_MIN_DIM, n_agents <= 0, a NULL required pointer;
 * MEDA_PLAN_ERR_UNSUPPORTED for a width or length above MEDA_PLAN_MAX_DIM or n_agents above MEDA_PLAN_MAX_AGENTS;
 * n_tasks == 0 returns 0 and launches nothing. */
int meda_plan_route(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, const int32_t *d_starts,
                    const int32_t *d_goals, const uint8_t *d_avoid, uint8_t *d_route, int8_t *d_u, int32_t *d_steps,
                    uint8_t *d_success, int32_t *d_attempt, int32_t *d_lower_bound, void *stream);

/* MEDA_PLAN_MAX_DIM of the library that was built. */
int meda_plan_max_dim(void);

/* Dynamic LDS bytes one task takes, (T - 1) * width * 8 + ((T + 1) * n_agents * 2 rounded up to 16), or a negative error code as
 * meda_plan_route. */
int meda_plan_lds_bytes(int32_t width, int32_t length, int32_t n_agents);

int meda_plan_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif
