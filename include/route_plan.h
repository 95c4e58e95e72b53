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

/* ROUTE_PLAN_MAX_DIM of the library that was built. */
int route_plan_max_dim(void);

/* Dynamic LDS bytes one task takes, or a negative error code as route_plan_dmfb. */
int route_plan_lds_bytes(int32_t width, int32_t length, int32_t n_agents);

int route_plan_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif
