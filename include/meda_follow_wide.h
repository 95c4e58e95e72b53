/*
 * meda_follow_wide.h -- C ABI of closed-loop planner routing for MEDA on chips up to 128 x 128
 * (marl_dmfb_amd.plan.MedaWideFollower, MedaWideFollowPlanner.follow; libmeda_follow_wide.so).  Conventions of the other headers:
 * plain C types, caller-owned DEVICE buffers, `stream` = hipStream_t as void*, asynchronous, negative int error codes before
 * anything is launched.
 *
 * The closed loop is the one of include/meda_follow.h (meda_follow_step; executable: marl_dmfb_amd.plan.follow_reference_meda),
 * every plan made with the failure-safe rule in the geometry of include/meda_plan_wide.h: lane i owns the chip rows i and i + 64,
 * each as two 64-bit words.  The open-loop entry of that rule on these chips is meda_plan_wide_route(safe = 1); there is no second
 * one here.  On chips of 64 x 64 and below the lock-step equals meda_follow_step bit for bit.
 *
 * One workgroup of one wave; a launch has min(n_tasks, MEDA_FOLLOW_WIDE_MAX_GROUPS) workgroups and workgroup b walks the chips
 * b, b + groups, b + 2 * groups, ...  The LDS of a workgroup and the workspace, one slice per workgroup, are those of
 * include/meda_plan_wide.h: the avoid rows, the first H `src` levels and the paths in LDS, the levels H .. T - 3 in the slice.
 */
#ifndef MEDA_FOLLOW_WIDE_H
#define MEDA_FOLLOW_WIDE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MEDA_FOLLOW_WIDE_ERR_BAD_ARG (-1)
#define MEDA_FOLLOW_WIDE_ERR_UNSUPPORTED (-6)
#define MEDA_FOLLOW_WIDE_ERR_HIP (-100)

/* The limits of include/meda_plan_wide.h. */
#define MEDA_FOLLOW_WIDE_MAX_DIM 128
#define MEDA_FOLLOW_WIDE_MIN_DIM 5
#define MEDA_FOLLOW_WIDE_MAX_AGENTS 16
#define MEDA_FOLLOW_WIDE_MAX_GROUPS 512

/* Lock-step t of the closed loop: the contract of meda_follow_step (include/meda_follow.h) in arrays, caller initialisation,
 * d_terminated, the parking rule, STALL (8) as the missing action and error codes, with width and length up to
 * MEDA_FOLLOW_WIDE_MAX_DIM (T = width + length).
 *   d_work, work_bytes  the workspace: at least meda_follow_wide_work_bytes(n_tasks, width, length, n_agents, lds_levels) bytes,
 *                       16-byte aligned; d_work may be NULL when that is 0.  Its content before and after a call means nothing,
 *                       so one workspace serves every lock-step of an episode.
 *   lds_levels          > 0: at most that many levels stay in LDS (the rest go to the workspace); <= 0: as many as fit.  The
 *                       episodes do not depend on it.
 * MEDA_FOLLOW_WIDE_ERR_BAD_ARG for n_tasks < 0, a width or length below MEDA_FOLLOW_WIDE_MIN_DIM, n_agents <= 0, t outside
 * [0, T), a NULL pointer (d_avoid excepted), an odd d_positions / d_route, a workspace that is needed and missing, too small or
 * misaligned; MEDA_FOLLOW_WIDE_ERR_UNSUPPORTED for a width or length above MEDA_FOLLOW_WIDE_MAX_DIM or n_agents above
 * MEDA_FOLLOW_WIDE_MAX_AGENTS; n_tasks == 0 returns 0 and launches nothing. */
int meda_follow_wide_step(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t t, const int32_t *d_goals,
                          const uint8_t *d_avoid, const uint8_t *d_positions, const uint8_t *d_terminated, uint8_t *d_route,
                          int8_t *d_route_u, int32_t *d_cursor, uint8_t *d_partial, int32_t *d_replans, uint8_t *d_gave_up,
                          uint8_t *d_active, int32_t *d_steps, int32_t *d_lower_bound, int32_t *d_actions, int8_t *d_u,
                          void *d_work, int64_t work_bytes, int32_t lds_levels, void *stream);

/* MEDA_FOLLOW_WIDE_MAX_DIM and MEDA_FOLLOW_WIDE_MAX_GROUPS of the library that was built. */
int meda_follow_wide_max_dim(void);
int meda_follow_wide_max_groups(void);

/* H, the levels a workgroup keeps in LDS when lds_levels <= 0:
 * min(T - 2, (160 KiB - 1 KiB - paths - width * 16) / (width * 16)); or a negative error code as meda_follow_wide_step. */
int meda_follow_wide_lds_levels(int32_t width, int32_t length, int32_t n_agents);

/* Dynamic LDS bytes of one workgroup: (1 + min(H, lds_levels if > 0)) * width * 16 + paths, the paths being
 * (T + 1) * n_agents * 2 bytes rounded up to 16; or a negative error code. */
int meda_follow_wide_lds_bytes(int32_t width, int32_t length, int32_t n_agents, int32_t lds_levels);

/* The workspace a launch needs: min(n_tasks, MEDA_FOLLOW_WIDE_MAX_GROUPS) * (T - 2 - levels in LDS) * width * 16 bytes; or a
 * negative error code. */
int64_t meda_follow_wide_work_bytes(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t lds_levels);

int meda_follow_wide_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif
