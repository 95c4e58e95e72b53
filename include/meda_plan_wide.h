/*
 * meda_plan_wide.h -- C ABI of the wide space-time planner for MEDA: chips up to 128 x 128
 * (marl_dmfb_amd.plan.MedaWidePlanner; libmeda_plan_wide.so).  Conventions of the other headers: plain C types, caller-owned
 * DEVICE buffers, `stream` = hipStream_t as void*, asynchronous, negative int error codes before anything is launched.
 *
 * The rule is the one of include/meda_plan.h (safe == 0: meda_plan_route) and include/meda_follow.h (safe != 0: meda_follow_plan),
 * stated in DESIGN.md ("Space-time planner", MEDA) and, executable, in marl_dmfb_amd.plan.plan_reference_meda(..., safe=...).  The
 * six result arrays and their meaning are those of meda_plan_route, and the kernel must equal plan_reference_meda bit for bit;
 * on chips of 64 x 64 and below it therefore equals the narrow planner too.
 *
 * One workgroup of one wave per task; lane i owns the chip rows i and i + 64, each as two 64-bit words (bit x of word x / 64).
 * A `src` level is now width * 16 bytes, and the T - 2 levels (T = width + length) of a large chip no longer fit the LDS of a
 * workgroup.  A task keeps in LDS
 *   the avoided cells widened in x (the rows `blocked` is made of)      width * 16 bytes
 *   the first H `src` levels of the droplet in flight                   H * width * 16 bytes
 *   the planned paths                                                   (T + 1) * n_agents * 2 bytes, rounded up to 16
 * with H = min(T - 2, what 160 KiB - 1 KiB holds beside the other two), and the levels H .. T - 3 in the caller's workspace.
 * The workspace is cut into one slice of (T - 2 - H) * width * 16 bytes per workgroup, so the grid is bounded: a launch has
 * min(n_tasks, MEDA_PLAN_WIDE_MAX_GROUPS) workgroups and workgroup b plans the tasks b, b + groups, b + 2 * groups, ...
 */
#ifndef MEDA_PLAN_WIDE_H
#define MEDA_PLAN_WIDE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MEDA_PLAN_WIDE_ERR_BAD_ARG (-1)
#define MEDA_PLAN_WIDE_ERR_UNSUPPORTED (-6)
#define MEDA_PLAN_WIDE_ERR_HIP (-100)

/* The largest width and the largest length: two rows per lane, two 64-bit words per row. */
#define MEDA_PLAN_WIDE_MAX_DIM 128
/* The smallest: a 5x5 droplet has to fit. */
#define MEDA_PLAN_WIDE_MIN_DIM 5
#define MEDA_PLAN_WIDE_MAX_AGENTS 16
/* The workgroups of one launch; each walks the tasks b, b + groups, ...  Two per compute unit of an MI355X. */
#define MEDA_PLAN_WIDE_MAX_GROUPS 512

/* Plans n_tasks independent tasks on a chip of `width` rows (y) and `length` columns (x), with the plain rule (safe == 0) or the
 * failure-safe rule (safe != 0).  d_starts, d_goals, d_avoid and the six result arrays are those of meda_plan_route
 * (include/meda_plan.h), T = width + length.
 *   d_work, work_bytes  the workspace: at least meda_plan_wide_work_bytes(n_tasks, width, length, n_agents, lds_levels) bytes,
 *                       16-byte aligned; d_work may be NULL when that is 0.  Its content before and after a call means nothing.
 *   lds_levels          > 0: at most that many levels stay in LDS (the rest go to the workspace); <= 0: as many as fit.  The
 *                       planned routes do not depend on it.
 * MEDA_PLAN_WIDE_ERR_BAD_ARG for n_tasks < 0, a width or length below MEDA_PLAN_WIDE_MIN_DIM, n_agents <= 0, a NULL required
 * pointer, a workspace that is too small or misaligned; MEDA_PLAN_WIDE_ERR_UNSUPPORTED for a width or length above
 * MEDA_PLAN_WIDE_MAX_DIM or n_agents above MEDA_PLAN_WIDE_MAX_AGENTS; n_tasks == 0 returns 0 and launches nothing. */
int meda_plan_wide_route(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t safe,
                         const int32_t *d_starts, const int32_t *d_goals, const uint8_t *d_avoid,
                         uint8_t *d_route, int8_t *d_u, int32_t *d_steps, uint8_t *d_success,
                         int32_t *d_attempt, int32_t *d_lower_bound,
                         void *d_work, int64_t work_bytes, int32_t lds_levels, void *stream);

/* MEDA_PLAN_WIDE_MAX_DIM and MEDA_PLAN_WIDE_MAX_GROUPS of the library that was built. */
int meda_plan_wide_max_dim(void);
int meda_plan_wide_max_groups(void);

/* H, the levels a task keeps in LDS when lds_levels <= 0:
 * min(T - 2, (160 KiB - 1 KiB - paths - width * 16) / (width * 16)); or a negative error code as meda_plan_wide_route. */
int meda_plan_wide_lds_levels(int32_t width, int32_t length, int32_t n_agents);

/* Dynamic LDS bytes of one task: (1 + min(H, lds_levels if > 0)) * width * 16 + paths; or a negative error code. */
int meda_plan_wide_lds_bytes(int32_t width, int32_t length, int32_t n_agents, int32_t lds_levels);

/* The workspace a launch needs: min(n_tasks, MEDA_PLAN_WIDE_MAX_GROUPS) * (T - 2 - levels in LDS) * width * 16 bytes; or a
 * negative error code. */
int64_t meda_plan_wide_work_bytes(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t lds_levels);

int meda_plan_wide_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif
