// meda_follow_wide.hip -- closed-loop planner routing for MEDA chips up to 128 x 128 of include/meda_follow_wide.h
// (libmeda_follow_wide.so): the lock-step of meda_follow.hip (follow_chip of plan_core.h) with the failure-safe rule of the geometry
// in meda_geo_wide.h.  One workgroup of ONE wave, a bounded grid whose workgroups walk the chips, the first H levels of a plan in
// LDS and the rest in the caller's workspace, as meda_plan_wide.hip.
#include "../../include/meda_follow_wide.h"

#define HIP_ABI_TAG "meda_follow_wide"
#define HIP_ABI_ERR MEDA_FOLLOW_WIDE_ERR_HIP
#include "hip_abi.h"
#include "plan_core.h"
#include "meda_geo.h"
#include "meda_geo_wide.h"

namespace {

struct FollowWideAbi {
    static constexpr int kMinDim = MEDA_FOLLOW_WIDE_MIN_DIM, kMaxDim = MEDA_FOLLOW_WIDE_MAX_DIM, kMaxAgents = MEDA_FOLLOW_WIDE_MAX_AGENTS;
    static constexpr int kBadArg = MEDA_FOLLOW_WIDE_ERR_BAD_ARG, kUnsupported = MEDA_FOLLOW_WIDE_ERR_UNSUPPORTED;
};
typedef MedaWide<true, FollowWideAbi> Safe;
static_assert(MEDA_FOLLOW_WIDE_MAX_GROUPS == kWideMaxGroups, "the sizing helpers of meda_geo_wide.h count these groups");

// Lock-step t of the closed loop.  Workgroup g takes the chips g, g + groups, ...: an inactive chip is left alone, a chip whose
// episode the env ended is frozen, a chip that is where its kept plan says costs one compare, any other is replanned from where
// it is with the safe rule.  The dynamic LDS: the widened avoid rows [W], the levels [H][W], the paths.  `work`: the slices of
// (T - 2 - H) * W rows, one per workgroup.
__global__ __launch_bounds__(kWave) void k_meda_follow_wide_step(int n_tasks, int W, int L, int n, int t, const int32_t *__restrict__ goals,
                                                                 const uint8_t *__restrict__ avoid, const uint8_t *__restrict__ positions,
                                                                 const uint8_t *__restrict__ terminated, FollowState st, int H,
                                                                 Row128 *work) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int T = Safe::limit(W, L);
    const int lane = threadIdx.x;
    Row128 *wide = (Row128 *)smem;
    const WideLevels levels = {wide + W, work + (size_t)blockIdx.x * (T - 2 - H) * W, H};
    unsigned short *path = (unsigned short *)(smem + (size_t)(H + 1) * W * sizeof(Row128));
    for (size_t b = blockIdx.x; b < (size_t)n_tasks; b += gridDim.x) {
        if (st.active[b]) {
            if (t > 0 && terminated[b]) {   // the last step ended the episode: every droplet done, or the step limit
                if (lane == 0) st.active[b] = 0;
            } else {
                const int pos = lane < n ? ((const unsigned short *)positions)[(b * (T + 1) + t) * n + lane] : 0;
                int gx = 0, gy = 0;
                if (lane < n) { gx = goals[(b * n + lane) * 2]; gy = goals[(b * n + lane) * 2 + 1]; }
                follow_chip<Safe>(b, W, L, T, n, t, pos, gx, gy, st, levels, path, 0, 0,
                                  [&] { return meda_blocked_rows(wide, avoid, b, W, L, lane); });
            }
        }
        __syncthreads();   // the task arrays, the avoid rows and the paths are free for the next chip
    }
}

}  // namespace

extern "C" {

int meda_follow_wide_max_dim(void) { return MEDA_FOLLOW_WIDE_MAX_DIM; }

int meda_follow_wide_max_groups(void) { return MEDA_FOLLOW_WIDE_MAX_GROUPS; }

int meda_follow_wide_lds_levels(int32_t width, int32_t length, int32_t n_agents) {
    if (const int rc = Safe::check_sizes(width, length, n_agents)) return rc;
    return levels_in_lds(width, length, n_agents, 0);
}

int meda_follow_wide_lds_bytes(int32_t width, int32_t length, int32_t n_agents, int32_t lds_levels) {
    if (const int rc = Safe::check_sizes(width, length, n_agents)) return rc;
    return (int)lds_bytes_wide(width, length, n_agents, levels_in_lds(width, length, n_agents, lds_levels));
}

int64_t meda_follow_wide_work_bytes(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t lds_levels) {
    if (n_tasks < 0) return MEDA_FOLLOW_WIDE_ERR_BAD_ARG;
    if (const int rc = Safe::check_sizes(width, length, n_agents)) return rc;
    return (int64_t)groups_of(n_tasks) * (int64_t)slice_bytes(width, length, levels_in_lds(width, length, n_agents, lds_levels));
}

int meda_follow_wide_step(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t t, const int32_t *d_goals,
                          const uint8_t *d_avoid, const uint8_t *d_positions, const uint8_t *d_terminated, uint8_t *d_route,
                          int8_t *d_route_u, int32_t *d_cursor, uint8_t *d_partial, int32_t *d_replans, uint8_t *d_gave_up,
                          uint8_t *d_active, int32_t *d_steps, int32_t *d_lower_bound, int32_t *d_actions, int8_t *d_u, void *d_work,
                          int64_t work_bytes, int32_t lds_levels, void *stream) {
    const FollowState st = {d_route, d_route_u, d_cursor, d_partial, d_replans, d_gave_up, d_active, d_steps, d_lower_bound, d_actions,
                            d_u};
    if (const int rc = check_follow<Safe>(n_tasks, width, length, n_agents, t, d_goals, d_positions, st, d_terminated != nullptr))
        return rc;
    const int H = levels_in_lds(width, length, n_agents, lds_levels);
    const int64_t need = (int64_t)groups_of(n_tasks) * (int64_t)slice_bytes(width, length, H);
    if (need > 0 && (!d_work || work_bytes < need || ((uintptr_t)d_work & (sizeof(Row128) - 1)))) return MEDA_FOLLOW_WIDE_ERR_BAD_ARG;
    if (n_tasks == 0) return 0;
    const size_t lds = lds_bytes_wide(width, length, n_agents, H);
    static LdsLimit lds_limit;   // one per kernel
    if (lds > 64 * 1024)
        if (const int rc = lds_limit.raise((const void *)k_meda_follow_wide_step, kLdsBudget)) return rc;
    LAUNCH(k_meda_follow_wide_step, dim3((unsigned)groups_of(n_tasks)), dim3(kWave), lds, (hipStream_t)stream, n_tasks, width, length,
           n_agents, t, d_goals, d_avoid, d_positions, d_terminated, st, H, (Row128 *)d_work);
    return 0;
}

int meda_follow_wide_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
