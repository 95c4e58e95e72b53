// meda_follow.hip -- closed-loop planner routing for MEDA of include/meda_follow.h (libmeda_follow.so): the failure-safe rule of the
// geometry in meda_geo.h as an open-loop planner (meda_follow_plan) and around it the lock-step kernel of the closed loop
// (meda_follow_step: follow_chip of plan_core.h).  One workgroup of ONE wave per chip, the planner's LDS, no global scratch.
#include "../../include/meda_follow.h"

#define HIP_ABI_TAG "meda_follow"
#define HIP_ABI_ERR MEDA_FOLLOW_ERR_HIP
#include "hip_abi.h"
#include "plan_core.h"
#include "meda_geo.h"

namespace {

struct FollowAbi {
    static constexpr int kMinDim = MEDA_FOLLOW_MIN_DIM, kMaxDim = MEDA_FOLLOW_MAX_DIM, kMaxAgents = MEDA_FOLLOW_MAX_AGENTS;
    static constexpr int kBadArg = MEDA_FOLLOW_ERR_BAD_ARG, kUnsupported = MEDA_FOLLOW_ERR_UNSUPPORTED;
};
typedef Meda<true, FollowAbi> Safe;

// Lock-step t of the closed loop, one chip per workgroup: a frozen chip returns at once, a chip whose episode the env ended is
// frozen, a chip that is where its kept plan says costs one compare, any other is replanned from where it is with the safe rule.
__global__ __launch_bounds__(kWave) void k_meda_follow_step(int W, int L, int n, int t, const int32_t *__restrict__ goals,
                                                            const uint8_t *__restrict__ avoid, const uint8_t *__restrict__ positions,
                                                            const uint8_t *__restrict__ terminated, FollowState st) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int T = Safe::limit(W, L);
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    if (!st.active[b]) return;
    if (t > 0 && terminated[b]) {   // the last step ended the episode: every droplet done, or the step limit
        if (lane == 0) st.active[b] = 0;
        return;
    }
    const int pos = lane < n ? ((const unsigned short *)positions)[(b * (T + 1) + t) * n + lane] : 0;
    int gx = 0, gy = 0;
    if (lane < n) { gx = goals[(b * n + lane) * 2]; gy = goals[(b * n + lane) * 2 + 1]; }
    u64 *wide = (u64 *)smem;
    follow_chip<Safe>(b, W, L, T, n, t, pos, gx, gy, st, wide + W, (unsigned short *)(smem + (size_t)(T - 1) * W * 8), 0, 0,
                      [&] { return meda_blocked_row(wide, avoid, b, W, L, lane); });
}

}  // namespace

extern "C" {

int meda_follow_max_dim(void) { return MEDA_FOLLOW_MAX_DIM; }

int meda_follow_lds_bytes(int32_t width, int32_t length, int32_t n_agents) {
    if (const int rc = Safe::check_sizes(width, length, n_agents)) return rc;
    return (int)lds_bytes(Safe::limit(width, length), width, n_agents);
}

int meda_follow_plan(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, const int32_t *d_starts,
                     const int32_t *d_goals, const uint8_t *d_avoid, uint8_t *d_route, int8_t *d_u, int32_t *d_steps,
                     uint8_t *d_success, int32_t *d_attempt, int32_t *d_lower_bound, void *stream) {
    const PlanIO io = {d_starts, d_goals, d_route, d_u, d_steps, d_success, d_attempt, d_lower_bound};
    return launch_plan<Safe>(k_meda_plan<Safe>, n_tasks, width, length, n_agents, io, true, stream, d_avoid);
}

int meda_follow_step(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t t, const int32_t *d_goals,
                     const uint8_t *d_avoid, const uint8_t *d_positions, const uint8_t *d_terminated, uint8_t *d_route,
                     int8_t *d_route_u, int32_t *d_cursor, uint8_t *d_partial, int32_t *d_replans, uint8_t *d_gave_up,
                     uint8_t *d_active, int32_t *d_steps, int32_t *d_lower_bound, int32_t *d_actions, int8_t *d_u, void *stream) {
    const FollowState st = {d_route, d_route_u, d_cursor, d_partial, d_replans, d_gave_up, d_active, d_steps, d_lower_bound, d_actions,
                            d_u};
    return launch_follow<Safe>(k_meda_follow_step, n_tasks, width, length, n_agents, t, d_goals, d_positions, st, d_terminated != nullptr,
                               stream, d_avoid, d_positions, d_terminated, st);
}

int meda_follow_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
