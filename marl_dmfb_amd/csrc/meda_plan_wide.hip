// meda_plan_wide.hip -- the space-time planner for MEDA chips up to 128 x 128 of include/meda_plan_wide.h (libmeda_plan_wide.so): the
// plain and the failure-safe rule of the geometry in meda_geo_wide.h, one workgroup of ONE wave per task, a bounded grid whose
// workgroups walk the tasks, the first H levels in LDS and the rest in the caller's workspace.
#include "../../include/meda_plan_wide.h"

#define HIP_ABI_TAG "meda_plan_wide"
#define HIP_ABI_ERR MEDA_PLAN_WIDE_ERR_HIP
#include "hip_abi.h"
#include "plan_core.h"
#include "meda_geo.h"
#include "meda_geo_wide.h"

namespace {

struct WideAbi {
    static constexpr int kMinDim = MEDA_PLAN_WIDE_MIN_DIM, kMaxDim = MEDA_PLAN_WIDE_MAX_DIM, kMaxAgents = MEDA_PLAN_WIDE_MAX_AGENTS;
    static constexpr int kBadArg = MEDA_PLAN_WIDE_ERR_BAD_ARG, kUnsupported = MEDA_PLAN_WIDE_ERR_UNSUPPORTED;
};
typedef MedaWide<false, WideAbi> Plain;
typedef MedaWide<true, WideAbi> Safe;

// Workgroup g plans the tasks g, g + groups, ...  The dynamic LDS: the widened avoid rows [W], the levels [H][W], the paths.
// `work`: the slices of (T - 2 - H) * W rows, one per workgroup.
template <class Geo>
__global__ __launch_bounds__(kWave) void k_meda_plan_wide(int n_tasks, int W, int L, int n, PlanIO io, const uint8_t *__restrict__ avoid,
                                                          int H, Row128 *work) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int T = Geo::limit(W, L);
    Row128 *wide = (Row128 *)smem;
    const WideLevels levels = {wide + W, work + (size_t)blockIdx.x * (T - 2 - H) * W, H};
    unsigned short *path = (unsigned short *)(smem + (size_t)(H + 1) * W * sizeof(Row128));
    for (size_t b = blockIdx.x; b < (size_t)n_tasks; b += gridDim.x) {
        const Rows blocked = meda_blocked_rows(wide, avoid, b, W, L, threadIdx.x);
        plan_task<Geo>(b, W, L, T, n, blocked, levels, path, io, 0, 0);   // no reservations, no retries
        __syncthreads();   // the task arrays, the avoid rows and the paths are free for the next task
    }
}

// ---------------------------------------------------------------------------------------------------- host side
static_assert(MEDA_PLAN_WIDE_MAX_GROUPS == kWideMaxGroups, "the sizing helpers of meda_geo_wide.h count these groups");

template <class Geo>
int launch_wide(int n_tasks, int width, int length, int n_agents, const PlanIO &io, const uint8_t *avoid, int H, void *work, void *stream) {
    const size_t lds = lds_bytes_wide(width, length, n_agents, H);
    static LdsLimit lds_limit;   // one per kernel
    if (lds > 64 * 1024)
        if (const int rc = lds_limit.raise((const void *)k_meda_plan_wide<Geo>, kLdsBudget)) return rc;
    LAUNCH(k_meda_plan_wide<Geo>, dim3((unsigned)groups_of(n_tasks)), dim3(kWave), lds, (hipStream_t)stream, n_tasks, width, length,
           n_agents, io, avoid, H, (Row128 *)work);
    return 0;
}

}  // namespace

extern "C" {

int meda_plan_wide_max_dim(void) { return MEDA_PLAN_WIDE_MAX_DIM; }

int meda_plan_wide_max_groups(void) { return MEDA_PLAN_WIDE_MAX_GROUPS; }

int meda_plan_wide_lds_levels(int32_t width, int32_t length, int32_t n_agents) {
    if (const int rc = Plain::check_sizes(width, length, n_agents)) return rc;
    return levels_in_lds(width, length, n_agents, 0);
}

int meda_plan_wide_lds_bytes(int32_t width, int32_t length, int32_t n_agents, int32_t lds_levels) {
    if (const int rc = Plain::check_sizes(width, length, n_agents)) return rc;
    return (int)lds_bytes_wide(width, length, n_agents, levels_in_lds(width, length, n_agents, lds_levels));
}

int64_t meda_plan_wide_work_bytes(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t lds_levels) {
    if (n_tasks < 0) return MEDA_PLAN_WIDE_ERR_BAD_ARG;
    if (const int rc = Plain::check_sizes(width, length, n_agents)) return rc;
    return (int64_t)groups_of(n_tasks) * (int64_t)slice_bytes(width, length, levels_in_lds(width, length, n_agents, lds_levels));
}

int meda_plan_wide_route(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t safe, const int32_t *d_starts,
                         const int32_t *d_goals, const uint8_t *d_avoid, uint8_t *d_route, int8_t *d_u, int32_t *d_steps,
                         uint8_t *d_success, int32_t *d_attempt, int32_t *d_lower_bound, void *d_work, int64_t work_bytes,
                         int32_t lds_levels, void *stream) {
    if (n_tasks < 0) return MEDA_PLAN_WIDE_ERR_BAD_ARG;
    if (const int rc = Plain::check_sizes(width, length, n_agents)) return rc;
    if (!d_starts || !d_goals || !d_route || !d_u || !d_steps || !d_success || !d_attempt || !d_lower_bound)
        return MEDA_PLAN_WIDE_ERR_BAD_ARG;
    const int H = levels_in_lds(width, length, n_agents, lds_levels);
    const int64_t need = (int64_t)groups_of(n_tasks) * (int64_t)slice_bytes(width, length, H);
    if (need > 0 && (!d_work || work_bytes < need || ((uintptr_t)d_work & (sizeof(Row128) - 1)))) return MEDA_PLAN_WIDE_ERR_BAD_ARG;
    if (n_tasks == 0) return 0;
    const PlanIO io = {d_starts, d_goals, d_route, d_u, d_steps, d_success, d_attempt, d_lower_bound};
    return safe ? launch_wide<Safe>(n_tasks, width, length, n_agents, io, d_avoid, H, d_work, stream)
                : launch_wide<Plain>(n_tasks, width, length, n_agents, io, d_avoid, H, d_work, stream);
}

int meda_plan_wide_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
