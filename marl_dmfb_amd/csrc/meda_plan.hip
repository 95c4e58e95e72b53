// meda_plan.hip -- the deterministic space-time planner for MEDA of include/meda_plan.h (libmeda_plan.so): the plain rule of the
// geometry in meda_geo.h, one workgroup of ONE wave per task.
#include "../../include/meda_plan.h"

#define HIP_ABI_TAG "meda_plan"
#define HIP_ABI_ERR MEDA_PLAN_ERR_HIP
#include "hip_abi.h"
#include "plan_core.h"
#include "meda_geo.h"

namespace {

struct PlanAbi {
    static constexpr int kMinDim = MEDA_PLAN_MIN_DIM, kMaxDim = MEDA_PLAN_MAX_DIM, kMaxAgents = MEDA_PLAN_MAX_AGENTS;
    static constexpr int kBadArg = MEDA_PLAN_ERR_BAD_ARG, kUnsupported = MEDA_PLAN_ERR_UNSUPPORTED;
};
typedef Meda<false, PlanAbi> Plain;

}  // namespace

extern "C" {

int meda_plan_max_dim(void) { return MEDA_PLAN_MAX_DIM; }

int meda_plan_lds_bytes(int32_t width, int32_t length, int32_t n_agents) {
    if (const int rc = Plain::check_sizes(width, length, n_agents)) return rc;
    return (int)lds_bytes(Plain::limit(width, length), width, n_agents);
}

int meda_plan_route(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, const int32_t *d_starts,
                    const int32_t *d_goals, const uint8_t *d_avoid, uint8_t *d_route, int8_t *d_u, int32_t *d_steps,
                    uint8_t *d_success, int32_t *d_attempt, int32_t *d_lower_bound, void *stream) {
    const PlanIO io = {d_starts, d_goals, d_route, d_u, d_steps, d_success, d_attempt, d_lower_bound};
    return launch_plan<Plain>(k_meda_plan<Plain>, n_tasks, width, length, n_agents, io, true, stream, d_avoid);
}

int meda_plan_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
