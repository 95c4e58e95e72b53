// route_plan.hip -- the deterministic space-time planner for DMFB of include/route_plan.h (libroute_plan.so).
//
// One workgroup of ONE wave per task; lane x owns chip row x as a 64-bit word (bit y = cell (x, y)).  A level of the search is
//     src        = reach[t] & ~F2[t+1] & ~goal                      (the cells a move may start from)
//     reach[t+1] = dilate4(src) & ~blocked & ~(F2[t+1] | F2[t])      (and without the goal while hold[t+1] is false)
// in registers: two shifts inside the row word, the rows above and below from the neighbouring lanes.  `src` of every level goes to
// LDS, so the walk back from the goal only tests bits (five lanes, one per action, and a ballot: the lowest set lane is the lowest
// action number) and needs no parent table.  The planned paths live in LDS too, in planning order (slot p = the p-th droplet of
// the attempt), so F2 of a level is a loop over the slots planned so far.  With reservations (R > 0) the lane also holds one word,
// its row of the union of near(start) over the droplets not yet planned, which joins F2 at the levels 1 .. R.
#include "../../include/route_plan.h"

#define HIP_ABI_TAG "route_plan"
#define HIP_ABI_ERR ROUTE_PLAN_ERR_HIP
#include "hip_abi.h"
#include "plan_core.h"

namespace {

struct Dmfb {
    static constexpr int kMaxAgents = ROUTE_PLAN_MAX_AGENTS, kBadArg = ROUTE_PLAN_ERR_BAD_ARG, kUnsupported = ROUTE_PLAN_ERR_UNSUPPORTED;
    static constexpr int kFirstLevel = 0, kStepsAfterArrival = 0;
    static constexpr int kParkMin = 1, kMissingAction = 0;   // a droplet off its goal may be parked; STALL

    static __host__ __device__ int limit(int W, int L) { return 2 * (W + L); }

    static int check_sizes(int width, int length, int n_agents) {
        if (width <= 0 || length <= 0 || n_agents <= 0 || n_agents > ROUTE_PLAN_MAX_AGENTS) return ROUTE_PLAN_ERR_BAD_ARG;
        if (width > ROUTE_PLAN_MAX_DIM || length > ROUTE_PLAN_MAX_DIM) return ROUTE_PLAN_ERR_UNSUPPORTED;
        return 0;
    }

    static __device__ int dist(int sx, int sy, int gx, int gy) { return abs(sx - gx) + abs(sy - gy); }

    // Row `row` of near(q): bits qy-1 .. qy+1 when the row is within one of qx (bits off the chip are masked by `blocked` later).
    static __device__ u64 near_row(int row, int qx, int qy) {
        const int d = row - qx;
        if (d < -1 || d > 1) return 0;
        return qy == 0 ? 3ull : (7ull << (qy - 1));
    }

    static __device__ bool near_goal(int dx, int dy) { return dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1; }

    // Every value that decides a branch is the same in all lanes.
    template <bool STORE>
    static __device__ int forward(int lane, int W, int L, int T, int n, int sx, int sy, int gx, int gy, u64 blocked,
                                  const unsigned short *path, int np, u64 *levels, Reserved res) {
        int last_bad = last_bad_level<Dmfb>(path, T, n, np, lane, gx, gy);
        // a reserved goal is held from the levels 1 .. R too (res.levels <= T)
        if (res.levels > 0 && res.levels > last_bad && ((__shfl(res.row, gx) >> gy) & 1ull)) last_bad = res.levels;
        if (sx == gx && sy == gy) return last_bad < 0 ? 0 : -1;
        const u64 goalbit = lane == gx ? (1ull << gy) : 0ull;
        u64 reach = lane == sx ? (1ull << sy) : 0ull;
        u64 f2prev = near_union_row<Dmfb>(path, np, lane);
        constexpr int kGoOn = -2;
        // reach[t] -> reach[t + 1] against f2 = F2'[t + 1]: forward's answer, or kGoOn
        auto level = [&](int t, u64 f2) -> int {
            const u64 src = reach & ~f2 & ~goalbit;
            if (STORE && lane < W) levels[t * W + lane] = src;
            u64 up = __shfl_up(src, 1), dn = __shfl_down(src, 1);
            if (lane == 0) up = 0;
            if (lane == kWave - 1) dn = 0;
            u64 nr = (src | (src << 1) | (src >> 1) | up | dn) & ~blocked & ~(f2 | f2prev);
            if (t + 1 <= last_bad) nr &= ~goalbit;
            reach = nr;
            f2prev = f2;
            if (__any((reach & goalbit) != 0)) return t + 1;
            if (!__any(reach != 0)) return -1;
            return kGoOn;
        };
        // the levels that carry the reservations first (none when nothing is reserved), then the rule's own loop
        int t = 0;
        for (; t < res.levels && t <= T - 2; ++t) {
            const int r = level(t, near_union_row<Dmfb>(path + (t + 1) * n, np, lane) | res.row);
            if (r != kGoOn) return r;
        }
        for (; t <= T - 2; ++t) {
            const int r = level(t, near_union_row<Dmfb>(path + (t + 1) * n, np, lane));
            if (r != kGoOn) return r;
        }
        return -1;
    }

    static __device__ void walk_back(int lane, int W, int L, int n, int slot, int a, int gx, int gy, const u64 *levels,
                                     unsigned short *path) {
        int cx = gx, cy = gy;
        if (lane == 0) path[a * n + slot] = pack_xy(cx, cy);
        const int dx = lane == 1 ? 1 : lane == 2 ? -1 : 0;   // lane u < 5 tests the predecessor of action u
        const int dy = lane == 3 ? -1 : lane == 4 ? 1 : 0;
        for (int t = a - 1; t >= 0; --t) {
            const int px = cx - dx, py = cy - dy;
            bool ok = false;
            if (lane < 5 && px >= 0 && px < W && py >= 0 && py < L) ok = (levels[t * W + px] >> py) & 1ull;
            const u64 m = __ballot(ok);
            const int u = m ? __ffsll((long long)m) - 1 : 0;   // never empty: level t + 1 was built from level t
            cx -= (u == 1) - (u == 2);
            cy -= (u == 4) - (u == 3);
            if (lane == 0) path[t * n + slot] = pack_xy(cx, cy);
        }
    }

    static __device__ int action(int p0, int p1, int gx, int gy, int W, int L) {
        const int dx = (p1 & 255) - (p0 & 255), dy = (p1 >> 8) - (p0 >> 8);
        return dx == 1 ? 1 : dx == -1 ? 2 : dy == -1 ? 3 : dy == 1 ? 4 : 0;
    }
};

// The blocked row of this lane: off the chip, a block or an avoided cell.
__device__ inline u64 blocked_row(int lane, size_t b, int W, int L, int nb, const int32_t *__restrict__ blocks,
                                  const uint8_t *__restrict__ avoid) {
    u64 blocked = ~0ull;
    if (lane < W) {
        blocked = ~run(0, L - 1);
        for (int k = 0; k < nb; ++k) {
            const int32_t *q = blocks + (b * nb + k) * 4;
            if (lane >= q[0] && lane <= q[1]) blocked |= run(q[2], q[3]);
        }
        if (avoid) {
            const uint8_t *row = avoid + (b * W + lane) * L;
            for (int y = 0; y < L; ++y) blocked |= row[y] ? (1ull << y) : 0ull;
        }
    }
    return blocked;
}

__global__ __launch_bounds__(kWave) void k_route_plan_dmfb(int W, int L, int n, const int32_t *__restrict__ starts, const int32_t *__restrict__ goals,
                                                           uint8_t *__restrict__ route, int8_t *__restrict__ act, int32_t *__restrict__ steps,
                                                           uint8_t *__restrict__ success, int32_t *__restrict__ attempt, int32_t *__restrict__ lower,
                                                           int nb, const int32_t *__restrict__ blocks, const uint8_t *__restrict__ avoid,
                                                           int reserve, int retries) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int T = Dmfb::limit(W, L);
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    const u64 blocked = blocked_row(lane, b, W, L, nb, blocks, avoid);
    plan_task<Dmfb>(blockIdx.x, W, L, T, n, blocked, (u64 *)smem, (unsigned short *)(smem + (size_t)(T - 1) * W * 8),
                    {starts, goals, route, act, steps, success, attempt, lower}, reserve, retries);
}

// Lock-step t of the closed loop, one chip per workgroup (follow_chip of plan_core.h): a frozen chip returns at once, a chip that
// is where its kept plan says costs one compare, any other is replanned from where it is.
__global__ __launch_bounds__(kWave) void k_route_follow_dmfb(int W, int L, int n, int t, const int32_t *__restrict__ goals, int nb,
                                                             const int32_t *__restrict__ blocks, const uint8_t *__restrict__ avoid,
                                                             const uint8_t *__restrict__ positions, FollowState st, int reserve,
                                                             int retries) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int T = Dmfb::limit(W, L);
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    if (!st.active[b]) return;

    // where the chip is, and where it should be
    const int pos = lane < n ? ((const unsigned short *)positions)[(b * (T + 1) + t) * n + lane] : 0;
    int gx = 0, gy = 0;
    if (lane < n) { gx = goals[(b * n + lane) * 2]; gy = goals[(b * n + lane) * 2 + 1]; }
    const bool away = lane < n && ((pos & 255) != gx || (pos >> 8) != gy);
    if (t > 0 && !__any(away)) {   // the last step brought every droplet home: the env ended the episode
        if (lane == 0) st.active[b] = 0;
        return;
    }
    follow_chip<Dmfb>(b, W, L, T, n, t, pos, gx, gy, st, (u64 *)smem, (unsigned short *)(smem + (size_t)(T - 1) * W * 8), reserve, retries,
                      [&] { return blocked_row(lane, b, W, L, nb, blocks, avoid); });
}

}  // namespace

extern "C" {

int route_plan_max_dim(void) { return ROUTE_PLAN_MAX_DIM; }

int route_plan_lds_bytes(int32_t width, int32_t length, int32_t n_agents) {
    if (const int rc = Dmfb::check_sizes(width, length, n_agents)) return rc;
    return (int)lds_bytes(Dmfb::limit(width, length), width, n_agents);
}

static bool rule_ok(int32_t reserve, int32_t retries) {
    return reserve >= 0 && reserve <= ROUTE_PLAN_MAX_RESERVE && retries >= 0 && retries <= ROUTE_PLAN_MAX_RETRIES;
}

int route_plan_dmfb_opt(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t n_blocks, const int32_t *d_starts,
                        const int32_t *d_goals, const int32_t *d_blocks, const uint8_t *d_avoid, uint8_t *d_route, int8_t *d_u,
                        int32_t *d_steps, uint8_t *d_success, int32_t *d_attempt, int32_t *d_lower_bound, int32_t reserve,
                        int32_t retries, void *stream) {
    if (n_blocks < 0 || !rule_ok(reserve, retries)) return ROUTE_PLAN_ERR_BAD_ARG;
    const PlanIO io = {d_starts, d_goals, d_route, d_u, d_steps, d_success, d_attempt, d_lower_bound};
    return launch_plan<Dmfb>(k_route_plan_dmfb, n_tasks, width, length, n_agents, io, n_blocks == 0 || d_blocks, stream, n_blocks,
                             d_blocks, d_avoid, reserve, retries);
}

int route_plan_dmfb(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t n_blocks, const int32_t *d_starts,
                    const int32_t *d_goals, const int32_t *d_blocks, const uint8_t *d_avoid, uint8_t *d_route, int8_t *d_u,
                    int32_t *d_steps, uint8_t *d_success, int32_t *d_attempt, int32_t *d_lower_bound, void *stream) {
    return route_plan_dmfb_opt(n_tasks, width, length, n_agents, n_blocks, d_starts, d_goals, d_blocks, d_avoid, d_route, d_u, d_steps,
                               d_success, d_attempt, d_lower_bound, 0, 0, stream);
}

int route_follow_dmfb_opt(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t n_blocks, int32_t t,
                          const int32_t *d_goals, const int32_t *d_blocks, const uint8_t *d_avoid, const uint8_t *d_positions,
                          uint8_t *d_route, int8_t *d_route_u, int32_t *d_cursor, uint8_t *d_partial, int32_t *d_replans,
                          uint8_t *d_gave_up, uint8_t *d_active, int32_t *d_steps, int32_t *d_lower_bound, int32_t *d_actions,
                          int8_t *d_u, int32_t reserve, int32_t retries, void *stream) {
    if (n_blocks < 0 || !rule_ok(reserve, retries)) return ROUTE_PLAN_ERR_BAD_ARG;
    const FollowState st = {d_route, d_route_u, d_cursor, d_partial, d_replans, d_gave_up, d_active, d_steps, d_lower_bound, d_actions,
                            d_u};
    return launch_follow<Dmfb>(k_route_follow_dmfb, n_tasks, width, length, n_agents, t, d_goals, d_positions, st, n_blocks == 0 || d_blocks,
                               stream, n_blocks, d_blocks, d_avoid, d_positions, st, reserve, retries);
}

int route_follow_dmfb(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t n_blocks, int32_t t,
                      const int32_t *d_goals, const int32_t *d_blocks, const uint8_t *d_avoid, const uint8_t *d_positions,
                      uint8_t *d_route, int8_t *d_route_u, int32_t *d_cursor, uint8_t *d_partial, int32_t *d_replans,
                      uint8_t *d_gave_up, uint8_t *d_active, int32_t *d_steps, int32_t *d_lower_bound, int32_t *d_actions, int8_t *d_u,
                      void *stream) {
    return route_follow_dmfb_opt(n_tasks, width, length, n_agents, n_blocks, t, d_goals, d_blocks, d_avoid, d_positions, d_route,
                                 d_route_u, d_cursor, d_partial, d_replans, d_gave_up, d_active, d_steps, d_lower_bound, d_actions, d_u,
                                 0, 0, stream);
}

int route_plan_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
