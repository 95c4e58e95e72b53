// route_plan.hip -- the deterministic space-time planner for DMFB of include/route_plan.h (libroute_plan.so).
//
// One workgroup of ONE wave per task; lane x owns chip row x as a 64-bit word (bit y = cell (x, y)).  A level of the search is
//     src        = reach[t] & ~F2[t+1] & ~goal                      (the cells a move may start from)
//     reach[t+1] = dilate4(src) & ~blocked & ~(F2[t+1] | F2[t])      (and without the goal while hold[t+1] is false)
// in registers: two shifts inside the row word, the rows above and below from the neighbouring lanes.  `src` of every level goes to
// LDS, so the walk back from the goal only tests bits (five lanes, one per action, and a ballot: the lowest set lane is the lowest
// action number) and needs no parent table.  The planned paths live in LDS too, in planning order (slot p = the p-th droplet of
// the attempt), so F2 of a level is a loop over the slots planned so far.
#include "../../include/route_plan.h"

#define HIP_ABI_TAG "route_plan"
#define HIP_ABI_ERR ROUTE_PLAN_ERR_HIP
#include "hip_abi.h"

namespace {

typedef unsigned long long u64;
constexpr int kWave = 64;
constexpr int kMaxN = ROUTE_PLAN_MAX_AGENTS;
constexpr size_t kLdsBudget = 160 * 1024 - 1024;   // a workgroup may hold all 160 KiB; 1 KiB stays for the static arrays

__device__ inline unsigned short pack_xy(int x, int y) { return (unsigned short)(x | (y << 8)); }

// Row `row` of near(q): bits qy-1 .. qy+1 when the row is within one of qx (bits off the chip are masked by `blocked` later).
__device__ inline u64 near_row(int row, int qx, int qy) {
    const int d = row - qx;
    if (d < -1 || d > 1) return 0;
    return qy == 0 ? 3ull : (7ull << (qy - 1));
}

// Row `lane` of F2 at one level: path_t = the positions of the `np` planned slots at that level.
__device__ inline u64 f2_row(const unsigned short *path_t, int np, int lane) {
    u64 m = 0;
    for (int q = 0; q < np; ++q) {
        const int p = path_t[q];
        m |= near_row(lane, p & 255, p >> 8);
    }
    return m;
}

// The search of one droplet against the first `np` slots of `path`.  Returns its arrival time, or -1.  STORE: level t's `src`
// goes to levels[t * W + row] for the walk back.  Every value that decides a branch is the same in all lanes.
template <bool STORE>
__device__ int forward(int lane, int W, int T, int n, int sx, int sy, int gx, int gy, u64 blocked, const unsigned short *path, int np,
                       u64 *levels) {
    // the last level whose F2 holds the goal: hold[a] is a > last_bad
    int last_bad = -1;
    for (int t = lane; t <= T; t += kWave) {
        const unsigned short *pt = path + t * n;
        for (int q = 0; q < np; ++q) {
            const int p = pt[q], dx = (p & 255) - gx, dy = (p >> 8) - gy;
            if (dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1) last_bad = t;
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const int o = __shfl_xor(last_bad, off);
        last_bad = o > last_bad ? o : last_bad;
    }
    if (sx == gx && sy == gy) return last_bad < 0 ? 0 : -1;
    const u64 goalbit = lane == gx ? (1ull << gy) : 0ull;
    u64 reach = lane == sx ? (1ull << sy) : 0ull;
    u64 f2prev = f2_row(path, np, lane);
    for (int t = 0; t <= T - 2; ++t) {
        const u64 f2 = f2_row(path + (t + 1) * n, np, lane);
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
    }
    return -1;
}

// The path of the droplet that arrived at level `a`, walked back through `levels` into slot `slot` of `path`.
__device__ void backtrack(int lane, int W, int L, int T, int n, int slot, int a, int gx, int gy, const u64 *levels,
                          unsigned short *path) {
    int cx = gx, cy = gy;
    if (lane == 0) path[a * n + slot] = pack_xy(gx, gy);
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
    for (int t = a + 1 + lane; t <= T; t += kWave) path[t * n + slot] = pack_xy(gx, gy);
}

__global__ __launch_bounds__(kWave) void k_route_plan_dmfb(int W, int L, int n, int nb, const int32_t *__restrict__ starts,
                                                           const int32_t *__restrict__ goals, const int32_t *__restrict__ blocks,
                                                           const uint8_t *__restrict__ avoid, uint8_t *__restrict__ route,
                                                           int8_t *__restrict__ act, int32_t *__restrict__ steps_out,
                                                           uint8_t *__restrict__ success, int32_t *__restrict__ attempt,
                                                           int32_t *__restrict__ lower) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int s_sx[kMaxN], s_sy[kMaxN], s_gx[kMaxN], s_gy[kMaxN], s_dist[kMaxN], s_rank[kMaxN], s_order[kMaxN];
    const int T = 2 * (W + L);
    u64 *levels = (u64 *)smem;                                             // [T - 1][W]
    unsigned short *path = (unsigned short *)(smem + (size_t)(T - 1) * W * 8);   // [T + 1][n], slot-major inside a level
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;

    if (lane < n) {
        const int32_t *s = starts + (b * n + lane) * 2, *g = goals + (b * n + lane) * 2;
        s_sx[lane] = s[0]; s_sy[lane] = s[1]; s_gx[lane] = g[0]; s_gy[lane] = g[1];
        s_dist[lane] = abs(s[0] - g[0]) + abs(s[1] - g[1]);
    }
    __syncthreads();
    if (lane < n) {   // base order: descending distance, ties by ascending index
        int r = 0;
        for (int j = 0; j < n; ++j) r += s_dist[j] > s_dist[lane] || (s_dist[j] == s_dist[lane] && j < lane);
        s_rank[lane] = r;
        s_order[r] = lane;
    }
    // the blocked row of this lane: off the chip, a block or an avoided cell
    u64 blocked = ~0ull;
    if (lane < W) {
        blocked = L < 64 ? (~0ull << L) : 0ull;
        for (int k = 0; k < nb; ++k) {
            const int32_t *q = blocks + (b * nb + k) * 4;
            const int x0 = q[0], x1 = q[1], y0 = q[2] < 0 ? 0 : q[2], y1 = q[3] > 63 ? 63 : q[3];
            if (lane >= x0 && lane <= x1 && y0 <= y1) blocked |= (~0ull << y0) & (~0ull >> (63 - y1));
        }
        if (avoid) {
            const uint8_t *row = avoid + (b * W + lane) * L;
            for (int y = 0; y < L; ++y) blocked |= row[y] ? (1ull << y) : 0ull;
        }
    }
    __syncthreads();

    // lower bound: every droplet alone
    int lb = 0;
    for (int i = 0; i < n; ++i) {
        const int a = forward<false>(lane, W, T, n, s_sx[i], s_sy[i], s_gx[i], s_gy[i], blocked, path, 0, levels);
        lb = (a < 0 || lb < 0) ? -1 : (a > lb ? a : lb);
    }

    int kept = -1, steps = 0;
    for (int k = 0; k < n && kept < 0; ++k) {
        int st = 0, p = 0;
        for (; p < n; ++p) {
            const int i = s_order[(p + k) % n];
            const int gx = s_gx[i], gy = s_gy[i];
            const int a = forward<true>(lane, W, T, n, s_sx[i], s_sy[i], gx, gy, blocked, path, p, levels);
            if (a < 0) break;
            __syncthreads();   // the levels are complete before any lane reads another lane's rows
            backtrack(lane, W, L, T, n, p, a, gx, gy, levels, path);
            __syncthreads();   // the path is complete before the next droplet plans against it
            st = a > st ? a : st;
        }
        if (p == n) { kept = k; steps = st; }
    }
    __syncthreads();

    if (lane == 0) {
        steps_out[b] = steps;
        success[b] = kept >= 0;
        attempt[b] = kept;
        lower[b] = lb;
    }
    unsigned short *route16 = (unsigned short *)route + b * (size_t)(T + 1) * n;   // (x, y) bytes of one droplet = one 16-bit store
    for (int idx = lane; idx < (T + 1) * n; idx += kWave) {
        const int t = idx / n, i = idx - t * n;
        const int slot = (s_rank[i] - kept + n) % n;
        route16[idx] = kept >= 0 ? path[t * n + slot] : pack_xy(s_sx[i], s_sy[i]);
    }
    int8_t *u_out = act + b * (size_t)T * n;
    for (int idx = lane; idx < T * n; idx += kWave) {
        const int t = idx / n, i = idx - t * n;
        int u = -1;
        if (kept >= 0 && t < steps) {
            const int slot = (s_rank[i] - kept + n) % n;
            const int p0 = path[t * n + slot], p1 = path[(t + 1) * n + slot];
            const int dx = (p1 & 255) - (p0 & 255), dy = (p1 >> 8) - (p0 >> 8);
            u = dx == 1 ? 1 : dx == -1 ? 2 : dy == -1 ? 3 : dy == 1 ? 4 : 0;
        }
        u_out[idx] = (int8_t)u;
    }
}

int check_sizes(int width, int length, int n_agents) {
    if (width <= 0 || length <= 0 || n_agents <= 0 || n_agents > ROUTE_PLAN_MAX_AGENTS) return ROUTE_PLAN_ERR_BAD_ARG;
    if (width > ROUTE_PLAN_MAX_DIM || length > ROUTE_PLAN_MAX_DIM) return ROUTE_PLAN_ERR_UNSUPPORTED;
    return 0;
}

size_t lds_bytes(int width, int length, int n_agents) {
    const size_t T = 2 * ((size_t)width + (size_t)length);
    return (T - 1) * (size_t)width * 8 + (((T + 1) * (size_t)n_agents * 2 + 15) & ~(size_t)15);
}

}  // namespace

extern "C" {

int route_plan_max_dim(void) { return ROUTE_PLAN_MAX_DIM; }

int route_plan_lds_bytes(int32_t width, int32_t length, int32_t n_agents) {
    if (const int rc = check_sizes(width, length, n_agents)) return rc;
    return (int)lds_bytes(width, length, n_agents);
}

int route_plan_dmfb(int32_t n_tasks, int32_t width, int32_t length, int32_t n_agents, int32_t n_blocks, const int32_t *d_starts,
                    const int32_t *d_goals, const int32_t *d_blocks, const uint8_t *d_avoid, uint8_t *d_route, int8_t *d_u,
                    int32_t *d_steps, uint8_t *d_success, int32_t *d_attempt, int32_t *d_lower_bound, void *stream) {
    if (n_tasks < 0 || n_blocks < 0) return ROUTE_PLAN_ERR_BAD_ARG;
    if (const int rc = check_sizes(width, length, n_agents)) return rc;
    if (!d_starts || !d_goals || !d_route || !d_u || !d_steps || !d_success || !d_attempt || !d_lower_bound)
        return ROUTE_PLAN_ERR_BAD_ARG;
    if (n_blocks > 0 && !d_blocks) return ROUTE_PLAN_ERR_BAD_ARG;
    const size_t lds = lds_bytes(width, length, n_agents);
    if (lds > kLdsBudget) return ROUTE_PLAN_ERR_UNSUPPORTED;
    if (n_tasks == 0) return 0;
    static LdsLimit lds_limit;
    if (lds > 64 * 1024)
        if (const int rc = lds_limit.raise((const void *)k_route_plan_dmfb, kLdsBudget)) return rc;
    LAUNCH(k_route_plan_dmfb, dim3((unsigned)n_tasks), dim3(kWave), lds, (hipStream_t)stream, width, length, n_agents, n_blocks,
           d_starts, d_goals, d_blocks, d_avoid, d_route, d_u, d_steps, d_success, d_attempt, d_lower_bound);
    return 0;
}

int route_plan_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
