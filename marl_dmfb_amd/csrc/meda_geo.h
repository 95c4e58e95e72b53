// meda_geo.h -- the MEDA geometry of the planning procedure of plan_core.h: what meda_plan.hip (the open-loop planner) and
// meda_follow.hip (the failure-safe rule and the closed loop) both compile.
//
// One workgroup of ONE wave per task; lane y owns chip row y as a 64-bit word (bit x = centre (x, y)).  A level of the search is
//     src        = reach[t] & ~G                                            (the centres a move may start from)
//     reach[t+1] = (union over the nine actions of move(src, u)) & ~blocked & ~F[t+1]
// in registers.  The rows 1, 2 and 3 below and above come from the neighbouring lanes; N / S take the row 3 away, the diagonals
// the row 2 away shifted by 2 bits, E / W the own row shifted by 3.  The clamps fold: the edge lane also takes the rows that would
// leave the range, and the bits that would leave the column range are OR-ed onto the edge column (taken before the shift).
// `src` of every level goes to LDS, so the walk back only tests bits: the at most 4 * 4 + 4 * 9 + 1 = 53 (action, source) pairs
// of a level are one lane each, ordered by (action, y, x), and one ballot gives the lowest.  The planned paths live in LDS too, in
// planning order (slot p = the p-th droplet of the attempt), so F of a level is a loop over the slots planned so far.
//
// Meda<SAFE, Abi>: SAFE = the failure-safe rule: with N[t] = F[t], level 0 included,
//     src[t]     = reach[t] & ~G & ~N[t+1]                                  (this droplet's move fails, the planned one moves)
//     reach[t+1] = (union of the moves of src[t]) & ~blocked & ~N[t+1] & ~N[t]    (the planned one's move fails, this one moves)
// and the arrival at level t needs the goal outside N[t] .. N[T].  Abi: kMinDim, kMaxDim, kMaxAgents, kBadArg, kUnsupported of
// the public header the translation unit implements.
//
// Include it after hip_abi.h and plan_core.h.
#pragma once

namespace {

constexpr int kStall = 8;

// Row `row` of G: the disc d2 < 16 around the goal.
__device__ inline u64 goal_row(int row, int gx, int gy) {
    int d = row - gy;
    d = d < 0 ? -d : d;
    if (d > 3) return 0;
    return run(gx - (d == 3 ? 2 : 3), gx + (d == 3 ? 2 : 3));
}

__device__ inline u64 lane_down(u64 v, int k, int lane) { const u64 r = __shfl_down(v, k); return lane + k < kWave ? r : 0ull; }
__device__ inline u64 lane_up(u64 v, int k, int lane) { const u64 r = __shfl_up(v, k); return lane >= k ? r : 0ull; }

// The column moves of a row word with their clamp folds; xh = length - 3.  The fold bits are taken before the shift.
__device__ inline u64 east(u64 w, int k, int xh) {
    const u64 fold = w & run(xh - k + 1, xh);
    return ((w << k) & run(2, xh)) | (fold ? (1ull << xh) : 0ull);
}
__device__ inline u64 west(u64 w, int k, int xh) {
    const u64 fold = w & run(2, 2 + k - 1);
    return ((w >> k) & run(2, xh)) | (fold ? 4ull : 0ull);
}

// The source coordinates of one axis: the j-th lowest c in lo .. hi with clamp(c + d) == to, or -1.
__device__ inline int axis_source(int to, int d, int j, int lo, int hi) {
    int c;
    if (d == 0) c = j == 0 ? to : -1;
    else if (d > 0) c = to < hi ? (j == 0 ? to - d : -1) : (j <= d ? hi - d + j : -1);
    else c = to > lo ? (j == 0 ? to - d : -1) : (j <= -d ? lo + j : -1);
    return (c < lo || c > hi) ? -1 : c;
}

__device__ inline int delta_x(int u) { return (u == 1) ? 3 : (u == 3) ? -3 : (u == 4 || u == 5) ? 2 : (u == 6 || u == 7) ? -2 : 0; }
__device__ inline int delta_y(int u) { return (u == 0) ? -3 : (u == 2) ? 3 : (u == 5 || u == 6) ? 2 : (u == 4 || u == 7) ? -2 : 0; }

template <bool SAFE, class Abi> struct Meda {
    static constexpr int kMaxAgents = Abi::kMaxAgents, kBadArg = Abi::kBadArg, kUnsupported = Abi::kUnsupported;
    static constexpr int kFirstLevel = SAFE ? 0 : 1, kStepsAfterArrival = 1;
    static constexpr int kParkMin = 16, kMissingAction = kStall;   // a droplet inside its goal disc is never parked: the env snaps it

    static __host__ __device__ int limit(int W, int L) { return W + L; }

    static int check_sizes(int width, int length, int n_agents) {
        if (width < Abi::kMinDim || length < Abi::kMinDim || n_agents <= 0) return Abi::kBadArg;
        if (width > Abi::kMaxDim || length > Abi::kMaxDim || n_agents > Abi::kMaxAgents) return Abi::kUnsupported;
        return 0;
    }

    static __device__ int dist(int sx, int sy, int gx, int gy) { return (sx - gx) * (sx - gx) + (sy - gy) * (sy - gy); }

    // Row `row` of the disc d2 < 36 around (px, py): a run whose half-width depends on |row - py| alone.
    static __device__ u64 near_row(int row, int px, int py) {
        int d = row - py;
        d = d < 0 ? -d : d;
        if (d > 5) return 0;
        const int hw = d <= 3 ? 5 : (d == 4 ? 4 : 3);
        return run(px - hw, px + hw);
    }

    static __device__ bool near_goal(int dx, int dy) { return dx * dx + dy * dy < 36; }

    // Every value that decides a branch is the same in all lanes.
    template <bool STORE>
    static __device__ int forward(int lane, int W, int L, int T, int n, int sx, int sy, int gx, int gy, u64 blocked,
                                  const unsigned short *path, int np, u64 *levels, Reserved) {   // MEDA reserves nothing
        const int xh = L - 3, yh = W - 3;
        const int last_bad = last_bad_level<Meda>(path, T, n, np, lane, gx, gy);
        const u64 G = goal_row(lane, gx, gy);
        u64 reach = lane == sy ? (1ull << sx) : 0ull;
        u64 nprev = SAFE ? near_union_row<Meda>(path, np, lane) : 0ull;   // N[t]; the plain rule has no such guard
        for (int t = 0; t <= T - 2; ++t) {
            const u64 arr = reach & G;   // reach[t] lies outside F[t] already (t >= 1), and the plain F[0] is empty
            if (t + (SAFE ? 0 : 1) > last_bad) {   // hold[t + 1]; safe: the goal is clear before the snap step too
                const u64 rows = __ballot(arr != 0);
                if (rows) {
                    const int y = __ffsll((long long)rows) - 1;
                    const u64 w = __shfl(arr, y);
                    return t | ((__ffsll((long long)w) - 1) << 8) | (y << 16);
                }
            }
            if (t == T - 2) break;
            u64 next = 0;   // F[t+1]
            if (SAFE) next = near_union_row<Meda>(path + (t + 1) * n, np, lane);
            const u64 src = reach & ~G & ~next;
            if (STORE && lane < W) levels[t * W + lane] = src;
            if (!__any(src != 0)) return -1;
            const u64 d1 = lane_down(src, 1, lane), d2 = lane_down(src, 2, lane), d3 = lane_down(src, 3, lane);
            const u64 u1 = lane_up(src, 1, lane), u2 = lane_up(src, 2, lane), u3 = lane_up(src, 3, lane);
            const bool top = lane == 2, bottom = lane == yh;
            const u64 n3 = d3 | (top ? (src | d1 | d2) : 0ull);      // rows moved by (0, -3), the clamp folded into row 2
            const u64 n2 = d2 | (top ? (src | d1) : 0ull);
            const u64 s3 = u3 | (bottom ? (src | u1 | u2) : 0ull);   // rows moved by (0, +3), folded into row width-3
            const u64 s2 = u2 | (bottom ? (src | u1) : 0ull);
            const u64 diag = n2 | s2;
            u64 nr = src | n3 | s3 | east(src, 3, xh) | west(src, 3, xh) | east(diag, 2, xh) | west(diag, 2, xh);
            if (!SAFE) next = near_union_row<Meda>(path + (t + 1) * n, np, lane);
            nr &= ~blocked & ~next & ~nprev;
            reach = nr;
            if (SAFE) nprev = next;
        }
        return -1;
    }

    static __device__ void walk_back(int lane, int W, int L, int n, int slot, int r, int gx, int gy, const u64 *levels,
                                     unsigned short *path) {
        const int a = r & 255;
        int cx = (r >> 8) & 255, cy = r >> 16;
        if (lane == 0) path[a * n + slot] = pack_xy(cx, cy);
        // this lane's (action, source index) pair, lanes ordered by (action, y, x)
        int u = -1, jy = 0, jx = 0;
        if (lane < 16) {
            u = lane >> 2;
            if (u & 1) jx = lane & 3; else jy = lane & 3;
        } else if (lane < 52) {
            const int k = lane - 16;
            u = 4 + k / 9;
            jy = (k % 9) / 3;
            jx = k % 3;
        } else if (lane == 52) {
            u = kStall;
        }
        const int dx = delta_x(u), dy = delta_y(u);
        for (int t = a - 1; t >= 0; --t) {
            int px = -1, py = -1;
            if (u >= 0) {
                px = axis_source(cx, dx, jx, 2, L - 3);
                py = axis_source(cy, dy, jy, 2, W - 3);
            }
            bool ok = false;
            if (px >= 0 && py >= 0) ok = (levels[t * W + py] >> px) & 1ull;
            const u64 m = __ballot(ok);
            const int win = m ? __ffsll((long long)m) - 1 : 52;   // never empty: level t + 1 was built from level t
            cx = __shfl(px, win);
            cy = __shfl(py, win);
            if (lane == 0) path[t * n + slot] = pack_xy(cx, cy);
        }
    }

    static __device__ int action(int p0, int p1, int gx, int gy, int W, int L) {
        const int x0 = p0 & 255, y0 = p0 >> 8, x1 = p1 & 255, y1 = p1 >> 8;
        int u = kStall;   // inside the goal disc (the snap) or done
        if ((x0 - gx) * (x0 - gx) + (y0 - gy) * (y0 - gy) >= 16) {
            // the walked action is the lowest one that takes p0 to p1: a lower one would have won the walk back
            for (int v = kStall - 1; v >= 0; --v) {
                int mx = x0 + delta_x(v), my = y0 + delta_y(v);
                mx = mx < 2 ? 2 : (mx > L - 3 ? L - 3 : mx);
                my = my < 2 ? 2 : (my > W - 3 ? W - 3 : my);
                if (mx == x1 && my == y1) u = v;
            }
        }
        return u;
    }
};

// The blocked row of this lane: centres out of range, or whose 5x5 box touches an avoided cell.  `wide` [W] in LDS takes the
// avoided cells of every row, widened by 2 in x.
__device__ inline u64 meda_blocked_row(u64 *wide, const uint8_t *__restrict__ avoid, size_t b, int W, int L, int lane) {
    if (lane < W) {
        u64 a = 0;
        if (avoid) {
            const uint8_t *row = avoid + (b * W + lane) * L;
            for (int x = 0; x < L; ++x) a |= row[x] ? (1ull << x) : 0ull;
        }
        wide[lane] = a | (a << 1) | (a << 2) | (a >> 1) | (a >> 2);
    }
    __syncthreads();
    u64 blocked = ~0ull;
    if (lane >= 2 && lane <= W - 3) {
        u64 m = 0;
        for (int dy = -2; dy <= 2; ++dy) m |= wide[lane + dy];
        blocked = m | ~run(2, L - 3);
    }
    return blocked;
}

// The open-loop planner of a MEDA geometry, one task per workgroup: meda_plan.hip instantiates it for the plain rule, meda_follow.hip
// for the safe one.
template <class Geo>
__global__ __launch_bounds__(kWave) void k_meda_plan(int W, int L, int n, const int32_t *__restrict__ starts, const int32_t *__restrict__ goals,
                                                     uint8_t *__restrict__ route, int8_t *__restrict__ act, int32_t *__restrict__ steps,
                                                     uint8_t *__restrict__ success, int32_t *__restrict__ attempt, int32_t *__restrict__ lower,
                                                     const uint8_t *__restrict__ avoid) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int T = Geo::limit(W, L);
    u64 *wide = (u64 *)smem;   // [W]: the avoided cells of a row, widened by 2 in x; the levels [T - 2][W] follow
    const u64 blocked = meda_blocked_row(wide, avoid, blockIdx.x, W, L, threadIdx.x);
    plan_task<Geo>(blockIdx.x, W, L, T, n, blocked, wide + W, (unsigned short *)(smem + (size_t)(T - 1) * W * 8),
                   {starts, goals, route, act, steps, success, attempt, lower}, 0, 0);   // no reservations, no retries
}

}  // namespace
