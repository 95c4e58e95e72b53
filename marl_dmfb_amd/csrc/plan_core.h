// plan_core.h -- the prioritized space-time planning procedure of route_plan.hip (DMFB) and meda_plan.hip (MEDA), stated once.
//
// One workgroup of ONE wave per task; a lane owns one chip row as a 64-bit word (the wide MEDA planner, meda_geo_wide.h: two rows of
// two words each; the procedure is stated over the geometry's row type and over what holds its levels).  The droplets are ranked by descending distance
// start -> goal (ties by ascending index); every droplet is planned alone for the lower bound; attempt k = 0 .. n-1 plans them in
// that order rotated left by k, each against the paths of those planned before it, and the first attempt that routes them all is
// kept.  Two opt-in parameters (DMFB only, MEDA passes 0 / 0): with `reserve` = R > 0 the droplets not yet
// planned in the attempt keep near(start) for the levels 1 .. R, and with `retries` = Q > 0 up to Q further attempts n .. n+Q-1
// follow the rotations, each with the first droplet that got no path moved to the front.  The dynamic LDS of a task is (T - 1) * W row words (the `src` rows of the levels, after any rows the geometry keeps for
// itself) and then the planned paths [T + 1][n] in planning order (slot p = the p-th droplet of the attempt).
//
// Include it after hip_abi.h.  The including file then defines the geometry, a type Geo with
//   kMaxAgents, kBadArg, kUnsupported      the droplet limit and the return codes of its public header
//   kFirstLevel                            the first level at which a planned droplet forbids cells (0 DMFB, 1 MEDA)
//   kStepsAfterArrival                     steps = arrival level + this (0 DMFB, 1 MEDA: the snap step)
//   limit(W, L)                            T, the episode limit
//   check_sizes(width, length, n_agents)   0 or a return code
//   dist(sx, sy, gx, gy)                   the priority key
//   near_row(row, px, py)                  row `row` of near((px, py)): the geometry's row type (u64; zero-initialised by {},
//                                          joined by |=), which `blocked` and the reservations have too
//   near_goal(dx, dy)                      is a droplet at goal + (dx, dy) near the goal?
//   forward<STORE>(lane, W, L, T, n, sx, sy, gx, gy, blocked, path, np, levels, res)
//                                          the search of one droplet against the first np slots: -1, or its arrival level in the
//                                          low 8 bits (MEDA adds the arrival cell, x << 8 | y << 16; DMFB arrives on the goal);
//                                          STORE keeps level t's `src` in levels[t * W + row]; res: the reservations (Reserved).
//                                          `levels` is passed through to forward and walk_back as the kernel gave it (u64 *)
//   walk_back(lane, W, L, n, slot, r, gx, gy, levels, path)
//                                          what forward returned as r: levels a .. 0 of the path into slot `slot`
//   action(p0, p1, gx, gy, W, L)           the action that took the packed position p0 to p1
// and, for the closed loop (follow_chip),
//   kParkMin                               the smallest distance to its goal at which a droplet may be parked
//   kMissingAction                         what a droplet plays where its plan has no action (the geometry's STALL)
#pragma once

namespace {

typedef unsigned long long u64;
constexpr int kWave = 64;
constexpr int kMaxN = 16;                          // the length of the shared task arrays
constexpr size_t kLdsBudget = 160 * 1024 - 1024;   // a workgroup may hold all 160 KiB; 1 KiB stays for the static arrays

// The arrays of a task, as the public headers describe them.
struct PlanIO {
    const int32_t *starts, *goals;
    uint8_t *route;
    int8_t *act;
    int32_t *steps;
    uint8_t *success;
    int32_t *attempt, *lower;
};

__device__ inline unsigned short pack_xy(int x, int y) { return (unsigned short)(x | (y << 8)); }

// Bits lo .. hi of a word, clipped to 0 .. 63.
__device__ inline u64 run(int lo, int hi) {
    lo = lo < 0 ? 0 : lo;
    hi = hi > 63 ? 63 : hi;
    return lo > hi ? 0ull : ((~0ull << lo) & (~0ull >> (63 - hi)));
}

// Row `lane` of the union of near() over the planned slots at one level: path_t = the positions of the `np` slots at that level.
template <class Geo> __device__ inline auto near_union_row(const unsigned short *path_t, int np, int lane) {
    decltype(Geo::near_row(0, 0, 0)) m = {};
    for (int q = 0; q < np; ++q) {
        const int p = path_t[q];
        m |= Geo::near_row(lane, p & 255, p >> 8);
    }
    return m;
}

// The last level whose near-union holds the goal, kFirstLevel - 1 if none does: hold[a] is a > last_bad.
template <class Geo> __device__ inline int last_bad_level(const unsigned short *path, int T, int n, int np, int lane, int gx, int gy) {
    int last_bad = Geo::kFirstLevel - 1;
    for (int t = Geo::kFirstLevel + lane; t <= T; t += kWave) {
        const unsigned short *pt = path + t * n;
        for (int q = 0; q < np; ++q) {
            const int p = pt[q];
            if (Geo::near_goal((p & 255) - gx, (p >> 8) - gy)) last_bad = t;
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const int o = __shfl_xor(last_bad, off);
        last_bad = o > last_bad ? o : last_bad;
    }
    return last_bad;
}

// What the droplets not yet planned in an attempt keep for themselves: `row` = this lane's row of the union of near(start) over
// them, forbidden at the levels 1 .. `levels` (0: nothing is reserved).
template <class Row> struct ReservedRows {
    Row row;
    int levels;
};
typedef ReservedRows<u64> Reserved;

// The droplets of the task in flight, in static LDS: starts, goals, the priority key, rank[i] = the place of droplet i in the base
// order and order[r] = the droplet at place r; of the attempt in flight, plan[p] = the droplet planned p-th (it takes slot p of
// the paths) and slot[i] = the place of droplet i.
struct TaskLds {
    int sx[kMaxN], sy[kMaxN], gx[kMaxN], gy[kMaxN], dist[kMaxN], rank[kMaxN], order[kMaxN];
    unsigned char plan[kMaxN], slot[kMaxN];
};

// The base order of the starts and goals lanes < n wrote into `s`: descending distance, ties by ascending index.
template <class Geo> __device__ inline void rank_task(TaskLds &s, int n, int lane) {
    if (lane < n) s.dist[lane] = Geo::dist(s.sx[lane], s.sy[lane], s.gx[lane], s.gy[lane]);
    __syncthreads();
    if (lane < n) {
        int r = 0;
        for (int j = 0; j < n; ++j) r += s.dist[j] > s.dist[lane] || (s.dist[j] == s.dist[lane] && j < lane);
        s.rank[lane] = r;
        s.order[r] = lane;
    }
    __syncthreads();
}

// The lower bound: every droplet alone; -1 if one of them cannot arrive.
template <class Geo, class Row, class Levels>
__device__ inline int lower_bound(const TaskLds &s, int lane, int W, int L, int T, int n, Row blocked, Levels levels, unsigned short *path) {
    int lb = 0;
    for (int i = 0; i < n; ++i) {
        const int r = Geo::template forward<false>(lane, W, L, T, n, s.sx[i], s.sy[i], s.gx[i], s.gy[i], blocked, path, 0, levels,
                                                   ReservedRows<Row>{Row{}, 0});
        const int a = r < 0 ? -1 : (r & 255) + Geo::kStepsAfterArrival;
        lb = (a < 0 || lb < 0) ? -1 : (a > lb ? a : lb);
    }
    return lb;
}

// The attempts: k = 0 .. n-1 plan the base order rotated left by k; if they all fail, k = n + r (r = 0 .. Q-1) plans order O_r, where
// O_0 is the base order with the first droplet that got no path in attempt 0 moved to the front and O_{r+1} is O_r with the first
// droplet that got no path in it moved to the front (the retries end when that droplet is at the front already).  While the
// droplet at place p is searched, those at the places after it reserve near(start) for the levels 1 .. R.  Returns the attempt
// that routed every droplet (its paths are then in `path`, its order in s.plan / s.slot, its steps in *steps), or -1.
template <class Geo, class Row, class Levels>
__device__ inline int attempts(TaskLds &s, int lane, int W, int L, int T, int n, Row blocked, Levels levels, unsigned short *path, int R,
                               int Q, int *steps) {
    int kept = -1;
    *steps = 0;
    int failed = 0, failed0 = 0;   // the place of the first droplet without a path: in the last attempt, in attempt 0
    for (int k = 0; k < n + Q && kept < 0; ++k) {
        if (k > n && failed == 0) break;   // O_{r+1} == O_r
        int mine = 0;
        if (lane < n) {
            if (k < n) {
                mine = s.order[(lane + k) % n];
            } else {   // the droplet at place f of the order before moves to the front; O_0 starts from the base order
                const int f = k == n ? failed0 : failed;
                const int from = lane == 0 ? f : (lane <= f ? lane - 1 : lane);
                mine = k == n ? s.order[from] : s.plan[from];
            }
        }
        __syncthreads();   // every lane has read the order before
        if (lane < n) { s.plan[lane] = (unsigned char)mine; s.slot[mine] = (unsigned char)lane; }
        __syncthreads();
        int st = 0, p = 0;
        for (; p < n; ++p) {
            const int i = s.plan[p];
            const int gx = s.gx[i], gy = s.gy[i];
            ReservedRows<Row> res = {Row{}, R < T ? R : T};
            if (R > 0)
                for (int q = p + 1; q < n; ++q) res.row |= Geo::near_row(lane, s.sx[s.plan[q]], s.sy[s.plan[q]]);
            const int r = Geo::template forward<true>(lane, W, L, T, n, s.sx[i], s.sy[i], gx, gy, blocked, path, p, levels, res);
            if (r < 0) break;
            const int a = r & 255;
            __syncthreads();   // the levels are complete before any lane reads another lane's rows
            Geo::walk_back(lane, W, L, n, p, r, gx, gy, levels, path);
            for (int t = a + 1 + lane; t <= T; t += kWave) path[t * n + p] = pack_xy(gx, gy);   // on its goal from then on
            __syncthreads();   // the path is complete before the next droplet plans against it
            st = a + Geo::kStepsAfterArrival > st ? a + Geo::kStepsAfterArrival : st;
        }
        if (p == n) { kept = k; *steps = st; }
        failed = p;
        if (k == 0) failed0 = p;
    }
    __syncthreads();
    return kept;
}

// The slot of droplet i in the paths of the kept attempt.
__device__ inline int slot_of(const TaskLds &s, int i) { return s.slot[i]; }

// The routes [T+1][n] (16 bits = the (x, y) bytes of one droplet) and actions [T][n] of one task, in droplet order: the kept
// attempt's, or the starts and -1 when kept < 0.
template <class Geo>
__device__ inline void write_route(const TaskLds &s, int lane, int W, int L, int T, int n, int kept, int steps, const unsigned short *path,
                                   unsigned short *route16, int8_t *u_out) {
    for (int idx = lane; idx < (T + 1) * n; idx += kWave) {
        const int t = idx / n, i = idx - t * n;
        route16[idx] = kept >= 0 ? path[t * n + slot_of(s, i)] : pack_xy(s.sx[i], s.sy[i]);
    }
    for (int idx = lane; idx < T * n; idx += kWave) {
        const int t = idx / n, i = idx - t * n;
        int u = -1;
        if (kept >= 0 && t < steps) {
            const int slot = slot_of(s, i);
            u = Geo::action(path[t * n + slot], path[(t + 1) * n + slot], s.gx[i], s.gy[i], W, L);
        }
        u_out[idx] = (int8_t)u;
    }
}

// What a chip keeps between the lock-steps of a followed episode (include/route_plan.h: route_follow_dmfb, include/meda_follow.h:
// meda_follow_step).
struct FollowState {
    uint8_t *route;     // the kept plan
    int8_t *route_u;
    int32_t *cursor;
    uint8_t *partial;
    int32_t *replans;
    uint8_t *gave_up, *active;
    int32_t *steps, *lower, *actions;
    int8_t *u;
};

// Lock-step t of the closed loop for chip `b`, which is active and has not ended: `pos` is the packed position
// of droplet `lane` now, (gx, gy) its goal.  A chip that is where its kept plan says costs one compare and one copy; any other is
// replanned from where it is, parking the droplets nearest their goals (ascending distance >= kParkMin, ties by descending index)
// until the rest can be routed; every plan is made with R / Q of `attempts`.  `blocked_row()` gives this lane's blocked row and is called on a replan only (by every lane: it
// may synchronise the workgroup); its result is the geometry's row type, `levels` what holds the geometry's levels.  Every return
// is taken by all lanes.  A workgroup that walks several chips puts a barrier between two calls: the static LDS here is reused.
template <class Geo, class Levels, class Blocked>
__device__ inline void follow_chip(size_t b, int W, int L, int T, int n, int t, int pos, int gx, int gy, const FollowState &st,
                                   Levels levels, unsigned short *path, int R, int Q, Blocked blocked_row) {
    __shared__ TaskLds s;
    __shared__ int s_d[kMaxN];
    const int lane = threadIdx.x;
    const int px = pos & 255, py = pos >> 8;
    int8_t *u_now = st.u + (b * T + t) * n;
    int32_t *act_now = st.actions + b * n;

    const int cursor = st.cursor[b];
    if (cursor >= 0 && cursor < T && !st.partial[b]) {
        const int planned = lane < n ? ((const unsigned short *)st.route)[(b * (T + 1) + cursor) * n + lane] : 0;
        if (!__any(planned != pos)) {   // on the plan: play its next actions
            if (lane < n) {
                const int u = st.route_u[(b * T + cursor) * n + lane];
                act_now[lane] = u < 0 ? Geo::kMissingAction : u;
                u_now[lane] = (int8_t)(u < 0 ? Geo::kMissingAction : u);
            }
            if (lane == 0) { st.cursor[b] = cursor + 1; st.steps[b] += 1; }
            return;
        }
    }

    const auto blocked = blocked_row();
    const int d = Geo::dist(px, py, gx, gy);
    const bool away = lane < n && d >= Geo::kParkMin;
    if (lane < n) { s.sx[lane] = px; s.sy[lane] = py; s_d[lane] = d; }
    __syncthreads();
    int place = 0;   // in the park order
    for (int j = 0; j < n; ++j) place += s_d[j] >= Geo::kParkMin && (s_d[j] < d || (s_d[j] == d && j > lane));
    const int n_away = __popcll(__ballot(away));
    int kept = -1, steps = 0, k = 0;
    for (; k < (n_away > 1 ? n_away : 1); ++k) {
        const bool parked = away && place < k;
        if (lane < n) { s.gx[lane] = parked ? px : gx; s.gy[lane] = parked ? py : gy; }
        rank_task<Geo>(s, n, lane);
        if (t == 0 && k == 0) {
            const int lb = lower_bound<Geo>(s, lane, W, L, T, n, blocked, levels, path);
            if (lane == 0) st.lower[b] = lb;
        }
        kept = attempts<Geo>(s, lane, W, L, T, n, blocked, levels, path, R, Q, &steps);
        if (kept >= 0) break;
    }
    if (kept < 0) {
        if (lane == 0) { st.gave_up[b] = 1; st.active[b] = 0; }
        return;
    }
    write_route<Geo>(s, lane, W, L, T, n, kept, steps, path, (unsigned short *)st.route + b * (size_t)(T + 1) * n,
                     st.route_u + b * (size_t)T * n);
    if (lane < n) {
        const int slot = slot_of(s, lane);
        const int u = steps > 0 ? Geo::action(path[slot], path[n + slot], s.gx[lane], s.gy[lane], W, L) : Geo::kMissingAction;
        act_now[lane] = u;
        u_now[lane] = (int8_t)u;
    }
    if (lane == 0) {
        st.cursor[b] = 1;
        st.partial[b] = k > 0;
        st.replans[b] += 1;
        st.steps[b] += 1;
    }
}

// Task b: `blocked` is this lane's row of cells no droplet may enter, `levels` and `path` the two parts of the dynamic LDS, R / Q
// the reservation levels and retries of `attempts`.
template <class Geo, class Row, class Levels>
__device__ inline void plan_task(size_t b, int W, int L, int T, int n, Row blocked, Levels levels, unsigned short *path, const PlanIO &io,
                                 int R, int Q) {
    static_assert(Geo::kMaxAgents <= kMaxN, "the shared task arrays hold kMaxN droplets");
    __shared__ TaskLds s;
    const int lane = threadIdx.x;

    if (lane < n) {
        const int32_t *st = io.starts + (b * n + lane) * 2, *g = io.goals + (b * n + lane) * 2;
        s.sx[lane] = st[0]; s.sy[lane] = st[1]; s.gx[lane] = g[0]; s.gy[lane] = g[1];
    }
    rank_task<Geo>(s, n, lane);
    const int lb = lower_bound<Geo>(s, lane, W, L, T, n, blocked, levels, path);
    // a droplet that cannot arrive alone arrives in no attempt: the reach sets only shrink with more planned paths
    int kept = -1, steps = 0;
    if (lb >= 0) kept = attempts<Geo>(s, lane, W, L, T, n, blocked, levels, path, R, Q, &steps);
    __syncthreads();

    if (lane == 0) {
        io.steps[b] = steps;
        io.success[b] = kept >= 0;
        io.attempt[b] = kept;
        io.lower[b] = lb;
    }
    write_route<Geo>(s, lane, W, L, T, n, kept, steps, path, (unsigned short *)io.route + b * (size_t)(T + 1) * n,
                     io.act + b * (size_t)T * n);
}

// ---------------------------------------------------------------------------------------------------- host side
inline size_t lds_bytes(size_t T, int width, int n_agents) {
    return (T - 1) * (size_t)width * 8 + (((T + 1) * (size_t)n_agents * 2 + 15) & ~(size_t)15);
}

// One workgroup per task with the LDS of its sizes: the end of launch_plan and launch_follow, after their checks.
template <class Geo, class Kernel, class... Args>
int launch_tasks(Kernel kernel, int n_tasks, int width, int length, int n_agents, void *stream, Args... args) {
    const size_t lds = lds_bytes(Geo::limit(width, length), width, n_agents);
    if (lds > kLdsBudget) return Geo::kUnsupported;
    if (n_tasks == 0) return 0;
    static LdsLimit lds_limit;   // one per kernel: the kernels of a library differ in their signatures
    if (lds > 64 * 1024)
        if (const int rc = lds_limit.raise((const void *)kernel, kLdsBudget)) return rc;
    LAUNCH(kernel, dim3((unsigned)n_tasks), dim3(kWave), lds, (hipStream_t)stream, args...);
    return 0;
}

// The checks every planner entry point makes, then its kernel.  `more_ok`: the geometry's own pointer checks; `more`: what its
// kernel takes after (W, L, n, io).
template <class Geo, class Kernel, class... More>
int launch_plan(Kernel kernel, int n_tasks, int width, int length, int n_agents, const PlanIO &io, bool more_ok, void *stream,
                More... more) {
    if (n_tasks < 0) return Geo::kBadArg;
    if (const int rc = Geo::check_sizes(width, length, n_agents)) return rc;
    if (!io.starts || !io.goals || !io.route || !io.act || !io.steps || !io.success || !io.attempt || !io.lower || !more_ok)
        return Geo::kBadArg;
    return launch_tasks<Geo>(kernel, n_tasks, width, length, n_agents, stream, width, length, n_agents, io.starts, io.goals, io.route,
                             io.act, io.steps, io.success, io.attempt, io.lower, more...);
}

// The checks every follow entry point makes: 0 or a return code.  `more_ok`: the geometry's own pointer checks.
template <class Geo>
int check_follow(int n_tasks, int width, int length, int n_agents, int t, const int32_t *goals, const uint8_t *positions,
                 const FollowState &st, bool more_ok) {
    if (n_tasks < 0) return Geo::kBadArg;
    if (const int rc = Geo::check_sizes(width, length, n_agents)) return rc;
    if (t < 0 || t >= Geo::limit(width, length)) return Geo::kBadArg;
    if (!goals || !positions || !st.route || !st.route_u || !st.cursor || !st.partial || !st.replans || !st.gave_up || !st.active ||
        !st.steps || !st.lower || !st.actions || !st.u || !more_ok)
        return Geo::kBadArg;
    if (((uintptr_t)positions | (uintptr_t)st.route) & 1) return Geo::kBadArg;   // read and written 16 bits at a time
    return 0;
}

// Those checks, then one workgroup per chip.  `more`: what its kernel takes after (W, L, n, t, goals).
template <class Geo, class Kernel, class... More>
int launch_follow(Kernel kernel, int n_tasks, int width, int length, int n_agents, int t, const int32_t *goals, const uint8_t *positions,
                  const FollowState &st, bool more_ok, void *stream, More... more) {
    if (const int rc = check_follow<Geo>(n_tasks, width, length, n_agents, t, goals, positions, st, more_ok)) return rc;
    return launch_tasks<Geo>(kernel, n_tasks, width, length, n_agents, stream, width, length, n_agents, t, goals, more...);
}

}  // namespace
