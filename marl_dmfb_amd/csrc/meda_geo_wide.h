// meda_geo_wide.h -- the MEDA geometry of meda_geo.h for chips up to 128 x 128: what meda_plan_wide.hip (the open-loop planner) and
// meda_follow_wide.hip (the closed loop) both compile, and the host-side sizes of their launches.
//
// One workgroup of ONE wave per task; lane i owns the chip rows i (`a`) and i + 64 (`b`), each as two 64-bit words (Row128: bit x
// of `lo` for x < 64, bit x - 64 of `hi`).  The level of meda_geo.h is computed on both rows of a lane: the rows 1, 2 and 3 below
// and above come from a wrapped wave shuffle and a select at the row-63 / row-64 seam, the column moves carry their bits across
// the word seam, and the clamp folds are 128-bit runs.  The first H `src` levels go to LDS and the levels from H on to the
// workgroup's slice of a global workspace (WideLevels); the walk back is the one of meda_geo.h, its bit tests reading either.
//
// Include it after hip_abi.h, plan_core.h and meda_geo.h.
#pragma once

namespace {

struct alignas(16) Row128 {
    u64 lo, hi;
};
__device__ inline Row128 operator|(Row128 x, Row128 y) { return {x.lo | y.lo, x.hi | y.hi}; }
__device__ inline Row128 operator&(Row128 x, Row128 y) { return {x.lo & y.lo, x.hi & y.hi}; }
__device__ inline Row128 operator~(Row128 x) { return {~x.lo, ~x.hi}; }
__device__ inline bool any(Row128 x) { return (x.lo | x.hi) != 0; }
__device__ inline Row128 when(bool c, Row128 x) { return {c ? x.lo : 0ull, c ? x.hi : 0ull}; }
__device__ inline Row128 bit128(int x) { return {x < 64 ? 1ull << x : 0ull, x < 64 ? 0ull : 1ull << (x - 64)}; }
__device__ inline bool test128(Row128 w, int x) { return ((x < 64 ? w.lo >> x : w.hi >> (x - 64)) & 1ull) != 0; }
// Bits lo .. hi, clipped to 0 .. 127.
__device__ inline Row128 run128(int lo, int hi) { return {run(lo, hi), run(lo - 64, hi - 64)}; }
// Shifts by k = 1 .. 3 columns.
__device__ inline Row128 shl128(Row128 w, int k) { return {w.lo << k, (w.hi << k) | (w.lo >> (64 - k))}; }
__device__ inline Row128 shr128(Row128 w, int k) { return {(w.lo >> k) | (w.hi << (64 - k)), w.hi >> k}; }
__device__ inline Row128 shfl128(Row128 w, int src) { return {__shfl(w.lo, src), __shfl(w.hi, src)}; }

// The two rows of a lane.
struct Rows {
    Row128 a, b;
};
__device__ inline Rows operator|(Rows x, Rows y) { return {x.a | y.a, x.b | y.b}; }
__device__ inline Rows operator&(Rows x, Rows y) { return {x.a & y.a, x.b & y.b}; }
__device__ inline Rows operator~(Rows x) { return {~x.a, ~x.b}; }
__device__ inline Rows &operator|=(Rows &x, Rows y) { return x = x | y; }
__device__ inline bool any(Rows x) { return any(x.a | x.b); }

// The rows k = 1 .. 3 below (y + k) and above (y - k) the two rows of a lane; rows off the 128 are empty.
__device__ inline Rows rows_down(Rows v, int k, int lane) {
    const int from = (lane + k) & (kWave - 1);
    const Row128 sa = shfl128(v.a, from), sb = shfl128(v.b, from);
    const bool same = lane + k < kWave;
    return {same ? sa : sb, when(same, sb)};
}
__device__ inline Rows rows_up(Rows v, int k, int lane) {
    const int from = (lane - k) & (kWave - 1);
    const Row128 sa = shfl128(v.a, from), sb = shfl128(v.b, from);
    const bool same = lane >= k;
    return {when(same, sa), same ? sb : sa};
}

// The column moves of a row with their clamp folds; xh = length - 3.  The fold bits are taken before the shift.
__device__ inline Row128 east128(Row128 w, int k, int xh) {
    const bool fold = any(w & run128(xh - k + 1, xh));
    return (shl128(w, k) & run128(2, xh)) | when(fold, bit128(xh));
}
__device__ inline Row128 west128(Row128 w, int k, int xh) {
    const bool fold = (w.lo & run(2, 2 + k - 1)) != 0;
    return (shr128(w, k) & run128(2, xh)) | when(fold, Row128{4ull, 0ull});
}

// The `src` levels of the droplet in flight: the levels 0 .. H-1 in LDS, the levels from H on in the workgroup's workspace slice;
// a level is W rows.
struct WideLevels {
    Row128 *lds, *work;
    int H;
};
// The two memories are named to the compiler, so that a level is read and written with LDS or global instructions, never through
// a pointer that may be either.
typedef __attribute__((address_space(3))) u64 lds_u64;
typedef __attribute__((address_space(1))) u64 global_u64;
__device__ inline void put_level(const WideLevels &lv, int t, int W, int row, Row128 v) {   // t is the same in all lanes
    if (t < lv.H) {
        lds_u64 *p = (lds_u64 *)(lv.lds + (t * W + row));
        p[0] = v.lo;
        p[1] = v.hi;
    } else {
        global_u64 *p = (global_u64 *)(lv.work + ((size_t)(t - lv.H) * W + row));
        p[0] = v.lo;
        p[1] = v.hi;
    }
}
__device__ inline Row128 get_level(const WideLevels &lv, int t, int W, int row) {
    if (t < lv.H) {
        const lds_u64 *p = (const lds_u64 *)(lv.lds + (t * W + row));
        return {p[0], p[1]};
    }
    const global_u64 *p = (const global_u64 *)(lv.work + ((size_t)(t - lv.H) * W + row));
    return {p[0], p[1]};
}

template <bool SAFE, class Abi> struct MedaWide : Meda<SAFE, Abi> {
    typedef Meda<SAFE, Abi> Narrow;   // limit, check_sizes, dist, near_goal, action and the constants are its own

    static __device__ Row128 goal_row(int row, int gx, int gy) {
        int d = row - gy;
        d = d < 0 ? -d : d;
        if (d > 3) return {0ull, 0ull};
        return run128(gx - (d == 3 ? 2 : 3), gx + (d == 3 ? 2 : 3));
    }

    static __device__ Row128 near_row128(int row, int px, int py) {
        int d = row - py;
        d = d < 0 ? -d : d;
        if (d > 5) return {0ull, 0ull};
        const int hw = d <= 3 ? 5 : (d == 4 ? 4 : 3);
        return run128(px - hw, px + hw);
    }

    // The rows `lane` and `lane + 64` of near((px, py)).
    static __device__ Rows near_row(int lane, int px, int py) { return {near_row128(lane, px, py), near_row128(lane + kWave, px, py)}; }

    // One row of a level: `src` and the rows 1 .. 3 below (d) and above (u) it -> the row of the union of the nine moves.
    static __device__ Row128 moves(Row128 src, Row128 d1, Row128 d2, Row128 d3, Row128 u1, Row128 u2, Row128 u3, bool top, bool bottom,
                                   int xh) {
        const Row128 n3 = d3 | when(top, src | d1 | d2);      // rows moved by (0, -3), the clamp folded into row 2
        const Row128 n2 = d2 | when(top, src | d1);
        const Row128 s3 = u3 | when(bottom, src | u1 | u2);   // rows moved by (0, +3), folded into row width-3
        const Row128 s2 = u2 | when(bottom, src | u1);
        const Row128 diag = n2 | s2;
        return src | n3 | s3 | east128(src, 3, xh) | west128(src, 3, xh) | east128(diag, 2, xh) | west128(diag, 2, xh);
    }

    // Every value that decides a branch is the same in all lanes.
    template <bool STORE>
    static __device__ int forward(int lane, int W, int L, int T, int n, int sx, int sy, int gx, int gy, Rows blocked,
                                  const unsigned short *path, int np, const WideLevels &levels, ReservedRows<Rows>) {   // nothing reserved
        const int xh = L - 3, yh = W - 3;
        const int last_bad = last_bad_level<Narrow>(path, T, n, np, lane, gx, gy);
        const Rows G = {goal_row(lane, gx, gy), goal_row(lane + kWave, gx, gy)};
        Rows reach = {when(lane == sy, bit128(sx)), when(lane + kWave == sy, bit128(sx))};
        Rows nprev = {};   // N[t]; the plain rule has no such guard
        if (SAFE) nprev = near_union_row<MedaWide>(path, np, lane);
        const bool top = lane == 2, bottom_a = lane == yh, bottom_b = lane + kWave == yh;
        for (int t = 0; t <= T - 2; ++t) {
            const Rows arr = reach & G;   // reach[t] lies outside F[t] already (t >= 1), and the plain F[0] is empty
            if (t + (SAFE ? 0 : 1) > last_bad) {   // hold[t + 1]; safe: the goal is clear before the snap step too
                const u64 in_a = __ballot(any(arr.a));
                const u64 in_b = in_a ? 0ull : __ballot(any(arr.b));
                if (in_a | in_b) {   // the lowest (y, x): the rows 0 .. 63 come first
                    const int from = __ffsll((long long)(in_a ? in_a : in_b)) - 1;
                    const Row128 w = shfl128(in_a ? arr.a : arr.b, from);
                    const int x = w.lo ? __ffsll((long long)w.lo) - 1 : __ffsll((long long)w.hi) + 63;
                    return t | (x << 8) | ((from + (in_a ? 0 : kWave)) << 16);
                }
            }
            if (t == T - 2) break;
            Rows next = {};   // F[t+1]
            if (SAFE) next = near_union_row<MedaWide>(path + (t + 1) * n, np, lane);
            const Rows src = reach & ~G & ~next;
            if (STORE) {
                if (lane < W) put_level(levels, t, W, lane, src.a);
                if (lane + kWave < W) put_level(levels, t, W, lane + kWave, src.b);
            }
            if (!__any(any(src))) return -1;
            const Rows d1 = rows_down(src, 1, lane), d2 = rows_down(src, 2, lane), d3 = rows_down(src, 3, lane);
            const Rows u1 = rows_up(src, 1, lane), u2 = rows_up(src, 2, lane), u3 = rows_up(src, 3, lane);
            Rows nr = {moves(src.a, d1.a, d2.a, d3.a, u1.a, u2.a, u3.a, top, bottom_a, xh),
                       moves(src.b, d1.b, d2.b, d3.b, u1.b, u2.b, u3.b, false, bottom_b, xh)};
            if (!SAFE) next = near_union_row<MedaWide>(path + (t + 1) * n, np, lane);
            nr = nr & ~blocked & ~next & ~nprev;
            reach = nr;
            if (SAFE) nprev = next;
        }
        return -1;
    }

    static __device__ void walk_back(int lane, int W, int L, int n, int slot, int r, int gx, int gy, const WideLevels &levels,
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
            if (px >= 0 && py >= 0) ok = test128(get_level(levels, t, W, py), px);
            const u64 m = __ballot(ok);
            const int win = m ? __ffsll((long long)m) - 1 : 52;   // never empty: level t + 1 was built from level t
            cx = __shfl(px, win);
            cy = __shfl(py, win);
            if (lane == 0) path[t * n + slot] = pack_xy(cx, cy);
        }
    }
};

// The blocked rows of this lane: centres out of range, or whose 5x5 box touches an avoided cell.  `wide` [W] in LDS takes the
// avoided cells of every row, widened by 2 in x.
__device__ inline Rows meda_blocked_rows(Row128 *wide, const uint8_t *__restrict__ avoid, size_t b, int W, int L, int lane) {
    for (int y = lane; y < W; y += kWave) {
        Row128 a = {0ull, 0ull};
        if (avoid) {
            const uint8_t *row = avoid + (b * W + y) * L;
            for (int x = 0; x < L; ++x) {
                const u64 bit = row[x] ? (1ull << (x & 63)) : 0ull;
                if (x < 64) a.lo |= bit; else a.hi |= bit;
            }
        }
        wide[y] = a | shl128(a, 1) | shl128(a, 2) | shr128(a, 1) | shr128(a, 2);
    }
    __syncthreads();
    const Row128 all = {~0ull, ~0ull};
    Rows blocked = {all, all};
    const Row128 off = ~run128(2, L - 3);
    if (lane >= 2 && lane <= W - 3) {
        Row128 m = off;
        for (int dy = -2; dy <= 2; ++dy) m = m | wide[lane + dy];
        blocked.a = m;
    }
    if (lane + kWave <= W - 3) {
        Row128 m = off;
        for (int dy = -2; dy <= 2; ++dy) m = m | wide[lane + kWave + dy];
        blocked.b = m;
    }
    return blocked;
}

// ---------------------------------------------------------------------------------------------------- host side
// The sizes of a launch, for the open-loop planner (meda_plan_wide.hip) and the closed loop (meda_follow_wide.hip) alike: both keep
// the avoid rows [W], the levels [H][W] and the paths in LDS and the other levels in one workspace slice per workgroup.
constexpr int kWideMaxGroups = 512;   // *_MAX_GROUPS of both public headers

inline int wide_limit(int width, int length) { return width + length; }   // Meda::limit

inline size_t path_bytes(int T, int n_agents) { return ((size_t)(T + 1) * n_agents * 2 + 15) & ~(size_t)15; }

// H of checked sizes: what the budget holds beside the avoid rows and the paths, at most the T - 2 levels there are and at most
// `cap` when that is positive.
inline int levels_in_lds(int width, int length, int n_agents, int cap) {
    const int T = wide_limit(width, length);
    const size_t row = (size_t)width * sizeof(Row128);
    const size_t fit = (kLdsBudget - path_bytes(T, n_agents) - row) / row;
    int H = fit < (size_t)(T - 2) ? (int)fit : T - 2;
    if (cap > 0 && cap < H) H = cap;
    return H;
}

inline size_t lds_bytes_wide(int width, int length, int n_agents, int H) {
    return (size_t)(H + 1) * width * sizeof(Row128) + path_bytes(wide_limit(width, length), n_agents);
}

inline int groups_of(int n_tasks) { return n_tasks < kWideMaxGroups ? n_tasks : kWideMaxGroups; }

// The bytes of one workgroup's workspace slice.
inline size_t slice_bytes(int width, int length, int H) { return (size_t)(wide_limit(width, length) - 2 - H) * width * sizeof(Row128); }

}  // namespace
