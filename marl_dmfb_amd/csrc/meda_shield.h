// meda_shield.h -- the action shield of the vectorised MEDA environment (meda_vec_shield in include/meda_vec.h; the rule in
// numpy: marl_dmfb_amd/shield.py: meda_shield_reference, the argument: DESIGN.md section 10c).  Include after meda_kernels.h.
//
// One step with two centres closer than 6 (d^2 < 36) sets the chip's `failed` for good (calPunish, meda.py:321-330).  A droplet
// that is done or inside its goal disc (d^2 < 16) is FORCED: the env puts it on its goal whatever its action and without a
// failure draw.  Its anchor -- where it is after the step if it "does nothing" -- is its goal, a free droplet's is its centre.
// land_i(c) = g_i if c is inside droplet i's disc, else c: the anchor one step later of a droplet that reaches c.  In index
// order the shield replaces every pick of a free droplet whose target c, or land(c), is within 6 of another droplet's anchor or
// of the target / land of a droplet decided before it, by that droplet's best-Q action of which neither is.  After the step a
// droplet stands on its anchor or its target, and its next anchor is its anchor or its land; every such combination of a pair
// was tested, so no subset of failed moves (degraded electrodes) brings two centres within 6 and the next state is safe again.
//
// Layout (that of dmfb_shield.h): 16 lanes per chip (MEDA_MAX_AGENTS), four chips per wave; lane j keeps droplet j's anchor, its
// target and land once decided, and its nine candidates (4 bits each) in registers.  Droplet i's turn is one 16-lane broadcast
// of its packed word, a nine-bit hit mask per lane and an OR butterfly over the 16 lanes; lane i then walks its candidates.  No
// LDS, no scratch, no atomics: one lane per row writes the outputs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "shield_common.h"

namespace medak {

using shieldk::kShieldBlock;
using shieldk::kShieldLanes;
using shieldk::ShieldArgs;
constexpr int kMedaShieldActions = 9;  // 0 N, 1 E, 2 S, 3 W, 4 NE, 5 SE, 6 SW, 7 NW, 8 STALL (meda.py:23-32)
static_assert(MEDA_MAX_AGENTS <= kShieldLanes, "one lane per droplet slot");

// Droplet.move (meda.py:106-138) of centre (x, y): each axis clamped into its range on its own (meda_move of plan.py; the
// clamps leave a STALL where it is, since a centre never leaves [2, L - 3] x [2, W - 3])
__device__ __forceinline__ void meda_shield_target(int x, int y, int u, int W, int L, int &tx, int &ty) {
    const int r = 3;
    const int dx = (u == 1) * r - (u == 3) * r + ((u == 4) | (u == 5)) * (r - 1) - ((u == 6) | (u == 7)) * (r - 1);
    const int dy = (u == 2) * r - (u == 0) * r + ((u == 5) | (u == 6)) * (r - 1) - ((u == 4) | (u == 7)) * (r - 1);
    tx = min(max(x + dx, kR), L - 1 - kR);
    ty = min(max(y + dy, kR), W - 1 - kR);
}

__global__ __launch_bounds__(kShieldBlock) void k_meda_shield(MCfg c, MPtrs p, ShieldArgs a) {
    const int gid = (int)(blockIdx.x * kShieldBlock + threadIdx.x);
    const int e = gid / kShieldLanes, j = gid & (kShieldLanes - 1);
    if (e >= c.E) return;                    // the 16 lanes of a chip leave together
    if (a.active && !a.active[e]) return;
    const int n = c.n, E = c.E, W = c.W, L = c.L;
    const bool has = j < n;                  // lanes n .. 15 hold no droplet
    uint32_t mine = 0;                       // cx | cy << 8 | gx << 16 | gy << 24
    int pick = 0;
    bool forced = false;
    uint64_t seq = 0;                        // the nine candidates, four bits each, first candidate lowest
    if (has) {
        mine = p.st[(size_t)j * E + e];
        const uint32_t status = p.st[(size_t)n * E + e];
        const int ox = mine & 0xff, oy = (mine >> 8) & 0xff, gx = (mine >> 16) & 0xff, gy = (int)(mine >> 24);
        forced = ((status >> j) & 1u) || d2(ox, oy, gx, gy) < 16;
        const size_t row = (size_t)e * n + j;
        pick = a.actions[row];
        seq = shieldk::shield_candidates<kMedaShieldActions, 4, uint64_t>(a.q, row, pick);
    }
    const int ox = mine & 0xff, oy = (mine >> 8) & 0xff, gx = (mine >> 16) & 0xff, gy = (int)(mine >> 24);
    const int ax = forced ? gx : ox, ay = forced ? gy : oy;   // the anchor
    int nx = ax, ny = ay, lx = ax, ly = ay;  // target and land: a forced droplet's are its anchor
    int final_u = pick;
    bool bad = false;                        // no candidate of this droplet was safe
    const int grp = (int)((threadIdx.x & (kWave - 1)) / kShieldLanes) * kShieldLanes;
    const uint32_t fmask = (uint32_t)((__ballot(has && forced) >> grp) & 0xffffu);
    for (int i = 0; i < n; ++i) {            // in index order, as the env moves them
        if ((fmask >> i) & 1u) continue;     // a forced droplet keeps its pick (the 16 lanes of the chip agree)
        const uint32_t w = (uint32_t)__shfl((int)mine, i, kShieldLanes);
        const int ix = (int)(w & 0xff), iy = (int)((w >> 8) & 0xff), igx = (int)((w >> 16) & 0xff), igy = (int)(w >> 24);
        uint32_t hit = 0;                    // bit u: droplet i's target of action u, or its land, is within 6 of this lane's
        if (has && j != i) {
            const bool before = j < i;
            // a target inside i's disc lands on i's goal, anywhere else on itself: the goal is tested once per turn
            bool goal_near = d2(igx, igy, ax, ay) < 36;
            if (before) goal_near = goal_near || d2(igx, igy, nx, ny) < 36 || d2(igx, igy, lx, ly) < 36;
#pragma unroll
            for (int u = 0; u < kMedaShieldActions; ++u) {
                int tx, ty;
                meda_shield_target(ix, iy, u, W, L, tx, ty);
                bool near = d2(tx, ty, ax, ay) < 36 || (goal_near && d2(tx, ty, igx, igy) < 16);
                if (before) near = near || d2(tx, ty, nx, ny) < 36 || d2(tx, ty, lx, ly) < 36;
                hit |= (uint32_t)near << u;
            }
        }
#pragma unroll
        for (int d = kShieldLanes / 2; d >= 1; d >>= 1) hit |= (uint32_t)__shfl_xor((int)hit, d, kShieldLanes);
        if (j == i) {
            int take = -1;
#pragma unroll
            for (int k = kMedaShieldActions - 1; k >= 0; --k) {  // the first safe candidate wins
                const int u = (int)((seq >> (4 * k)) & 15u);
                if (!((hit >> u) & 1u)) take = u;
            }
            bad = take < 0;
            if (!bad) final_u = take;
            // an unsafe pre-state keeps the pick; a pick outside [0, 9) moves nothing (the env's step ignores it)
            if ((unsigned)final_u < (unsigned)kMedaShieldActions) meda_shield_target(ox, oy, final_u, W, L, nx, ny);
            const bool in = d2(nx, ny, gx, gy) < 16;
            lx = in ? gx : nx; ly = in ? gy : ny;
        }
    }
    shieldk::shield_write<kMedaShieldActions>(a, e, j, n, has, pick, final_u, bad);
}

}  // namespace medak
