// shield_common.h -- what the action shields of the two vectorised environments share (dmfb_shield.h, meda_shield.h): the launch
// shape, the arguments of the launch, the order of a droplet's candidate actions and the staging of the executed action.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace shieldk {

constexpr int kShieldLanes = 16;   // lanes per chip: one per droplet slot
constexpr int kShieldBlock = 256;  // 16 chips per workgroup
constexpr int kShieldWave = 64;

struct ShieldArgs {          // A = the env's action count
    const float *q;          // [E*n][A]
    const uint8_t *active;   // [E] or nullptr
    int32_t *actions;        // [E*n] in/out
    int8_t *last_onehot;     // [E*n][A]
    int8_t *ep_u;            // [E][T][n] or nullptr
    int8_t *ep_onehot;       // [E][T][n][A] or nullptr (given together with ep_u)
    int T, t;
    const int32_t *t_ep;     // [E] or nullptr
    int32_t *overrides;      // [E] or nullptr
    uint8_t *unsafe;         // [E] or nullptr
};

// float `>` with a NaN below every number (two NaNs are equal)
__device__ __forceinline__ bool shield_better(float a, float b) { return a > b || (a == a && b != b); }

// The candidates of row `row`, BITS bits each, first candidate lowest: the pick if it lies in [0, A), then the remaining actions
// by descending q, ties to the lower action, NaN last.
template <int A, int BITS, typename Word>
__device__ __forceinline__ Word shield_candidates(const float *q, size_t row, int pick) {
    static_assert(A <= (1 << BITS) && A * BITS <= (int)sizeof(Word) * 8, "the candidates do not fit the word");
    float qv[A];
#pragma unroll
    for (int u = 0; u < A; ++u) qv[u] = q[row * A + u];
    Word order = 0;
#pragma unroll
    for (int u = 0; u < A; ++u) {
        int rank = 0;
#pragma unroll
        for (int v = 0; v < A; ++v)
            if (v != u) rank += shield_better(qv[v], qv[u]) || (!shield_better(qv[u], qv[v]) && v < u);
        order |= (Word)u << (BITS * rank);
    }
    Word seq = 0;
    int cnt = 0;
    if ((unsigned)pick < (unsigned)A) { seq = (Word)pick; cnt = 1; }  // the pick comes first
#pragma unroll
    for (int r = 0; r < A; ++r) {
        const int u = (int)((order >> (BITS * r)) & (Word)((1 << BITS) - 1));
        if (u != pick) { seq |= (Word)u << (BITS * cnt); ++cnt; }
    }
    return seq;
}

// The end of a shield kernel, called by all 16 lanes of chip e: lane 0 adds the changed picks to overrides[e] and sets unsafe[e];
// lane j < n writes droplet j's executed action, its one-hot row and, when staged, its slot of the episode.
template <int A>
__device__ __forceinline__ void shield_write(const ShieldArgs &a, int e, int j, int n, bool has, int pick, int final_u, bool bad) {
    const int grp = (int)((threadIdx.x & (kShieldWave - 1)) / kShieldLanes) * kShieldLanes;
    const uint32_t changed = (uint32_t)((__ballot(has && final_u != pick) >> grp) & 0xffffu);
    const uint32_t anybad = (uint32_t)((__ballot(has && bad) >> grp) & 0xffffu);
    if (j == 0) {
        if (a.overrides && changed) a.overrides[e] += __popc(changed);
        if (a.unsafe && anybad) a.unsafe[e] = 1;
    }
    if (!has) return;
    const size_t row = (size_t)e * n + j;
    a.actions[row] = final_u;
#pragma unroll
    for (int u = 0; u < A; ++u) a.last_onehot[row * A + u] = (int8_t)(u == final_u);
    if (a.ep_u) {
        const int ts = a.t_ep ? a.t_ep[e] : a.t;
        if ((unsigned)ts < (unsigned)a.T) {
            const size_t k = ((size_t)e * a.T + ts) * n + j;
            a.ep_u[k] = (int8_t)final_u;
#pragma unroll
            for (int u = 0; u < A; ++u) a.ep_onehot[k * A + u] = (int8_t)(u == final_u);
        }
    }
}

}  // namespace shieldk
