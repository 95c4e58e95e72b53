// qmix_ops.hip -- the mixing + TD block of QMIX.learn (policy/qmix.py:104-122, network/qmix_net.py) after the hypernetworks'
// first-layer GEMM, one kernel each way.  See include/qmix_ops.h.
//
// Eight lanes share one (episode, step) row: lane `slot` owns the mixer columns j = slot, slot + 8, ... (M / 8 of them), so that
// the n x M hypernetwork outputs of a row are spread over the lanes; the row's sums over j are butterfly reductions inside the
// group of eight.  Every row is computed and written by its own group: no atomics besides the bad-action counter.
//
// The kernels are templated on an INDEX RULE that says where a row's operands live: PaddedIndex = the (b, t) rows of a padded
// batch (include/qmix_ops.h), PackedIndex = the packed (episode, step) units of include/qmix_packed.h.  The per-row arithmetic is
// one body, so a unit has the bits of the padded row.  k_gather_states (int8 state rows -> float32) is at the end.
//
// k_mix_forward<H, Index, true> is the same row body for the lambda-return targets (include/qmix_lambda.h): it writes the two q_tot of
// a row instead of mtd and mask, and the walk kernels of qmix_lambda_kernels.h form the targets from them.
//
// k_mix_forward<H, Index, kTotals, QSel> is the row body with double-Q targets (include/qmix_double.h): a selector's first maximum
// picks the action whose target value goes into the target mixer, where NoSel takes the row's own maximum.
//
// File map: td_rules.h (shared with vdn_ops.hip) holds NoSel / QSel, LambdaOff with its host check, and the packed preamble and
// phase B of the lambda walk; qmix_lambda_kernels.h holds phases A and C and the two walk kernels.  Here: the
// index rules, the operand structs (MixIn / MixOut, BackIn / BackOut), the mixer, the two row kernels, k_gather_states, then the host
// side: one argument check per shape, one launch function per kernel, forward_padded / forward_packed (rows, then the optional
// walk), and the extern "C" entry points, which fill the structs and call those.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/qmix_ops.h"
#include "../../include/qmix_packed.h"
#include "../../include/qmix_lambda.h"
#include "../../include/qmix_double.h"

#define HIP_ABI_TAG "qmix_ops"
#define HIP_ABI_ERR QMIX_ERR_HIP
#include "hip_abi.h"
#include "td_rules.h"   // NoSel / QSel (the compile-time variant of the target side of k_mix_forward), the lambda pieces

namespace {

constexpr int kM = 32;            // qmix_hidden_dim of every TrainParas table
constexpr int kLanes = 8;         // lanes per row
constexpr int kJ = kM / kLanes;   // mixer columns per lane
constexpr int kMaxN = 16;         // droplets (DMFB_MAX_AGENTS)
constexpr int kMaxA = 16;
constexpr int kBlock = 256;

struct Dims {
    int B, T, Tl, n, A;
    int p_rows, p_off;    // eval P layout
    int pt_rows, pt_off;  // target P layout
};

// Where the operands of row `row` live: its step in the replay tensors (ep), the first element of its n x A block in the Q
// tensors (q0) and its rows in the eval / target P.  The outputs of a row (mtd, mask, Z, X) are row `row` under either rule.
struct Loc {
    size_t ep, q0, pe, pt;
};

struct PaddedIndex {   // include/qmix_ops.h: time-major Q, P row b * p_rows + t + p_off
    Dims d;
    __device__ __forceinline__ long rows() const { return (long)d.B * d.T; }
    __device__ __forceinline__ Loc at(long row) const {
        const int b = (int)(row / d.T), t = (int)(row - (long)b * d.T);
        return Loc{(size_t)b * d.Tl + t, ((size_t)t * d.B + b) * d.n * d.A, (size_t)b * d.p_rows + t + d.p_off,
                   (size_t)b * d.pt_rows + t + d.pt_off};
    }
    __device__ __forceinline__ void zero_tail(float *, long, long) const {}
};

struct PackedIndex {   // include/qmix_packed.h: unit j = step units[j], Q rows j*n.., eval P row j, target P row target_row[j]
    const int32_t *units, *target_row;
    int n_units, n, A;
    long pad_elems;    // backward: floats of grad_q behind the units' rows, written as zeros
    __device__ __forceinline__ long rows() const { return n_units; }
    __device__ __forceinline__ Loc at(long row) const {
        return Loc{(size_t)units[row], (size_t)row * n * A, (size_t)row, target_row ? (size_t)target_row[row] : (size_t)row};
    }
    __device__ __forceinline__ void zero_tail(float *gq, long gid, long threads) const {
        float *tail = gq + (size_t)n_units * n * A;
        for (long e = gid; e < pad_elems; e += threads) tail[e] = 0.f;
    }
};

__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = 1; m < kLanes; m <<= 1) v += __shfl_xor(v, m, kLanes);
    return v;
}

template <int H> __device__ __forceinline__ float dot(const float *__restrict__ w, const float (&h)[H]) {
    const float4 *w4 = reinterpret_cast<const float4 *>(w);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < H / 4; ++k) {
        const float4 v = w4[k];
        acc = fmaf(v.x, h[4 * k], acc);
        acc = fmaf(v.y, h[4 * k + 1], acc);
        acc = fmaf(v.z, h[4 * k + 2], acc);
        acc = fmaf(v.w, h[4 * k + 3], acc);
    }
    return acc;
}

__device__ __forceinline__ float elu(float x) { return x > 0.f ? x : expm1f(x); }
__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

// q_tot of one row (every lane of the group returns it)
template <int H>
__device__ float mix_row(const float *__restrict__ P, const qmix_mixer &w, const float (&q)[kMaxN], int n, int slot) {
    float h1[H], h2[H];
#pragma unroll
    for (int h = 0; h < H; ++h) { h1[h] = fmaxf(P[h], 0.f); h2[h] = fmaxf(P[H + h], 0.f); }
    float acc = 0.f, accb = 0.f;
#pragma unroll
    for (int jj = 0; jj < kJ; ++jj) {
        const int j = slot + kLanes * jj;
        float pre = 0.f;
#pragma unroll
        for (int i = 0; i < kMaxN; ++i)
            if (i < n) pre = fmaf(q[i], fabsf(w.b1[i * kM + j] + dot<H>(w.w1 + (size_t)(i * kM + j) * H, h1)), pre);
        pre += P[2 * H + j];
        acc = fmaf(elu(pre), fabsf(w.b2[j] + dot<H>(w.w2 + (size_t)j * H, h2)), acc);
        accb = fmaf(w.wb[j], fmaxf(P[2 * H + kM + j], 0.f), accb);
    }
    return group_sum(acc) + (group_sum(accb) + w.bb[0]);
}

// ---- the operands of the block as the entry points of include/qmix_ops.h, qmix_packed.h, qmix_lambda.h and qmix_double.h take them
struct MixIn {
    const float *qe, *qt;
    const int8_t *u;
    const float *r;
    const int8_t *avail;
    const uint8_t *term, *padded;
    const float *pe, *pt;
    qmix_mixer we, wt;
    int n, A;
    float gamma;
};
struct MixOut {
    float *out0, *out1;   // mtd and mask, or with kTotals the two q_tot of the row
    int32_t *bad;
    float *targets;       // the one-step double-Q form only, may be NULL (under lambda the walk writes the targets)
};

// kTotals: out0 / out1 receive tot_e (NaN for a bad-action row) / tot_t of the row instead of mtd / mask.
// Sel: NoSel or QSel (td_rules.h).  Every lane of a row forms the picks; slot 0 writes them.
// The row body takes the operands one by one: pointers that arrive inside a struct cannot be __restrict__, and without it the picks
// store (a char store) and the row stores of the backward keep later loads from moving ahead of them (profiles/mix_block/NOTES.md).
// The selector comes by value for the same reason: behind a reference its members are formed again after every picks store.
template <int H, bool kTotals, class Index, class Sel>
__device__ __forceinline__ void mix_forward_row(const Index &ix, int n, int A, const float *__restrict__ qe, const float *__restrict__ qt,
                                                const int8_t *__restrict__ u, const float *__restrict__ r, const int8_t *__restrict__ avail,
                                                const uint8_t *__restrict__ term, const uint8_t *__restrict__ padded,
                                                const float *__restrict__ pe, const float *__restrict__ pt, const qmix_mixer &we,
                                                const qmix_mixer &wt, float gamma, float *__restrict__ out0, float *__restrict__ out1,
                                                int32_t *__restrict__ bad, float *__restrict__ targets, const Sel sel) {
    const long gid = (long)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = gid / kLanes < ix.rows();
    const long row = valid ? gid / kLanes : 0;   // idle lanes of the last group follow row 0 (the shuffles need every lane)
    const int slot = (int)(gid % kLanes);
    const Loc at = ix.at(row);
    const size_t ep = at.ep, q0 = at.q0;
    float q_e[kMaxN], q_t[kMaxN];
    bool ok = true;
    size_t s0 = q0;   // the selector's block of the row: laid out as q_target's unless sel_units places it
    if constexpr (Sel::on) ok = sel.place(row, n, A, s0);   // refused: the row's own target rows select
    const bool placed = ok;
    // the pick rule of vdn_ops.hip: td_row, with the agents' values kept apart for the mixer instead of added: change both together
    // (one shared function for the two cost k_mix_forward<32, PaddedIndex> a wave in every form tried: profiles/mix_block/NOTES.md)
#pragma unroll
    for (int i = 0; i < kMaxN; ++i) {
        q_e[i] = 0.f; q_t[i] = 0.f;
        if (i < n) {
            int a_taken = (int)u[ep * n + i];
            if ((unsigned)a_taken >= (unsigned)A) { ok = false; a_taken = 0; }   // torch.gather raises; never read out of bounds
            q_e[i] = qe[q0 + (size_t)i * A + a_taken];
            float m;
            if constexpr (Sel::on) {
                const int8_t *av = avail + (ep * n + i) * A;
                const float *qs = (placed ? sel.qs + s0 : qt + q0) + (size_t)i * A;
                int best = 0;
                float sm = av[0] == 0 ? -9999999.0f : qs[0];
                for (int a = 1; a < A; ++a) {
                    const float v = av[a] == 0 ? -9999999.0f : qs[a];
                    if (v > sm) { sm = v; best = a; }
                }
                m = av[best] == 0 ? -9999999.0f : qt[q0 + (size_t)i * A + best];
                if (valid && slot == 0 && sel.picks) sel.picks[(size_t)row * n + i] = placed ? (int8_t)best : (int8_t)-1;
            } else {
                m = -3.4e38f;
                for (int a = 0; a < A; ++a) {
                    const float v = avail[(ep * n + i) * A + a] == 0 ? -9999999.0f : qt[q0 + (size_t)i * A + a];
                    m = v > m ? v : m;
                }
            }
            q_t[i] = m;
        }
    }
    const float tot_e = mix_row<H>(pe + at.pe * (2 * H + 2 * kM), we, q_e, n, slot);
    const float tot_t = mix_row<H>(pt + at.pt * (2 * H + 2 * kM), wt, q_t, n, slot);
    if (valid && slot == 0) {
        if constexpr (kTotals) {
            out0[row] = ok ? tot_e : __builtin_nanf("");
            out1[row] = tot_t;
        } else {
            const float not_term = 1.0f - (term[ep] ? 1.0f : 0.0f);
            const float target = r[ep] + (gamma * tot_t) * not_term;
            const float mk = 1.0f - (padded[ep] ? 1.0f : 0.0f);
            out0[row] = ok ? mk * (tot_e - target) : __builtin_nanf("");
            out1[row] = mk;
            if constexpr (Sel::on) { if (targets) targets[row] = target; }
        }
        if (!ok && bad) atomicAdd(bad, 1);
    }
}

template <int H, class Index, bool kTotals = false, class Sel = NoSel>
__global__ __launch_bounds__(kBlock) void k_mix_forward(const Index ix, const MixIn in, const MixOut out, const Sel sel) {
    mix_forward_row<H, kTotals>(ix, in.n, in.A, in.qe, in.qt, in.u, in.r, in.avail, in.term, in.padded, in.pe, in.pt, in.we, in.wt, in.gamma,
                                out.out0, out.out1, out.bad, out.targets, sel);
}

#include "qmix_lambda_kernels.h"   // the walk over the episodes on those totals (include/qmix_lambda.h)

struct BackIn {
    const float *mtd, *maskf, *qe;
    const int8_t *u;
    const float *pe;
    qmix_mixer w;
    const float *g0;
    int n, A;
};
struct BackOut {
    float *gq, *gp, *z, *x;
};

template <int H, class Index>
__device__ __forceinline__ void mix_backward_row(const Index &ix, int n, int A, const float *__restrict__ mtd, const float *__restrict__ maskf,
                                                 const float *__restrict__ qe, const int8_t *__restrict__ u, const float *__restrict__ pe,
                                                 const qmix_mixer &w, const float *__restrict__ g0, float *__restrict__ gq,
                                                 float *__restrict__ gp, float *__restrict__ z, float *__restrict__ x) {
    constexpr int F = 2 * H + 2 * kM, XW = 2 * H + kM + 3;
    const long gid = (long)blockIdx.x * kBlock + threadIdx.x;
    ix.zero_tail(gq, gid, (long)gridDim.x * kBlock);
    const bool valid = gid / kLanes < ix.rows();
    const long row = valid ? gid / kLanes : 0;
    const int slot = (int)(gid % kLanes);
    const int ZW = n * kM + kM + 1;
    const Loc at = ix.at(row);
    const size_t ep = at.ep, q0 = at.q0;
    const float g = ((2.0f * mtd[row]) * maskf[row]) * g0[0];   // d num / d q_tot_eval of this row
    float q[kMaxN], dq[kMaxN];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < kMaxN; ++i) {
        q[i] = 0.f; dq[i] = 0.f;
        if (i < n) {
            int a_taken = (int)u[ep * n + i];
            if ((unsigned)a_taken >= (unsigned)A) { ok = false; a_taken = 0; }   // mtd is NaN for the row: every gradient below is NaN
            q[i] = qe[q0 + (size_t)i * A + a_taken];
        }
    }
    const float *P = pe + at.pe * F;
    float *dP = gp + at.pe * F;
    float *Z = z + (size_t)row * ZW;
    float *X = x + (size_t)row * XW;
    float h1[H], h2[H], dh1[H], dh2[H];
#pragma unroll
    for (int h = 0; h < H; ++h) { h1[h] = fmaxf(P[h], 0.f); h2[h] = fmaxf(P[H + h], 0.f); dh1[h] = 0.f; dh2[h] = 0.f; }
#pragma unroll
    for (int jj = 0; jj < kJ; ++jj) {
        const int j = slot + kLanes * jj;
        float zi[kMaxN];
        float pre = 0.f;
#pragma unroll
        for (int i = 0; i < kMaxN; ++i) {
            zi[i] = 0.f;
            if (i < n) {
                zi[i] = w.b1[i * kM + j] + dot<H>(w.w1 + (size_t)(i * kM + j) * H, h1);
                pre = fmaf(q[i], fabsf(zi[i]), pre);
            }
        }
        pre += P[2 * H + j];
        const float hid = elu(pre);
        const float z2 = w.b2[j] + dot<H>(w.w2 + (size_t)j * H, h2);
        const float dpre = (g * fabsf(z2)) * (pre > 0.f ? 1.f : expf(pre));
        const float dz2 = sgn(z2) * (g * hid);
        const float hbp = P[2 * H + kM + j];
        if (valid) {
            Z[n * kM + j] = dz2;
            dP[2 * H + j] = dpre;
            dP[2 * H + kM + j] = hbp > 0.f ? g * w.wb[j] : 0.f;
            X[2 * H + 2 + j] = fmaxf(hbp, 0.f);
        }
        const float *w2r = w.w2 + (size_t)j * H;
#pragma unroll
        for (int h = 0; h < H; ++h) dh2[h] = fmaf(w2r[h], dz2, dh2[h]);
#pragma unroll
        for (int i = 0; i < kMaxN; ++i) {
            if (i < n) {
                const float dz1 = sgn(zi[i]) * (q[i] * dpre);
                if (valid) Z[i * kM + j] = dz1;
                const float *w1r = w.w1 + (size_t)(i * kM + j) * H;
#pragma unroll
                for (int h = 0; h < H; ++h) dh1[h] = fmaf(w1r[h], dz1, dh1[h]);
                dq[i] = fmaf(fabsf(zi[i]), dpre, dq[i]);
            }
        }
    }
#pragma unroll
    for (int h = 0; h < H; ++h) { dh1[h] = group_sum(dh1[h]); dh2[h] = group_sum(dh2[h]); }
#pragma unroll
    for (int i = 0; i < kMaxN; ++i) dq[i] = group_sum(dq[i]);
    if (!valid) return;
#pragma unroll
    for (int h = 0; h < H; ++h) {
        if (h % kLanes == slot) {
            dP[h] = P[h] > 0.f ? dh1[h] : 0.f;
            dP[H + h] = P[H + h] > 0.f ? dh2[h] : 0.f;
            X[h] = h1[h];
            X[H + 1 + h] = h2[h];
        }
    }
    if (slot == 0) {
        X[H] = 1.f; X[2 * H + 1] = 1.f; X[2 * H + 2 + kM] = 1.f;
        Z[n * kM + kM] = g;
    }
#pragma unroll
    for (int i = 0; i < kMaxN; ++i) {
        if (i < n) {
            const int a_taken = (int)u[ep * n + i];
            float *dst = gq + q0 + (size_t)i * A;
            // a bad action anywhere in the row: the whole row of grad_q is NaN, every agent's entries
            for (int a = slot; a < A; a += kLanes) dst[a] = (!ok || a == a_taken) ? dq[i] : 0.f;
        }
    }
}

template <int H, class Index>
__global__ __launch_bounds__(kBlock) void k_mix_backward(const Index ix, const BackIn in, const BackOut out) {
    mix_backward_row<H>(ix, in.n, in.A, in.mtd, in.maskf, in.qe, in.u, in.pe, in.w, in.g0, out.gq, out.gp, out.z, out.x);
}

// ---- qmix_gather_states: int8 state rows picked by index -> float32 rows.  1 byte in, 4 bytes out per element: a bandwidth kernel.
// Sixteen lanes share one (row, chunk) item of 256 FRAME columns; frame column f = column + (source address of the row & 15), so
// that f % 16 == 0 is where the source is 16-byte aligned.  A lane owns 16 frame columns (one 16-byte load), the four lanes of a
// lane quad 64.  A quad whose 64 columns lie inside the row and whose output is 16-byte aligned there takes the fast path: one
// 16-byte load per lane, a 4 x 4 transpose of the dwords inside the quad, then four stores in each of which a lane turns 4 source
// bytes into one 16-byte store and the quad writes 64 contiguous bytes.  In every other quad (the head and the tail of a row, rows
// whose source and output phases differ) a lane takes its groups of four columns one by one: a 4-byte load and one 16-byte store
// where the group lies inside the row and its output is 16-byte aligned, byte by byte otherwise.
constexpr int kGLanes = 16;
constexpr int kGCols = kGLanes * 16;
constexpr int kGMaxBlocks = 8192;

__device__ __forceinline__ float4 bytes4(uint32_t w) {
    return make_float4((float)(int8_t)(w & 0xffu), (float)(int8_t)((w >> 8) & 0xffu), (float)(int8_t)((w >> 16) & 0xffu),
                       (float)(int8_t)(w >> 24));
}

__global__ __launch_bounds__(kBlock) void k_gather_states(const int8_t *__restrict__ states, long n_state_rows, int S,
                                                          const int32_t *__restrict__ rows, long n_items, int chunks,
                                                          float *__restrict__ out) {
    const long threads = (long)gridDim.x * kBlock;
    const float nan = __builtin_nanf("");
    for (long g = (long)blockIdx.x * kBlock + threadIdx.x; g < n_items * kGLanes; g += threads) {   // a quad shares its trip count
        const long item = g / kGLanes;
        const int lane = (int)(g % kGLanes), j = lane & 3;
        const long i = item / chunks, ch = item - i * chunks;
        const int r = rows[i];
        const bool ok = r >= 0 && (long)r < n_state_rows;       // a row id outside the tensor is never turned into an address
        const int8_t *src = states + (ok ? (size_t)r * S : 0);
        float *dst = out + (size_t)i * S;
        const long ps = (long)((uintptr_t)src & 15);
        const long quad = ch * kGCols + (lane & ~3) * 16 - ps;    // first column of the quad's 64 (may be < 0 or >= S)
        const bool fast = quad >= 0 && quad + 64 <= S && ((uintptr_t)(dst + quad) & 15) == 0;
        if (fast) {
            float4 *o = reinterpret_cast<float4 *>(dst + quad + 4 * j);
            if (!ok) {
#pragma unroll
                for (int k = 0; k < 4; ++k) o[4 * k] = make_float4(nan, nan, nan, nan);
                continue;
            }
            const uint4 w = *reinterpret_cast<const uint4 *>(src + quad + 16 * j);
            uint32_t v[4] = {w.x, w.y, w.z, w.w};
            // transpose inside the quad: lane j ends with v[k] = dword j of lane k, the source bytes 16 k + 4 j .. + 3 of the quad
            {
                const bool odd = j & 1;
                const uint32_t a = __shfl_xor(odd ? v[0] : v[1], 1, 4), b = __shfl_xor(odd ? v[2] : v[3], 1, 4);
                if (odd) { v[0] = a; v[2] = b; } else { v[1] = a; v[3] = b; }
                const bool hi = j & 2;
                const uint32_t c = __shfl_xor(hi ? v[0] : v[2], 2, 4), e = __shfl_xor(hi ? v[1] : v[3], 2, 4);
                if (hi) { v[0] = c; v[1] = e; } else { v[2] = c; v[3] = e; }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) o[4 * k] = bytes4(v[k]);
        } else {
            // the same four columns per lane and step as above (their source is 4-byte aligned: src + quad is 16-byte aligned);
            // a group that lies inside the row with a 16-byte aligned output still leaves as one store, the others byte by byte
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long c4 = quad + 16 * k + 4 * j;
                if (c4 >= 0 && c4 + 4 <= S && ((uintptr_t)(dst + c4) & 15) == 0) {
                    *reinterpret_cast<float4 *>(dst + c4) =
                        ok ? bytes4(*reinterpret_cast<const uint32_t *>(src + c4)) : make_float4(nan, nan, nan, nan);
                } else {
                    for (int e = 0; e < 4; ++e) {
                        const long c = c4 + e;
                        if (c >= 0 && c < S) dst[c] = ok ? (float)src[c] : nan;
                    }
                }
            }
        }
    }
}

// ---- host side.  Every check below answers with the code its entry point returns; their order is part of the ABI: n_units < 0
// before the shape, the shape (QMIX_ERR_UNSUPPORTED outside the build limits) before the NULL checks, no units (QMIX_OK, nothing
// launched) only after every check.
int check_shape(int n, int A, int H, int M, const qmix_mixer *m) {
    if (n <= 0 || A <= 0 || !m) return QMIX_ERR_BAD_ARG;
    if (M != kM || (H != 24 && H != 32) || n > kMaxN || A > kMaxA) return QMIX_ERR_UNSUPPORTED;
    const uintptr_t al = (uintptr_t)m->w1 | (uintptr_t)m->w2;   // rows are read as float4
    if (!m->w1 || !m->b1 || !m->w2 || !m->b2 || !m->wb || !m->bb || (al & 15)) return QMIX_ERR_BAD_ARG;
    return QMIX_OK;
}

// a NULL mixer is refused by check_shape before anything reads this copy
qmix_mixer mixer(const qmix_mixer *m) { return m ? *m : qmix_mixer{}; }

// what the target kinds add to the one-step block: lambda-returns (include/qmix_lambda.h) and double-Q targets (include/qmix_double.h)
struct Form {
    enum Kind { one_step, lambda, double_q } kind;
    float lam;
    float *tot_e, *tot_t;   // the hand-off of the rows launch to the walk
    QSel sel;               // double_q only
    int n_steps;            // packed forms that walk: the steps of the longest episode and, per step, the episodes longer than it
    const int32_t *counts;
    bool walk() const { return kind == lambda || (kind == double_q && lam > 0.0f); }   // double-Q at lam == 0 is the one-step rule
};
constexpr Form kOneStep{Form::one_step, 0.0f, nullptr, nullptr, QSel{}, 0, nullptr};

// the shape and the operands that the padded and the packed entry points share; the callers check their own row layout
int forward_args_check(int H, int M, const qmix_mixer *eval, const qmix_mixer *target, const MixIn &in, const MixOut &out) {
    int rc = check_shape(in.n, in.A, H, M, eval);
    if (!rc) rc = check_shape(in.n, in.A, H, M, target);
    if (rc) return rc;
    const bool given = in.qe && in.qt && in.u && in.r && in.avail && in.term && in.padded && in.pe && in.pt && out.out0 && out.out1;
    return given ? QMIX_OK : QMIX_ERR_BAD_ARG;
}
int backward_args_check(int H, int M, const qmix_mixer *eval, const BackIn &in, const BackOut &out) {
    const int rc = check_shape(in.n, in.A, H, M, eval);
    if (rc) return rc;
    const bool given = in.mtd && in.maskf && in.qe && in.u && in.pe && in.g0 && out.gq && out.gp && out.z && out.x;
    return given ? QMIX_OK : QMIX_ERR_BAD_ARG;
}
bool padded_shape_ok(const Dims &d) { return d.B > 0 && d.T > 0 && d.Tl >= d.T; }
bool p_rows_ok(int T, int rows, int off) { return off >= 0 && rows >= T + off; }

dim3 grid(long rows) { return dim3((unsigned)((rows * kLanes + kBlock - 1) / kBlock)); }

// ---- the one launch of each row kernel
template <class Index, bool kTotals, class Sel>
int launch_forward(const Index &ix, long rows, int H, const MixIn &in, const MixOut &out, const Sel &sel, void *stream) {
    const auto kernel = H == 24 ? k_mix_forward<24, Index, kTotals, Sel> : k_mix_forward<32, Index, kTotals, Sel>;
    LAUNCH(kernel, grid(rows), dim3(kBlock), 0, (hipStream_t)stream, ix, in, out, sel);
    return QMIX_OK;
}
template <class Index>
int launch_backward(const Index &ix, long rows, int H, const BackIn &in, const BackOut &out, void *stream) {
    const auto kernel = H == 24 ? k_mix_backward<24, Index> : k_mix_backward<32, Index>;
    LAUNCH(kernel, grid(rows), dim3(kBlock), 0, (hipStream_t)stream, ix, in, out);
    return QMIX_OK;
}

// the rows of a forward: mtd and mask, or under a walk the two q_tot that the walk reads
template <class Index>
int forward_rows(const Index &ix, long rows, int H, const MixIn &in, const MixOut &out, const Form &f, void *stream) {
    if (!f.walk()) {
        return f.kind == Form::double_q ? launch_forward<Index, false>(ix, rows, H, in, out, f.sel, stream)
                                        : launch_forward<Index, false>(ix, rows, H, in, out, NoSel{}, stream);
    }
    const MixOut totals{f.tot_e, f.tot_t, out.bad, nullptr};
    return f.kind == Form::double_q ? launch_forward<Index, true>(ix, rows, H, in, totals, f.sel, stream)
                                    : launch_forward<Index, true>(ix, rows, H, in, totals, NoSel{}, stream);
}
dim3 walk_grid(int episodes) { return dim3((unsigned)((episodes + kLamEp - 1) / kLamEp)); }
WalkIn walk_in(const MixIn &in, const Form &f) { return WalkIn{f.tot_e, f.tot_t, in.r, in.term, in.padded, in.gamma, f.lam}; }

// ---- the padded forward of every form: the rows, then the walk where the form has one (the lambda form also at lam == 0)
int forward_padded(const Dims &d, int H, int M, const qmix_mixer *eval, const qmix_mixer *target, const MixIn &in, const MixOut &out,
                   const Form &f, void *stream) {
    if (!padded_shape_ok(d)) return QMIX_ERR_BAD_ARG;
    int rc = forward_args_check(H, M, eval, target, in, out);
    if (rc) return rc;
    if (!p_rows_ok(d.T, d.p_rows, d.p_off) || !p_rows_ok(d.T, d.pt_rows, d.pt_off)) return QMIX_ERR_BAD_ARG;
    if (f.kind != Form::one_step && !lambda_ok(f.lam)) return QMIX_ERR_BAD_ARG;
    if (f.kind == Form::double_q && !f.sel.qs) return QMIX_ERR_BAD_ARG;
    if (f.walk() && (d.T > QMIX_LAMBDA_MAX_T || !f.tot_e || !f.tot_t)) return QMIX_ERR_BAD_ARG;
    rc = forward_rows(PaddedIndex{d}, (long)d.B * d.T, H, in, out, f, stream);
    if (rc || !f.walk()) return rc;
    LAUNCH(k_mix_lambda_walk, walk_grid(d.B), dim3(256), 0, (hipStream_t)stream, PaddedWalk{d.T, d.Tl}, d.B, walk_in(in, f),
           WalkOut{out.out0, out.out1, out.targets});
    return QMIX_OK;
}

// ---- the packed forward of every form.  f.counts is read only where the form walks.
int forward_packed(const int32_t *units, const int32_t *target_row, int n_units, int H, int M, const qmix_mixer *eval,
                   const qmix_mixer *target, const MixIn &in, const MixOut &out, const Form &f, void *stream) {
    if (n_units < 0) return QMIX_ERR_BAD_ARG;
    int rc = forward_args_check(H, M, eval, target, in, out);
    if (rc) return rc;
    if (!units) return QMIX_ERR_BAD_ARG;
    if (f.kind != Form::one_step && !lambda_ok(f.lam)) return QMIX_ERR_BAD_ARG;
    if (f.kind == Form::double_q && (!f.sel.qs || f.sel.n_sel < 1 || (!f.sel.sel_units && f.sel.n_sel < n_units))) return QMIX_ERR_BAD_ARG;
    LambdaOff lo;
    if (f.walk() && (!f.tot_e || !f.tot_t || f.n_steps < 0 || f.n_steps > QMIX_LAMBDA_MAX_T ||
                     !lambda_offsets(n_units, f.n_steps, f.counts, lo)))
        return QMIX_ERR_BAD_ARG;
    if (n_units == 0) return QMIX_OK;
    rc = forward_rows(PackedIndex{units, target_row, n_units, in.n, in.A, 0}, n_units, H, in, out, f, stream);
    if (rc || !f.walk()) return rc;
    const int E = f.counts[0];
    LAUNCH(k_mix_lambda_walk_packed, walk_grid(E), dim3(256), 0, (hipStream_t)stream, PackedWalk{units, nullptr}, E, f.n_steps, walk_in(in, f),
           WalkOut{out.out0, out.out1, out.targets}, lo);
    return QMIX_OK;
}

}  // namespace

extern "C" {

int qmix_mix_td_forward(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r, const int8_t *d_avail_next,
                        const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T, int32_t t_limit, int32_t n_agents,
                        int32_t n_actions, const float *d_p_eval, int32_t p_eval_rows, int32_t p_eval_off, const float *d_p_target,
                        int32_t p_target_rows, int32_t p_target_off, int32_t hyper_hidden, int32_t qmix_hidden, const qmix_mixer *eval,
                        const qmix_mixer *target, float gamma, float *d_mtd, float *d_mask, int32_t *d_bad_actions, void *stream) {
    const Dims d{B, T, t_limit, n_agents, n_actions, p_eval_rows, p_eval_off, p_target_rows, p_target_off};
    const MixIn in{d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded, d_p_eval, d_p_target, mixer(eval), mixer(target),
                   n_agents, n_actions, gamma};
    return forward_padded(d, hyper_hidden, qmix_hidden, eval, target, in, MixOut{d_mtd, d_mask, d_bad_actions, nullptr}, kOneStep, stream);
}

int qmix_mix_td_backward(const float *d_mtd, const float *d_mask, const float *d_q_eval, const int8_t *d_u, int32_t B, int32_t T,
                         int32_t t_limit, int32_t n_agents, int32_t n_actions, const float *d_p_eval, int32_t p_eval_rows,
                         int32_t p_eval_off, int32_t hyper_hidden, int32_t qmix_hidden, const qmix_mixer *eval,
                         const float *d_grad_num, float *d_grad_q, float *d_grad_p, float *d_z, float *d_x, void *stream) {
    const Dims d{B, T, t_limit, n_agents, n_actions, p_eval_rows, p_eval_off, 0, 0};
    const BackIn in{d_mtd, d_mask, d_q_eval, d_u, d_p_eval, mixer(eval), d_grad_num, n_agents, n_actions};
    const BackOut out{d_grad_q, d_grad_p, d_z, d_x};
    if (!padded_shape_ok(d)) return QMIX_ERR_BAD_ARG;
    const int rc = backward_args_check(hyper_hidden, qmix_hidden, eval, in, out);
    if (rc) return rc;
    if (!p_rows_ok(T, p_eval_rows, p_eval_off)) return QMIX_ERR_BAD_ARG;
    return launch_backward(PaddedIndex{d}, (long)B * T, hyper_hidden, in, out, stream);
}

int qmix_mix_td_forward_packed(const float *d_q_eval, const float *d_q_target, const int32_t *d_units, int32_t n_units,
                               const int8_t *d_u, const float *d_r, const int8_t *d_avail_next, const uint8_t *d_terminated,
                               const uint8_t *d_padded, int32_t n_agents, int32_t n_actions, const float *d_p_eval,
                               const float *d_p_target, const int32_t *d_p_target_row, int32_t hyper_hidden, int32_t qmix_hidden,
                               const qmix_mixer *eval, const qmix_mixer *target, float gamma, float *d_mtd, float *d_mask,
                               int32_t *d_bad_actions, void *stream) {
    const MixIn in{d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded, d_p_eval, d_p_target, mixer(eval), mixer(target),
                   n_agents, n_actions, gamma};
    return forward_packed(d_units, d_p_target_row, n_units, hyper_hidden, qmix_hidden, eval, target, in,
                          MixOut{d_mtd, d_mask, d_bad_actions, nullptr}, kOneStep, stream);
}

int qmix_mix_td_backward_packed(const float *d_mtd, const float *d_mask, const float *d_q_eval, const int32_t *d_units,
                                int32_t n_units, const int8_t *d_u, int32_t n_agents, int32_t n_actions, int32_t rows_pad,
                                const float *d_p_eval, int32_t hyper_hidden, int32_t qmix_hidden, const qmix_mixer *eval,
                                const float *d_grad_num, float *d_grad_q, float *d_grad_p, float *d_z, float *d_x, void *stream) {
    if (n_units < 0) return QMIX_ERR_BAD_ARG;
    const BackIn in{d_mtd, d_mask, d_q_eval, d_u, d_p_eval, mixer(eval), d_grad_num, n_agents, n_actions};
    const BackOut out{d_grad_q, d_grad_p, d_z, d_x};
    const int rc = backward_args_check(hyper_hidden, qmix_hidden, eval, in, out);
    if (rc) return rc;
    if (!d_units || (long)rows_pad < (long)n_units * n_agents) return QMIX_ERR_BAD_ARG;
    if (n_units == 0) return QMIX_OK;
    const PackedIndex ix{d_units, nullptr, n_units, n_agents, n_actions, ((long)rows_pad - (long)n_units * n_agents) * n_actions};
    return launch_backward(ix, n_units, hyper_hidden, in, out, stream);
}

// ---- the mixing + TD block on lambda-returns (include/qmix_lambda.h): the rows' totals, then the walk of qmix_lambda_kernels.h
int qmix_mix_td_lambda_forward(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r,
                               const int8_t *d_avail_next, const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T,
                               int32_t t_limit, int32_t n_agents, int32_t n_actions, const float *d_p_eval, int32_t p_eval_rows,
                               int32_t p_eval_off, const float *d_p_target, int32_t p_target_rows, int32_t p_target_off,
                               int32_t hyper_hidden, int32_t qmix_hidden, const qmix_mixer *eval, const qmix_mixer *target, float gamma,
                               float *d_mtd, float *d_mask, int32_t *d_bad_actions, float lam, float *d_q_tot_eval,
                               float *d_q_tot_target, float *d_targets, void *stream) {
    const Dims d{B, T, t_limit, n_agents, n_actions, p_eval_rows, p_eval_off, p_target_rows, p_target_off};
    const MixIn in{d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded, d_p_eval, d_p_target, mixer(eval), mixer(target),
                   n_agents, n_actions, gamma};
    return forward_padded(d, hyper_hidden, qmix_hidden, eval, target, in, MixOut{d_mtd, d_mask, d_bad_actions, d_targets},
                          Form{Form::lambda, lam, d_q_tot_eval, d_q_tot_target, QSel{}, 0, nullptr}, stream);
}

int qmix_mix_td_lambda_forward_packed(const float *d_q_eval, const float *d_q_target, const int32_t *d_units, int32_t n_units,
                                      const int8_t *d_u, const float *d_r, const int8_t *d_avail_next, const uint8_t *d_terminated,
                                      const uint8_t *d_padded, int32_t n_agents, int32_t n_actions, const float *d_p_eval,
                                      const float *d_p_target, const int32_t *d_p_target_row, int32_t hyper_hidden,
                                      int32_t qmix_hidden, const qmix_mixer *eval, const qmix_mixer *target, float gamma, float *d_mtd,
                                      float *d_mask, int32_t *d_bad_actions, float lam, float *d_q_tot_eval, float *d_q_tot_target,
                                      float *d_targets, int32_t n_steps, const int32_t *counts, void *stream) {
    const MixIn in{d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded, d_p_eval, d_p_target, mixer(eval), mixer(target),
                   n_agents, n_actions, gamma};
    return forward_packed(d_units, d_p_target_row, n_units, hyper_hidden, qmix_hidden, eval, target, in,
                          MixOut{d_mtd, d_mask, d_bad_actions, d_targets},
                          Form{Form::lambda, lam, d_q_tot_eval, d_q_tot_target, QSel{}, n_steps, counts}, stream);
}

// ---- the same two blocks with double-Q targets (include/qmix_double.h): lam == 0 is the one-step row kernel with the selector,
// lam > 0 the rows' totals with the selector, then the unchanged walk
int qmix_mix_td_double_forward(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r,
                               const int8_t *d_avail_next, const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T,
                               int32_t t_limit, int32_t n_agents, int32_t n_actions, const float *d_p_eval, int32_t p_eval_rows,
                               int32_t p_eval_off, const float *d_p_target, int32_t p_target_rows, int32_t p_target_off,
                               int32_t hyper_hidden, int32_t qmix_hidden, const qmix_mixer *eval, const qmix_mixer *target, float gamma,
                               float *d_mtd, float *d_mask, int32_t *d_bad_actions, float lam, float *d_q_tot_eval,
                               float *d_q_tot_target, float *d_targets, const float *d_q_sel, int8_t *d_picks, void *stream) {
    const Dims d{B, T, t_limit, n_agents, n_actions, p_eval_rows, p_eval_off, p_target_rows, p_target_off};
    const MixIn in{d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded, d_p_eval, d_p_target, mixer(eval), mixer(target),
                   n_agents, n_actions, gamma};
    return forward_padded(d, hyper_hidden, qmix_hidden, eval, target, in, MixOut{d_mtd, d_mask, d_bad_actions, d_targets},
                          Form{Form::double_q, lam, d_q_tot_eval, d_q_tot_target, QSel{d_q_sel, nullptr, 0, d_picks}, 0, nullptr}, stream);
}

int qmix_mix_td_double_forward_packed(const float *d_q_eval, const float *d_q_target, const int32_t *d_units, int32_t n_units,
                                      const int8_t *d_u, const float *d_r, const int8_t *d_avail_next, const uint8_t *d_terminated,
                                      const uint8_t *d_padded, int32_t n_agents, int32_t n_actions, const float *d_p_eval,
                                      const float *d_p_target, const int32_t *d_p_target_row, int32_t hyper_hidden,
                                      int32_t qmix_hidden, const qmix_mixer *eval, const qmix_mixer *target, float gamma, float *d_mtd,
                                      float *d_mask, int32_t *d_bad_actions, float lam, float *d_q_tot_eval, float *d_q_tot_target,
                                      float *d_targets, int32_t n_steps, const int32_t *counts, const float *d_q_sel,
                                      int32_t n_sel_units, const int32_t *d_sel_units, int8_t *d_picks, void *stream) {
    const MixIn in{d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded, d_p_eval, d_p_target, mixer(eval), mixer(target),
                   n_agents, n_actions, gamma};
    return forward_packed(d_units, d_p_target_row, n_units, hyper_hidden, qmix_hidden, eval, target, in,
                          MixOut{d_mtd, d_mask, d_bad_actions, d_targets},
                          Form{Form::double_q, lam, d_q_tot_eval, d_q_tot_target, QSel{d_q_sel, d_sel_units, n_sel_units, d_picks}, n_steps,
                               counts},
                          stream);
}

int qmix_gather_states(const int8_t *d_states, int64_t n_state_rows, int32_t state_len, const int32_t *d_rows, int32_t n_rows,
                       float *d_out, void *stream) {
    if (!d_states || !d_rows || !d_out || n_rows < 0 || state_len < 1 || n_state_rows < 1) return QMIX_ERR_BAD_ARG;
    if (n_rows == 0) return QMIX_OK;
    const long chunks = ((long)state_len + 15 + kGCols - 1) / kGCols;   // the frame columns of a row lie in [0, state_len + 15)
    const long n_items = (long)n_rows * chunks;
    const long blocks = (n_items * kGLanes + kBlock - 1) / kBlock;
    LAUNCH(k_gather_states, dim3((unsigned)(blocks < kGMaxBlocks ? blocks : kGMaxBlocks)), dim3(kBlock), 0, (hipStream_t)stream, d_states,
           (long)n_state_rows, state_len, d_rows, n_items, (int)chunks, d_out);
    return QMIX_OK;
}

int qmix_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
