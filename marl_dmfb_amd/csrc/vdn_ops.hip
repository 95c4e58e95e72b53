// vdn_ops.hip -- the TD-error block of VDN.learn (policy/vdn.py:104-123) as one kernel each way.  See include/vdn_ops.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vdn_ops.h"
#include "../../include/vdn_tail.h"
#include "../../include/vdn_double.h"

#define HIP_ABI_TAG "vdn_ops"
#define HIP_ABI_ERR VDN_ERR_HIP
#include "hip_abi.h"
#include "td_rules.h"   // NoSel / QSel and the shared pieces of the lambda walk: one copy for this file and qmix_ops.hip

namespace {

// ---- num = sum(mtd^2) and mask_sum inside the TD forward launch (d_sums != NULL): every workgroup adds its 256 slots in a fixed
// order (wave shuffles, then the four waves), writes the pair to part[2 * block], and the workgroup that arrives last
// (hip_abi.h: last_workgroup_arrives) adds the pairs of all workgroups in a fixed order: deterministic, no float atomics.
__device__ unsigned g_td_ticket = 0;
__device__ __forceinline__ void td_block_sums(float sq, float mk, float *part, float *__restrict__ sums) {
    __shared__ float s_w[2][4];
    __shared__ int s_last;
    for (int o = 32; o > 0; o >>= 1) { sq += __shfl_xor(sq, o); mk += __shfl_xor(mk, o); }
    if ((threadIdx.x & 63) == 0) { s_w[0][threadIdx.x >> 6] = sq; s_w[1][threadIdx.x >> 6] = mk; }
    __syncthreads();
    if (threadIdx.x < 2) part[2 * blockIdx.x + threadIdx.x] = (s_w[threadIdx.x][0] + s_w[threadIdx.x][1]) + (s_w[threadIdx.x][2] + s_w[threadIdx.x][3]);
    if (!last_workgroup_arrives(&g_td_ticket, gridDim.x, &s_last)) return;
    if (threadIdx.x < 128) {   // wave 0 adds the squares, wave 1 the mask: lane-strided walks, then the shuffle tree
        const int which = threadIdx.x >> 6;
        float t = 0.0f;
        for (unsigned b = threadIdx.x & 63; b < gridDim.x; b += 64) t += partial_load(part + 2 * b + which);
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if ((threadIdx.x & 63) == 0) sums[which] = t;
    }
}

// ---- the operands of the TD block as the entry points of include/vdn_ops.h, vdn_tail.h and vdn_lambda.h take them
struct TdIn {
    const float *qe, *qt;
    const int8_t *u;
    const float *r;
    const int8_t *avail;
    const uint8_t *term, *padded;
    int n, A;
    float gamma;
};
struct TdOut {
    float *mtd, *maskf, *targets;   // targets: the lambda entry points only
    int32_t *bad;
    float *part, *sums;
};

// ---- where an output row lives.  at(row): ep, its slot in the replay tensors, q0, the first element of its n x A block in the
// Q tensors, and s0, that of its selector block (include/vdn_double.h; q0 until QSel::place moves it); row(b, t): step t of episode b
// (the lambda walk); unit(k): Q-tensor unit k -> (output row, ep), for the backward; pad_rows: the zero rows of grad_q behind the
// last unit.
struct At {
    size_t ep, q0, s0;
};
struct UnitOf {
    size_t row, ep;
};
// padded: outputs [B][T], chip-major replay tensors [B][Tl], time-major Q tensors [T][B]
struct PaddedIndex {
    int B, T, Tl;
    static constexpr long pad_rows = 0;
    __device__ __forceinline__ int rows() const { return B * T; }
    __device__ __forceinline__ int row(int b, int t) const { return b * T + t; }
    __device__ __forceinline__ At at(int row, int n, int A) const {
        const int b = row / T, t = row - b * T;
        const size_t q0 = ((size_t)t * B + b) * n * A;
        return {(size_t)b * Tl + t, q0, q0};
    }
    __device__ __forceinline__ UnitOf unit(long k) const {
        const int b = (int)(k % B), t = (int)(k / B);
        return {(size_t)(b * T + t), (size_t)b * Tl + t};
    }
};
// packed (include/vdn_ops.h: vdn_td_forward_packed): row j is unit j, step units[j] % t_limit of the episode in slot
// units[j] / t_limit; its n rows of the Q tensors are rows j*n .. j*n + n - 1.  off[t]: the first unit of step t (lambda walk only)
struct PackedIndex {
    const int32_t *units;
    int U;
    long pad_rows;
    const int32_t *off;
    __device__ __forceinline__ int rows() const { return U; }
    __device__ __forceinline__ int row(int b, int t) const { return off[t] + b; }
    __device__ __forceinline__ At at(int row, int n, int A) const { return {(size_t)units[row], (size_t)row * n * A, (size_t)row * n * A}; }
    __device__ __forceinline__ UnitOf unit(long k) const { return {(size_t)k, (size_t)units[k]}; }
};

// ---- the pick rule of one (episode, step): the taken action's Q and the best available target Q, the agents added in index order.
// Sel is the compile-time variant of the target side: NoSel, the maximum over the target network's own row, or QSel, the selector of
// include/vdn_double.h (td_rules.h), where the first maximum of the selector row picks the action that the target network values.
// k_mix_forward of qmix_ops.hip holds the same pick with the agents kept apart: change both together.
struct TdRow {
    float qe_tot, qt_tot;
    bool ok;   // false: an action outside [0, A), or a selector unit outside its tensor
};
template <class Sel>
__device__ __forceinline__ TdRow td_row(const TdIn &in, At at, const Sel &sel, int row) {
    const int n = in.n, A = in.A;
    float qe_tot = 0.0f, qt_tot = 0.0f;
    bool ok = true;
    if constexpr (Sel::on) ok = sel.place(row, n, A, at.s0);   // refused: the slot's own target rows select
    const bool placed = ok;
    for (int i = 0; i < n; ++i) {
        int a_taken = (int)in.u[at.ep * n + i];
        if ((unsigned)a_taken >= (unsigned)A) { ok = false; a_taken = 0; }  // torch.gather raises here; never read out of bounds
        qe_tot = qe_tot + in.qe[at.q0 + (size_t)i * A + a_taken];
        float m;
        if constexpr (Sel::on) {
            const int8_t *av = in.avail + (at.ep * n + i) * A;
            const float *qs = (placed ? sel.qs + at.s0 : in.qt + at.q0) + (size_t)i * A;
            int best = 0;
            float sm = av[0] == 0 ? -9999999.0f : qs[0];
            for (int a = 1; a < A; ++a) {
                const float v = av[a] == 0 ? -9999999.0f : qs[a];
                if (v > sm) { sm = v; best = a; }
            }
            m = av[best] == 0 ? -9999999.0f : in.qt[at.q0 + (size_t)i * A + best];
            if (sel.picks) sel.picks[(size_t)row * n + i] = placed ? (int8_t)best : (int8_t)-1;
        } else {
            m = -3.4e38f;
            for (int a = 0; a < A; ++a) {
                const float v = in.avail[(at.ep * n + i) * A + a] == 0 ? -9999999.0f : in.qt[at.q0 + (size_t)i * A + a];
                m = v > m ? v : m;
            }
        }
        qt_tot = qt_tot + m;
    }
    return {qe_tot, qt_tot, ok};
}

// one thread per output row
template <class Index, class Sel>
__device__ __forceinline__ void td_forward_rows(const Index &ix, const TdIn &in, const TdOut &out, const Sel &sel, const int row) {
    float sq = 0.0f, mks = 0.0f;
    if (row < ix.rows()) {
        const At at = ix.at(row, in.n, in.A);
        const TdRow q = td_row(in, at, sel, row);
        const float not_term = 1.0f - (in.term[at.ep] ? 1.0f : 0.0f);
        const float target = in.r[at.ep] + (in.gamma * q.qt_tot) * not_term;
        const float mk = 1.0f - (in.padded[at.ep] ? 1.0f : 0.0f);
        const float m = q.ok ? mk * (target - q.qe_tot) : __builtin_nanf("");  // an action outside [0, A) poisons the loss (loud) ...
        out.mtd[row] = m;
        out.maskf[row] = mk;
        if constexpr (Sel::on) { if (out.targets) out.targets[row] = target; }
        if (!q.ok && out.bad) atomicAdd(out.bad, 1);                            // ... and is counted for vdn_td_forward's caller
        sq = m * m;
        mks = mk;
    }
    if (out.sums) td_block_sums(sq, mks, out.part, out.sums);
}
template <class Index>
__global__ __launch_bounds__(256) void k_td_forward(const Index ix, const TdIn in, const TdOut out) {
    td_forward_rows(ix, in, out, NoSel{}, blockIdx.x * blockDim.x + threadIdx.x);
}

// one thread per row of grad_q: agent i of Q-tensor unit row / n, then the zero rows behind the last unit (GEMM-friendly padding of
// the packed learn)
template <class Index>
__global__ __launch_bounds__(256) void k_td_backward(const Index ix, const float *__restrict__ mtd, const float *__restrict__ maskf,
                                                     const int8_t *__restrict__ u, const float *__restrict__ g, long rows, int n, int A,
                                                     float *__restrict__ gq) {
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows + ix.pad_rows) return;
    if (row >= rows) {
        for (int a = 0; a < A; ++a) gq[row * A + a] = 0.0f;
        return;
    }
    const int i = (int)(row % n);
    const UnitOf s = ix.unit(row / n);
    const float d = -((2.0f * mtd[s.row]) * maskf[s.row]) * g[0];
    const int a_taken = (int)u[s.ep * n + i];  // outside [0, A): mtd is NaN for the slot, so d is NaN: keep it visible
    const bool bad_a = (unsigned)a_taken >= (unsigned)A;
    for (int a = 0; a < A; ++a) gq[row * A + a] = (bad_a || a == a_taken) ? d : 0.0f;
}

// dst unit j = src unit units[j] + shift (zeros for j < zero_below): coalesced copies of whole units (n rows of the replay tensors)
template <typename V>
__global__ __launch_bounds__(256) void k_gather_units(const V *__restrict__ src, int unit_v, const int32_t *__restrict__ units, int U, int shift,
                                                      int zero_below, V *__restrict__ dst) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)U * unit_v) return;
    const int j = (int)(idx / unit_v), k = (int)(idx - (long)j * unit_v);
    dst[idx] = j < zero_below ? (V)0 : src[((size_t)units[j] + shift) * unit_v + k];
}

// up to VDN_GATHER_MAX gathers over ONE unit list in one launch (blockIdx.y = descriptor); words behind the last unit up to the
// destination's size are zero-filled
struct GatherBatch {
    const void *src[VDN_GATHER_MAX];
    void *dst[VDN_GATHER_MAX];
    long total[VDN_GATHER_MAX], total_pad[VDN_GATHER_MAX];   // words of the U units / of the whole destination
    int unit_v[VDN_GATHER_MAX], shift[VDN_GATHER_MAX], zero_below[VDN_GATHER_MAX], dw[VDN_GATHER_MAX];
    int vec[VDN_GATHER_MAX];   // the destination's start is aligned to four words: one store for a thread's four
    int narrow;                // every total_pad + 4 fits 31 bits: 32-bit index arithmetic
};
template <typename V> struct Four;
template <> struct Four<uint32_t> { typedef uint4 type; };
template <> struct Four<uint8_t> { typedef uchar4 type; };
// a thread moves the four destination words idx0 .. idx0 + 3: ONE division, then (unit, word in unit) stepped along (four words may
// straddle units; a unit may be shorter than four words), the four source loads issued before the first store
template <typename V, typename I>
__device__ __forceinline__ void gather_four(const void *src, int unit_v, const int32_t *__restrict__ units, int shift, int zero_below,
                                            void *dst, bool vec, I total, I total_pad, I idx0) {
    V v[4] = {(V)0, (V)0, (V)0, (V)0};
    if (idx0 < total) {   // else: the zero tail behind the last unit (and no unit at all: `units` may be empty)
        // Loads without branches, so that the four unit numbers and then the four words are in flight together: a word that is not
        // copied (behind the last unit, or below zero_below) reads units[0] / src[0] and is replaced by zero.
        I j = idx0 / (I)unit_v, k = idx0 - j * (I)unit_v;
        bool on[4];
        I kk[4];
        int un[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            on[w] = idx0 + (I)w < total && (long)j >= (long)zero_below;
            kk[w] = k;
            un[w] = units[on[w] ? j : (I)0];
            if (++k == (I)unit_v) { k = 0; ++j; }
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const V x = ((const V *)src)[on[w] ? ((size_t)un[w] + shift) * unit_v + kk[w] : (size_t)0];
            v[w] = on[w] ? x : (V)0;
        }
    }
    if (vec && idx0 + (I)3 < total_pad) {
        typename Four<V>::type o;
        o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
        *(typename Four<V>::type *)((V *)dst + idx0) = o;
    } else {
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (idx0 + (I)w < total_pad) ((V *)dst)[idx0 + (I)w] = v[w];
    }
}
__global__ __launch_bounds__(256) void k_gather_units_batch(GatherBatch gb, const int32_t *__restrict__ units) {
    const int d = blockIdx.y;
    const long idx0 = 4 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
    if (idx0 >= gb.total_pad[d]) return;
    const bool vec = gb.vec[d] != 0;
    if (gb.narrow) {
        const uint32_t t = (uint32_t)gb.total[d], tp = (uint32_t)gb.total_pad[d], i0 = (uint32_t)idx0;
        if (gb.dw[d]) gather_four<uint32_t, uint32_t>(gb.src[d], gb.unit_v[d], units, gb.shift[d], gb.zero_below[d], gb.dst[d], vec, t, tp, i0);
        else gather_four<uint8_t, uint32_t>(gb.src[d], gb.unit_v[d], units, gb.shift[d], gb.zero_below[d], gb.dst[d], vec, t, tp, i0);
    } else {
        if (gb.dw[d]) gather_four<uint32_t, long>(gb.src[d], gb.unit_v[d], units, gb.shift[d], gb.zero_below[d], gb.dst[d], vec, gb.total[d], gb.total_pad[d], idx0);
        else gather_four<uint8_t, long>(gb.src[d], gb.unit_v[d], units, gb.shift[d], gb.zero_below[d], gb.dst[d], vec, gb.total[d], gb.total_pad[d], idx0);
    }
}

}  // namespace

#include "vdn_lambda_kernels.h"   // the TD block on lambda-returns (include/vdn_lambda.h); uses td_block_sums above
#include "vdn_double_kernels.h"   // both with double-Q targets (include/vdn_double.h): four kernel shells with QSel

namespace {

// ---- clip_grad_norm_ + Adam over a list of tensors (include/vdn_ops.h)
struct TensorList {
    float *p[VDN_MAX_TENSORS];
    float *g[VDN_MAX_TENSORS];
    float *m[VDN_MAX_TENSORS];
    float *v[VDN_MAX_TENSORS];
    long off[VDN_MAX_TENSORS + 1];  // prefix sums of the element counts
    int n;
};

// element i of the concatenation -> (tensor k, index inside it); i only grows along a thread's walk, so k is carried along
__device__ __forceinline__ void locate(const TensorList &tl, long i, int &k) {
    while (i >= tl.off[k + 1]) ++k;
}
constexpr int kFly = 4;   // elements of a thread whose loads are in flight together (the headline's trip count is four or five)

__global__ __launch_bounds__(256) void k_sqnorm_partials(TensorList tl, float *__restrict__ partials, const float *__restrict__ grad_div) {
    __shared__ float s_w[4];
    const long total = tl.off[tl.n];
    const long per = (total + gridDim.x - 1) / gridDim.x;
    const long lo = (long)blockIdx.x * per, hi = min(total, lo + per);
    const bool div = grad_div != nullptr;
    const float gd = div ? grad_div[0] : 1.0f;
    float acc = 0.0f;
    int k = 0;
    // a thread's elements lo + tid, + 256, ... in that order, as one fma chain; kFly of them are loaded before the chain goes on
    for (long i = lo + threadIdx.x; i < hi; i += 256 * kFly) {
        float g[kFly];
#pragma unroll
        for (int s = 0; s < kFly; ++s) {
            const long e = i + 256 * s;
            g[s] = 0.0f;
            if (e < hi) {
                locate(tl, e, k);
                g[s] = tl.g[k][e - tl.off[k]];
            }
        }
#pragma unroll
        for (int s = 0; s < kFly; ++s)
            if (i + 256 * s < hi) {
                const float x = div ? g[s] / gd : g[s];
                acc = fmaf(x, x, acc);
            }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

__global__ __launch_bounds__(256) void k_clip_adam(TensorList tl, const float *__restrict__ partials, int n_partials, float max_norm,
                                                   float step_size, float omb1, float beta2, float omb2, float eps, float bc2_sqrt,
                                                   float *__restrict__ total_norm, const float *__restrict__ grad_div) {
    __shared__ float s_coef;
    const int tid = threadIdx.x;
    const long total = tl.off[tl.n];
    const long per = (total + gridDim.x - 1) / gridDim.x;
    const long lo = (long)blockIdx.x * per, hi = min(total, lo + per);
    const bool div = grad_div != nullptr;
    // requested before anything waits: the first wave's two partial sums, the divisor, and every thread's first kFly elements
    float x0 = 0.0f, x1 = 0.0f;
    if (tid < 64) {
        if (tid < n_partials) x0 = partials[tid];
        if (tid + 64 < n_partials) x1 = partials[tid + 64];
    }
    const float gd = div ? grad_div[0] : 1.0f;
    struct El { float *g, *m, *v, *p; float gv, mv, vv, pv; };
    El el[kFly];
    int k = 0;
    auto fetch = [&](long i) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < kFly; ++s) {
            const long e = i + 256 * s;
            if (e < hi) {
                locate(tl, e, k);
                const long j = e - tl.off[k];
                el[s].g = tl.g[k] + j; el[s].m = tl.m[k] + j; el[s].v = tl.v[k] + j; el[s].p = tl.p[k] + j;
                el[s].gv = *el[s].g; el[s].mv = *el[s].m; el[s].vv = *el[s].v; el[s].pv = *el[s].p;
            }
        }
    };
    fetch(lo + tid);
    if (tid < 64) {  // every workgroup adds the partial sums in the same fixed order
        float t = 0.0f;
        if (tid < n_partials) t += x0;
        if (tid + 64 < n_partials) t += x1;
        for (int b = tid + 128; b < n_partials; b += 64) t += partials[b];
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if (threadIdx.x == 0) {
            const float norm = sqrtf(t);
            // clamp(max_norm / (norm + 1e-6), max = 1) of clip_grad_norm_; a NaN norm stays NaN in every gradient, as in torch
            s_coef = norm != norm ? norm : fminf(max_norm / (norm + 1e-6f), 1.0f);
            if (blockIdx.x == 0) total_norm[0] = norm;
        }
    }
    __syncthreads();
    const float coef = s_coef;
    // a thread's elements lo + tid, + 256, ...: kFly at a time, every load of a batch (above for the first) ahead of its arithmetic
    for (long i = lo + tid; i < hi; i += 256 * kFly) {
        if (i != lo + tid) fetch(i);
#pragma unroll
        for (int s = 0; s < kFly; ++s) {
            if (i + 256 * s >= hi) continue;
            float g = el[s].gv;
            if (div) g = g / gd;  // the gradient of the un-normalised loss / the (global) mask count
            g = g * coef;
            if (div || coef != 1.0f) *el[s].g = g;  // clip_grad_norm_ leaves the rescaled gradient in p.grad
            float m = el[s].mv, v = el[s].vv;
            m = m + omb1 * (g - m);
            v = beta2 * v + omb2 * g * g;
            *el[s].m = m;
            *el[s].v = v;
            // torch's element arithmetic (foreach and fused Adam alike): float operations, the Python-double scalars rounded to float
            // where they enter: denom = sqrt(v) / sqrt(bias_correction2) + eps;  p += -step_size * (m / denom)   (addcdiv)
            const float denom = sqrtf(v) / bc2_sqrt + eps;
            *el[s].p = el[s].pv - step_size * (m / denom);
        }
    }
}

// ---- host side of the TD block: one argument rule for the forward entry points, one for the backward ones
bool td_forward_args_ok(const TdIn &in, const TdOut &out) {
    return !(out.sums && !out.part) && in.qe && in.qt && in.u && in.r && in.avail && in.term && in.padded && out.mtd && out.maskf && in.n >= 1 &&
           in.A >= 1 && in.A <= 127;
}
bool td_backward_args_ok(const float *mtd, const float *mask, const int8_t *u, const float *g, const float *gq, int n, int A) {
    return mtd && mask && u && g && gq && n >= 1 && A >= 1 && A <= 127;
}
bool padded_shape_ok(int B, int T, int Tl) { return B >= 0 && T >= 1 && Tl >= T; }

// no row at all: the sums are zero, nothing else is written
int td_no_rows(const TdOut &out, void *stream) {
    if (out.sums) HIP_TRY(hipMemsetAsync(out.sums, 0, 2 * sizeof(float), (hipStream_t)stream));
    return VDN_OK;
}

// ---- the argument rules of the lambda entry points (include/vdn_lambda.h), shared with the double-Q ones (include/vdn_double.h)
bool lambda_padded_args_ok(const TdIn &in, const TdOut &out, int B, int T, int Tl, float lam) {
    return td_forward_args_ok(in, out) && padded_shape_ok(B, T, Tl) && T <= VDN_LAMBDA_MAX_T && lambda_ok(lam) &&
           (int64_t)B * T <= 0x7fffffffL;
}
bool lambda_packed_args_ok(const TdIn &in, const TdOut &out, const int32_t *units, int n_units, float lam, int n_steps) {
    return td_forward_args_ok(in, out) && units && n_units >= 0 && lambda_ok(lam) && n_steps >= 0 && n_steps <= VDN_LAMBDA_MAX_T;
}
template <class Index>
int td_forward(const Index &ix, int rows, const TdIn &in, const TdOut &out, void *stream) {
    if (rows == 0) return td_no_rows(out, stream);
    LAUNCH((k_td_forward<Index>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ix, in, out);
    return VDN_OK;
}

template <class Index>
int td_backward(const Index &ix, const float *mtd, const float *mask, const int8_t *u, const float *g, long rows, int n, int A, float *gq,
                void *stream) {
    const long rows_pad = rows + ix.pad_rows;
    if (rows_pad == 0) return VDN_OK;
    LAUNCH((k_td_backward<Index>), dim3((unsigned)((rows_pad + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ix, mtd, mask, u, g, rows, n, A, gq);
    return VDN_OK;
}

}  // namespace

extern "C" {

int vdn_clip_adam_step(int32_t n_tensors, float *const *params, float *const *grads, float *const *exp_avg,
                       float *const *exp_avg_sq, const int64_t *numel, float max_norm, double lr, double beta1, double beta2,
                       double eps, double bias_correction1, double bias_correction2, float *d_partials, float *d_total_norm,
                       const float *d_grad_div, void *stream) {
    if (n_tensors < 1 || n_tensors > VDN_MAX_TENSORS || !params || !grads || !exp_avg || !exp_avg_sq || !numel || !d_partials ||
        !d_total_norm || !(bias_correction1 > 0.0) || !(bias_correction2 > 0.0))
        return VDN_ERR_BAD_ARG;
    TensorList tl;
    tl.n = n_tensors;
    tl.off[0] = 0;
    for (int k = 0; k < VDN_MAX_TENSORS; ++k) {
        const bool on = k < n_tensors;
        if (on && (!params[k] || !grads[k] || !exp_avg[k] || !exp_avg_sq[k] || numel[k] < 1)) return VDN_ERR_BAD_ARG;
        tl.p[k] = on ? params[k] : nullptr;
        tl.g[k] = on ? grads[k] : nullptr;
        tl.m[k] = on ? exp_avg[k] : nullptr;
        tl.v[k] = on ? exp_avg_sq[k] : nullptr;
        tl.off[k + 1] = tl.off[k] + (on ? (long)numel[k] : 0);
    }
    HIP_TRY(launch_status([&] {
        hipLaunchKernelGGL(k_sqnorm_partials, dim3(VDN_NORM_BLOCKS), dim3(256), 0, (hipStream_t)stream, tl, d_partials, d_grad_div);
        const long total = tl.off[n_tensors];
        const int blocks = (int)((total + 1023) / 1024 < 1024 ? (total + 1023) / 1024 : 1024);
        hipLaunchKernelGGL(k_clip_adam, dim3(blocks), dim3(256), 0, (hipStream_t)stream, tl, d_partials, VDN_NORM_BLOCKS, max_norm,
                           (float)((double)lr / bias_correction1), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps,
                           (float)sqrt(bias_correction2), d_total_norm, d_grad_div);
    }));
    return VDN_OK;
}


int vdn_td_sum_parts(int64_t n_slots) { return n_slots < 1 ? 2 : (int)(2 * ((n_slots + 255) / 256)); }

int vdn_td_forward_sums(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r,
                        const int8_t *d_avail_next, const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T,
                        int32_t t_limit, int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd, float *d_mask,
                        int32_t *d_bad_actions, float *d_part, float *d_sums, void *stream) {
    const TdIn in{d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded, n_agents, n_actions, gamma};
    const TdOut out{d_mtd, d_mask, nullptr, d_bad_actions, d_part, d_sums};
    if (!td_forward_args_ok(in, out) || !padded_shape_ok(B, T, t_limit)) return VDN_ERR_BAD_ARG;
    return td_forward(PaddedIndex{B, T, t_limit}, B * T, in, out, stream);
}

int vdn_td_forward(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r,
                   const int8_t *d_avail_next, const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T,
                   int32_t t_limit, int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd, float *d_mask, int32_t *d_bad_actions,
                   void *stream) {
    return vdn_td_forward_sums(d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded, B, T, t_limit, n_agents, n_actions,
                               gamma, d_mtd, d_mask, d_bad_actions, nullptr, nullptr, stream);
}

int vdn_td_backward(const float *d_mtd, const float *d_mask, const int8_t *d_u, const float *d_grad_num, int32_t B, int32_t T,
                    int32_t t_limit, int32_t n_agents, int32_t n_actions, float *d_grad_q, void *stream) {
    if (!td_backward_args_ok(d_mtd, d_mask, d_u, d_grad_num, d_grad_q, n_agents, n_actions) || !padded_shape_ok(B, T, t_limit))
        return VDN_ERR_BAD_ARG;
    const long rows = (long)T * B * n_agents;
    return td_backward(PaddedIndex{B, T, t_limit}, d_mtd, d_mask, d_u, d_grad_num, rows, n_agents, n_actions, d_grad_q, stream);
}

int vdn_td_forward_packed_sums(const float *d_q_eval, const float *d_q_target, const int32_t *d_units, int32_t n_units,
                               const int8_t *d_u, const float *d_r, const int8_t *d_avail_next, const uint8_t *d_terminated,
                               const uint8_t *d_padded, int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd, float *d_mask,
                               int32_t *d_bad_actions, float *d_part, float *d_sums, void *stream) {
    const TdIn in{d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded, n_agents, n_actions, gamma};
    const TdOut out{d_mtd, d_mask, nullptr, d_bad_actions, d_part, d_sums};
    if (!td_forward_args_ok(in, out) || !d_units || n_units < 0) return VDN_ERR_BAD_ARG;
    return td_forward(PackedIndex{d_units, n_units, 0, nullptr}, n_units, in, out, stream);
}

int vdn_td_forward_packed(const float *d_q_eval, const float *d_q_target, const int32_t *d_units, int32_t n_units, const int8_t *d_u,
                          const float *d_r, const int8_t *d_avail_next, const uint8_t *d_terminated, const uint8_t *d_padded,
                          int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd, float *d_mask, int32_t *d_bad_actions,
                          void *stream) {
    return vdn_td_forward_packed_sums(d_q_eval, d_q_target, d_units, n_units, d_u, d_r, d_avail_next, d_terminated, d_padded, n_agents,
                                      n_actions, gamma, d_mtd, d_mask, d_bad_actions, nullptr, nullptr, stream);
}

int vdn_td_backward_packed_pad(const float *d_mtd, const float *d_mask, const int32_t *d_units, int32_t n_units, const int8_t *d_u,
                               const float *d_grad_num, int32_t n_agents, int32_t n_actions, int64_t rows_pad, float *d_grad_q,
                               void *stream) {
    if (!td_backward_args_ok(d_mtd, d_mask, d_u, d_grad_num, d_grad_q, n_agents, n_actions) || !d_units || n_units < 0 ||
        rows_pad < (int64_t)n_units * n_agents)
        return VDN_ERR_BAD_ARG;
    const long rows = (long)n_units * n_agents;
    return td_backward(PackedIndex{d_units, n_units, (long)rows_pad - rows, nullptr}, d_mtd, d_mask, d_u, d_grad_num, rows, n_agents, n_actions,
                       d_grad_q, stream);
}

int vdn_td_backward_packed(const float *d_mtd, const float *d_mask, const int32_t *d_units, int32_t n_units, const int8_t *d_u,
                           const float *d_grad_num, int32_t n_agents, int32_t n_actions, float *d_grad_q, void *stream) {
    return vdn_td_backward_packed_pad(d_mtd, d_mask, d_units, n_units, d_u, d_grad_num, n_agents, n_actions, (int64_t)n_units * n_agents,
                                      d_grad_q, stream);
}

// ---- the TD block on lambda-returns (include/vdn_lambda.h; kernels in vdn_lambda_kernels.h)
int vdn_td_lambda_sum_parts(int64_t n_episodes) {
    return n_episodes < 1 ? 2 : (int)(2 * ((n_episodes + VDN_LAMBDA_WG_EPISODES - 1) / VDN_LAMBDA_WG_EPISODES));
}

int vdn_td_lambda_forward_sums(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r,
                               const int8_t *d_avail_next, const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T,
                               int32_t t_limit, int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd, float *d_mask,
                               int32_t *d_bad_actions, float *d_part, float *d_sums, float lam, float *d_targets, void *stream) {
    const TdIn in{d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded, n_agents, n_actions, gamma};
    const TdOut out{d_mtd, d_mask, d_targets, d_bad_actions, d_part, d_sums};
    if (!lambda_padded_args_ok(in, out, B, T, t_limit, lam)) return VDN_ERR_BAD_ARG;
    if (B == 0) return td_no_rows(out, stream);
    LAUNCH(k_td_lambda_forward, dim3((unsigned)((B + VDN_LAMBDA_WG_EPISODES - 1) / VDN_LAMBDA_WG_EPISODES)), dim3(256), 0,
           (hipStream_t)stream, PaddedIndex{B, T, t_limit}, in, lam, out);
    return VDN_OK;
}

int vdn_td_lambda_forward_packed_sums(const float *d_q_eval, const float *d_q_target, const int32_t *d_units, int32_t n_units,
                                      const int8_t *d_u, const float *d_r, const int8_t *d_avail_next, const uint8_t *d_terminated,
                                      const uint8_t *d_padded, int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd,
                                      float *d_mask, int32_t *d_bad_actions, float *d_part, float *d_sums, float lam, float *d_targets,
                                      int32_t n_steps, const int32_t *counts, void *stream) {
    const TdIn in{d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded, n_agents, n_actions, gamma};
    const TdOut out{d_mtd, d_mask, d_targets, d_bad_actions, d_part, d_sums};
    LambdaOff lo;
    if (!lambda_packed_args_ok(in, out, d_units, n_units, lam, n_steps) || !lambda_offsets(n_units, n_steps, counts, lo))
        return VDN_ERR_BAD_ARG;
    if (n_units == 0) return td_no_rows(out, stream);
    const int E = counts[0];
    LAUNCH(k_td_lambda_forward_packed, dim3((unsigned)((E + VDN_LAMBDA_WG_EPISODES - 1) / VDN_LAMBDA_WG_EPISODES)), dim3(256), 0,
           (hipStream_t)stream, PackedIndex{d_units, n_units, 0, nullptr}, E, n_steps, in, lam, out, lo);
    return VDN_OK;
}

// ---- both TD blocks with double-Q targets (include/vdn_double.h; kernels in vdn_double_kernels.h)
int vdn_td_double_forward_sums(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r,
                               const int8_t *d_avail_next, const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T,
                               int32_t t_limit, int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd, float *d_mask,
                               int32_t *d_bad_actions, float *d_part, float *d_sums, float lam, float *d_targets, const float *d_q_sel,
                               int8_t *d_picks, void *stream) {
    const TdIn in{d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded, n_agents, n_actions, gamma};
    const TdOut out{d_mtd, d_mask, d_targets, d_bad_actions, d_part, d_sums};
    if (!lambda_padded_args_ok(in, out, B, T, t_limit, lam) || !d_q_sel) return VDN_ERR_BAD_ARG;
    if (B == 0) return td_no_rows(out, stream);
    const PaddedIndex ix{B, T, t_limit};
    const QSel sel{d_q_sel, nullptr, 0, d_picks};
    if (lam == 0.0f)
        LAUNCH((k_td_double_forward<PaddedIndex>), dim3((unsigned)((B * T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ix, in, out, sel);
    else
        LAUNCH(k_td_double_lambda_forward, dim3((unsigned)((B + VDN_LAMBDA_WG_EPISODES - 1) / VDN_LAMBDA_WG_EPISODES)), dim3(256), 0,
               (hipStream_t)stream, ix, in, lam, out, sel);
    return VDN_OK;
}

int vdn_td_double_forward_packed_sums(const float *d_q_eval, const float *d_q_target, const int32_t *d_units, int32_t n_units,
                                      const int8_t *d_u, const float *d_r, const int8_t *d_avail_next, const uint8_t *d_terminated,
                                      const uint8_t *d_padded, int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd,
                                      float *d_mask, int32_t *d_bad_actions, float *d_part, float *d_sums, float lam, float *d_targets,
                                      int32_t n_steps, const int32_t *counts, const float *d_q_sel, int32_t n_sel_units,
                                      const int32_t *d_sel_units, int8_t *d_picks, void *stream) {
    const TdIn in{d_q_eval, d_q_target, d_u, d_r, d_avail_next, d_terminated, d_padded, n_agents, n_actions, gamma};
    const TdOut out{d_mtd, d_mask, d_targets, d_bad_actions, d_part, d_sums};
    if (!lambda_packed_args_ok(in, out, d_units, n_units, lam, n_steps) || !d_q_sel || n_sel_units < 1 ||
        (!d_sel_units && n_sel_units < n_units))
        return VDN_ERR_BAD_ARG;
    LambdaOff lo;
    if (lam > 0.0f && !lambda_offsets(n_units, n_steps, counts, lo)) return VDN_ERR_BAD_ARG;
    if (n_units == 0) return td_no_rows(out, stream);
    const PackedIndex ix{d_units, n_units, 0, nullptr};
    const QSel sel{d_q_sel, d_sel_units, n_sel_units, d_picks};
    if (lam == 0.0f) {
        LAUNCH((k_td_double_forward<PackedIndex>), dim3((unsigned)((n_units + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ix, in, out, sel);
    } else {
        const int E = counts[0];
        LAUNCH(k_td_double_lambda_forward_packed, dim3((unsigned)((E + VDN_LAMBDA_WG_EPISODES - 1) / VDN_LAMBDA_WG_EPISODES)), dim3(256), 0,
               (hipStream_t)stream, ix, E, n_steps, in, lam, out, lo, sel);
    }
    return VDN_OK;
}

int vdn_gather_units(const void *d_src, int32_t unit_bytes, const int32_t *d_units, int32_t n_units, int32_t unit_shift,
                     int32_t zero_below, void *d_dst, void *stream) {
    if (!d_src || !d_units || !d_dst || unit_bytes < 1 || n_units < 0 || zero_below < 0) return VDN_ERR_BAD_ARG;
    if (n_units == 0) return VDN_OK;
    HIP_TRY(launch_status([&] {
        const bool dw = unit_bytes % 4 == 0 && ((size_t)d_src | (size_t)d_dst) % 4 == 0;
        const int uv = dw ? unit_bytes / 4 : unit_bytes;
        const long total = (long)n_units * uv;
        if (dw)
            hipLaunchKernelGGL((k_gather_units<uint32_t>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                               (const uint32_t *)d_src, uv, d_units, n_units, unit_shift, zero_below, (uint32_t *)d_dst);
        else
            hipLaunchKernelGGL((k_gather_units<uint8_t>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                               (const uint8_t *)d_src, uv, d_units, n_units, unit_shift, zero_below, (uint8_t *)d_dst);
    }));
    return VDN_OK;
}

int vdn_gather_units_batch(int32_t n_gathers, const void *const *d_src, const int32_t *unit_bytes, const int32_t *unit_shift,
                           const int32_t *zero_below, void *const *d_dst, const int64_t *dst_bytes, const int32_t *d_units,
                           int32_t n_units, void *stream) {
    if (n_gathers < 1 || n_gathers > VDN_GATHER_MAX || !d_src || !unit_bytes || !unit_shift || !zero_below || !d_dst || !dst_bytes ||
        !d_units || n_units < 0)
        return VDN_ERR_BAD_ARG;
    GatherBatch gb{};
    long most = 0;
    for (int i = 0; i < n_gathers; ++i) {
        if (!d_src[i] || !d_dst[i] || unit_bytes[i] < 1 || zero_below[i] < 0 || dst_bytes[i] < (int64_t)n_units * unit_bytes[i])
            return VDN_ERR_BAD_ARG;
        const bool dw = unit_bytes[i] % 4 == 0 && dst_bytes[i] % 4 == 0 && ((size_t)d_src[i] | (size_t)d_dst[i]) % 4 == 0;
        gb.src[i] = d_src[i];
        gb.dst[i] = d_dst[i];
        gb.dw[i] = dw ? 1 : 0;
        gb.unit_v[i] = dw ? unit_bytes[i] / 4 : unit_bytes[i];
        gb.total[i] = (long)n_units * gb.unit_v[i];
        gb.total_pad[i] = (long)(dw ? dst_bytes[i] / 4 : dst_bytes[i]);
        gb.shift[i] = unit_shift[i];
        gb.zero_below[i] = zero_below[i];
        gb.vec[i] = (size_t)d_dst[i] % (dw ? 16 : 4) == 0 ? 1 : 0;
        most = gb.total_pad[i] > most ? gb.total_pad[i] : most;
    }
    if (most == 0) return VDN_OK;
    gb.narrow = most + 4 <= 0x7fffffffL ? 1 : 0;
    const long threads = (most + 3) / 4;   // four destination words (bytes) per thread
    if ((threads + 255) / 256 > 0x7fffffffL) return VDN_ERR_BAD_ARG;
    LAUNCH(k_gather_units_batch, dim3((unsigned)((threads + 255) / 256), (unsigned)n_gathers), dim3(256), 0, (hipStream_t)stream, gb, d_units);
    return VDN_OK;
}

int vdn_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
