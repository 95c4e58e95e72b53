// crnn_fov.hip -- HIP front end of the reference's CRNN (network/base_net.py:23-71) for fov 5 and 7, hand-written for gfx950.
// See include/crnn_fov.h.
//
// Forward (k_front_fov): blocks of 16 rows.  Both convolutions are GEMMs on the matrix cores with f32 operands
// (v_mfma_f32_16x16x4_f32: an exact f32 fma chain), tiled as the ROWLANE geometry of crnn_mfma.h: the 16 M entries of a tile
// are the 16 ROWS of the block at ONE output position (9 output positions per row would not fill a 16-wide tile), N is a
// 16-channel half, K the (input channel, tap) pairs.  The B operands (weights of the lane's output channel) stay in registers
// for the whole persistent kernel.  A row's output (conv features | vector branch | zero tail) is staged in LDS and streamed
// out with 16-byte stores, a wave per row.
//   fov 7: ~126 kFLOP per row (od 24) against ~1.2 KB of traffic: matrix-core bound.  conv1 7x7->5x5 into LDS, conv2 5x5->3x3.
//   fov 5: ~12 kFLOP per row against ~1.1 KB: bound by the fp32 output write.  One conv (7 MFMAs per tile); the workgroup
//          needs at most 27 KB of LDS and 96 VGPRs, so four of them share a CU and one's MFMAs overlap another's store stream.
// Backward (k_front_fov_bwd): one persistent workgroup per partial vector walks a contiguous range of row blocks; every thread
// keeps its weight-gradient sums in registers and writes them once; crnn_front::k_front_bwd_reduce adds the partial vectors in a
// fixed order (deterministic, no atomics).
// Shared with the other front-end files through crnn_front.h: the constants of the vector branch, the stream-out, the LDS staging
// of the backward, the reduce kernel, the launchers and the argument contracts.  The rest of the forward kernel keeps its own lines:
// with the shared helpers it measured slower at fov 7 / od 32 (profiles/crnn_front/NOTES.md).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/crnn_fov.h"

#define HIP_ABI_TAG "crnn_fov"
#define HIP_ABI_ERR CRNN_FOV_ERR_HIP
#include "hip_abi.h"
#include "crnn_front.h"

namespace {

using crnn_front::kVec;
using crnn_front::kMlp;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlockF = 256;  // forward: 4 waves = (channel half nh = wave & 1, position parity sub = wave >> 1)
constexpr int kRB = 16;       // rows per forward block: lane j of a tile = row j

template <int FOV, int OD> struct GeoF {
    static constexpr bool TWO = FOV == 7;             // conv2 follows conv1
    static constexpr int NPIX = 3 * FOV * FOV;        // 147 / 75 pixel bytes (odd: the 16 row lanes of a gather hit 16 banks)
    static constexpr int S1 = FOV - 2;                // conv1 output side: 5 / 3
    static constexpr int P1 = S1 * S1;
    static constexpr int NFEAT = OD * 9;              // 3 x 3 output positions
    static constexpr int PAD_COLS = crnn_front::padded_cols(NFEAT);  // 256 / 320
    static constexpr int OUT_STRIDE = PAD_COLS + 4;   // staged output row (16-byte multiple)
    static constexpr int ROW_A1 = OD * 25 + 1;        // conv1 activations of a row (fov 7), odd
    static constexpr int KQ = OD / 4;                 // channel quads: conv2 K steps = KQ * 9
    static constexpr size_t LDS_FLOATS = (size_t)kRB * NPIX + (TWO ? (size_t)kRB * ROW_A1 : 0) + (size_t)kRB * OUT_STRIDE +
                                         (size_t)kRB * kVec + kMlp;
    static_assert((kRB * NPIX) % 4 == 0 && (kRB * ROW_A1) % 4 == 0, "s_out must stay 16-byte aligned");
};

template <int FOV, int OD>
__global__ __launch_bounds__(kBlockF) void k_front_fov(const int8_t *__restrict__ obs, long obs_stride, long rows,
                                                       const float *__restrict__ w1, const float *__restrict__ b1,
                                                       const float *__restrict__ w2, const float *__restrict__ b2,
                                                       float *__restrict__ out, long out_stride, int out_cols,
                                                       const int8_t *__restrict__ onehot, int n_actions,
                                                       const float *__restrict__ mlp_w, const float *__restrict__ mlp_b) {
    using G = GeoF<FOV, OD>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *s_in = lds;                                          // [16][NPIX] float image of the pixel bytes
    float *s_a1 = s_in + kRB * G::NPIX;                         // [16][ROW_A1] conv1 activations (fov 7)
    float *s_out = s_a1 + (G::TWO ? kRB * G::ROW_A1 : 0);       // [16][OUT_STRIDE] staged output rows
    float *s_vec = s_out + kRB * G::OUT_STRIDE;                 // [16][18] inputs of the vector branch
    float *s_mlp = s_vec + kRB * kVec;                          // [10][nin] weights, then [10] biases
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nh = wave & 1, sub = __builtin_amdgcn_readfirstlane(wave >> 1);
    const int j = lane & 15, kq = lane >> 4;
    const int ch = nh * 16 + j;                                 // this lane's B / D column
    const bool chv = ch < OD;
    const int nin = 2 + n_actions;

    if (mlp_w) {
        for (int i = tid; i < 10 * nin; i += kBlockF) s_mlp[i] = mlp_w[i];
        if (tid < 10) s_mlp[10 * kVec + tid] = mlp_b[tid];
    }
    // B operands: conv1 K = 27 (+1 zero) in 7 steps, lane k = 4 s + kq; conv2 K = (channel quad, tap), lane channel 4 cq + kq
    float bw1[7];
    int off1[7];
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        const int k = 4 * s + kq;
        const bool kv = k < 27;
        bw1[s] = (chv && kv) ? w1[ch * 27 + k] : 0.0f;
        const int c0 = k / 9, tap = k - c0 * 9;
        off1[s] = kv ? c0 * FOV * FOV + (tap / 3) * FOV + tap % 3 : 0;  // k = 27: zero weight, any valid address
    }
    float bw2[G::TWO ? G::KQ * 9 : 1];
    float bias2 = 0.0f;
    if constexpr (G::TWO) {
#pragma unroll
        for (int cq = 0; cq < G::KQ; ++cq)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) bw2[cq * 9 + tap] = chv ? w2[(ch * OD + 4 * cq + kq) * 9 + tap] : 0.0f;
        bias2 = chv ? b2[ch] : 0.0f;
    }
    const float bias1 = chv ? b1[ch] : 0.0f;
    const int n_feat = G::NFEAT + (mlp_w ? 10 : 0);
    const int n_out = out_cols > n_feat ? out_cols : n_feat;   // columns n_feat .. n_out-1 are zeros
    const bool quad_out = (out_stride % 4 == 0) && (((size_t)out) % 16 == 0) && (n_out % 4 == 0);
    for (int i = tid; i < kRB * (G::OUT_STRIDE - n_feat); i += kBlockF) {  // the zero tail of every staged row, once
        const int rr = i / (G::OUT_STRIDE - n_feat), k = i - rr * (G::OUT_STRIDE - n_feat);
        s_out[rr * G::OUT_STRIDE + n_feat + k] = 0.0f;
    }
    const int rowb = G::NPIX + (mlp_w ? 2 : 0);   // bytes read per row: the direction bytes only with the vector branch
    const long n_blocks = (rows + kRB - 1) / kRB;

    for (long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const long row0 = blk * kRB;
        const int rv = (int)min((long)kRB, rows - row0);
        __syncthreads();   // the previous block's stream-out and gathers are done with s_out / s_in / s_vec
        for (int i = tid; i < kRB * rowb; i += kBlockF) {
            const int r = i / rowb, b = i - r * rowb;
            const float v = r < rv ? (float)obs[(row0 + r) * obs_stride + b] : 0.0f;   // rows past the end: finite zeros
            if (b < G::NPIX) s_in[r * G::NPIX + b] = v;
            else s_vec[r * kVec + b - G::NPIX] = v;
        }
        if (mlp_w) {
            for (int i = tid; i < kRB * 16; i += kBlockF) {
                const int r = i >> 4, a = i & 15;
                s_vec[r * kVec + 2 + a] = (r < rv && onehot && a < n_actions) ? (float)onehot[(row0 + r) * n_actions + a] : 0.0f;
            }
        }
        __syncthreads();
        // ---- conv1: wave `sub` of a channel half takes the positions sub, sub + 2, ...; two tiles per pass
        {
            float *dst = G::TWO ? s_a1 : s_out;
            constexpr int RS = G::TWO ? G::ROW_A1 : G::OUT_STRIDE, CS = G::TWO ? 25 : 9;
            const int jb = j * G::NPIX;
#pragma unroll
            for (int m = 0; m < (G::P1 + 1) / 2; m += 2) {
                const int pa = sub + 2 * m, pb = pa + 2;
                if (pa < G::P1) {   // wave-uniform
                    const bool two = pb < G::P1;
                    const int oa = (pa / G::S1) * FOV + pa % G::S1, ob = two ? (pb / G::S1) * FOV + pb % G::S1 : oa;
                    float va[7], vb[7];
#pragma unroll
                    for (int s = 0; s < 7; ++s) { va[s] = s_in[jb + off1[s] + oa]; vb[s] = s_in[jb + off1[s] + ob]; }
                    f32x4 acc_a = {bias1, bias1, bias1, bias1}, acc_b = acc_a;
#pragma unroll
                    for (int s = 0; s < 7; ++s) {
                        acc_a = __builtin_amdgcn_mfma_f32_16x16x4f32(va[s], bw1[s], acc_a, 0, 0, 0);
                        acc_b = __builtin_amdgcn_mfma_f32_16x16x4f32(vb[s], bw1[s], acc_b, 0, 0, 0);
                    }
                    if (chv) {   // D row 4 kq + q = block row
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            dst[(kq * 4 + q) * RS + ch * CS + pa] = fmaxf(acc_a[q], 0.0f);
                            if (two) dst[(kq * 4 + q) * RS + ch * CS + pb] = fmaxf(acc_b[q], 0.0f);
                        }
                    }
                }
            }
        }
        // ---- vector branch relu(mlp1([dir_x, dir_y, last-action one-hot])) (base_net.py:66): thread (row, output)
        if (mlp_w && tid < kRB * 10) {
            const int mr = tid / 10, mc = tid - mr * 10;
            float mv = s_mlp[10 * kVec + mc];
            for (int k = 0; k < nin; ++k) mv = fmaf(s_vec[mr * kVec + k], s_mlp[mc * nin + k], mv);
            s_out[mr * G::OUT_STRIDE + G::NFEAT + mc] = fmaxf(mv, 0.0f);
        }
        // ---- conv2 (fov 7): 9 output positions, K = od * 9; the gathers of channel quad cq + 1 are issued before the MFMAs of cq
        if constexpr (G::TWO) {
            __syncthreads();
#pragma unroll
            for (int m = 0; m < 5; m += 2) {
                const int pa = sub + 2 * m, pb = pa + 2;
                if (pa < 9) {   // wave-uniform
                    const bool two = pb < 9;
                    const float *ap = s_a1 + j * G::ROW_A1 + kq * 25 + (pa / 3) * 5 + pa % 3;
                    const float *bp = s_a1 + j * G::ROW_A1 + kq * 25 + (two ? (pb / 3) * 5 + pb % 3 : (pa / 3) * 5 + pa % 3);
                    f32x4 acc_a = {bias2, bias2, bias2, bias2}, acc_b = acc_a;
                    float va[2][9], vb[2][9];
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) { va[0][tap] = ap[(tap / 3) * 5 + tap % 3]; vb[0][tap] = bp[(tap / 3) * 5 + tap % 3]; }
#pragma unroll
                    for (int cq = 0; cq < G::KQ; ++cq) {
                        if (cq + 1 < G::KQ) {
#pragma unroll
                            for (int tap = 0; tap < 9; ++tap) {
                                va[(cq + 1) & 1][tap] = ap[(cq + 1) * 100 + (tap / 3) * 5 + tap % 3];
                                vb[(cq + 1) & 1][tap] = bp[(cq + 1) * 100 + (tap / 3) * 5 + tap % 3];
                            }
                        }
#pragma unroll
                        for (int tap = 0; tap < 9; ++tap) {
                            acc_a = __builtin_amdgcn_mfma_f32_16x16x4f32(va[cq & 1][tap], bw2[cq * 9 + tap], acc_a, 0, 0, 0);
                            acc_b = __builtin_amdgcn_mfma_f32_16x16x4f32(vb[cq & 1][tap], bw2[cq * 9 + tap], acc_b, 0, 0, 0);
                        }
                    }
                    if (chv) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            s_out[(kq * 4 + q) * G::OUT_STRIDE + ch * 9 + pa] = fmaxf(acc_a[q], 0.0f);
                            if (two) s_out[(kq * 4 + q) * G::OUT_STRIDE + ch * 9 + pb] = fmaxf(acc_b[q], 0.0f);
                        }
                    }
                }
            }
        }
        __syncthreads();
        // ---- stream the staged rows out, with 16-byte or 4-byte stores (no 8-byte path)
        crnn_front::stream_rows_out<kBlockF>(s_out, G::OUT_STRIDE, out, out_stride, row0, rv, n_out, quad_out, false, wave, lane);
    }
}

// ---- backward w.r.t. the conv parameters.  Thread roles (256 threads):
//   fov 7, per block of RB = 8 rows:
//     A  a1[r][c1][25] = relu(conv1) recomputed, thread (r, c1)
//     B  dW2[c2][c1][tap] += sum_pos dz2[c2][pos] a1[c1][pos + tap], thread = (c2, c1) pairs; db2 thread c2;
//        da1[r][c1][.] = sum_c2,tap dz2[c2][. - tap] W2[c2][c1][tap], thread (r, c1)
//     C  dz1 = da1 * (a1 > 0) written over a1
//     D  dW1[c1][c0][tap] += sum_pos dz1[c1][pos] in[c0][pos + tap], thread = (c1, c0, tap) items; db1 thread c1
//   fov 5, per block of RB = 32 rows: D only, with dz1 = g * (out > 0) over the 3x3 positions.
constexpr int kBlockB = 256;

template <int FOV, int OD> struct GeoBF {
    static constexpr bool TWO = FOV == 7;
    static constexpr int NPIX = 3 * FOV * FOV;
    static constexpr int S1 = FOV - 2;
    static constexpr int RB = TWO ? 8 : 32;
    static constexpr int NDZ = OD * 9;                              // gradient at the stack's output, per row
    static constexpr int N2 = TWO ? OD * OD * 9 + OD : 0;           // dW2 | db2
    static constexpr int GRADS = N2 + OD * 27 + OD;                 // ... | dW1 | db1: also the partial vector's length
    static constexpr int NPAIR = TWO ? (OD * OD + kBlockB - 1) / kBlockB : 1;   // (c2, c1) pairs per thread: 3 / 4
    static constexpr int NITEM = (OD * 27 + kBlockB - 1) / kBlockB;            // (c1, c0, tap) items per thread: 3 / 4
    static_assert(!TWO || RB * OD <= kBlockB, "one thread per (row, channel)");
    static constexpr size_t LDS_FLOATS = (TWO ? (size_t)OD * OD * 9 : 0) + (size_t)OD * 28 + (size_t)RB * NPIX + (size_t)RB * NDZ +
                                         (TWO ? (size_t)RB * OD * 25 : 0);
};

template <int FOV, int OD>
__global__ __launch_bounds__(kBlockB) void k_front_fov_bwd(const int8_t *__restrict__ obs, long obs_stride, long rows,
                                                           const float *__restrict__ y, long y_stride, const float *__restrict__ g,
                                                           long g_stride, const float *__restrict__ w1, const float *__restrict__ b1,
                                                           const float *__restrict__ w2, float *__restrict__ part) {
    using G = GeoBF<FOV, OD>;
    constexpr int F2 = FOV * FOV;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *s_w2 = lds;                                       // [c2][c1][9] (fov 7)
    float *s_w1 = s_w2 + (G::TWO ? OD * OD * 9 : 0);         // [c1][27], then [od] biases
    float *s_x = s_w1 + OD * 28;                             // [RB][NPIX]
    float *s_dz = s_x + G::RB * G::NPIX;                     // [RB][od][9]: upstream gradient through the last ReLU
    float *s_a1 = s_dz + G::RB * G::NDZ;                     // [RB][od][25]: a1, then dz1 (fov 7)
    const int tid = threadIdx.x;
    crnn_front::stage_bwd_weights<kBlockB, OD, G::TWO>(s_w2, s_w1, w2, w1, b1, tid);

    float acc2[G::NPAIR][9], acc1[G::NITEM], accb2 = 0.0f, accb1 = 0.0f;
#pragma unroll
    for (int i = 0; i < G::NPAIR; ++i)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc2[i][k] = 0.0f;
#pragma unroll
    for (int i = 0; i < G::NITEM; ++i) acc1[i] = 0.0f;
    const int rc_r = tid / OD, rc_c = tid - rc_r * OD;       // (row, channel) role

    const long n_blocks = (rows + G::RB - 1) / G::RB;
    const long per = (n_blocks + gridDim.x - 1) / gridDim.x;
    const long blk0 = (long)blockIdx.x * per, blk1 = min(n_blocks, blk0 + per);
    for (long blk = blk0; blk < blk1; ++blk) {
        const long row0 = blk * G::RB;
        const int rv = (int)min((long)G::RB, rows - row0);
        __syncthreads();
        crnn_front::stage_bwd_rows<kBlockB, G::RB, G::NPIX, G::NDZ>(s_x, s_dz, obs, obs_stride, y, y_stride, g, g_stride, row0, rv, tid);
        __syncthreads();
        if constexpr (G::TWO) {
            // A: conv1 + ReLU of (row rc_r, channel rc_c), taps in the order of the forward's K (c0, kx, ky)
            const bool rc_on = tid < G::RB * OD && rc_r < rv;
            if (rc_on) {
                float a[25];
                const float bias = s_w1[OD * 27 + rc_c];
#pragma unroll
                for (int p = 0; p < 25; ++p) a[p] = bias;
                const float *xin = s_x + rc_r * G::NPIX;
#pragma unroll 1
                for (int c0 = 0; c0 < 3; ++c0)
#pragma unroll
                    for (int t = 0; t < 9; ++t) {
                        const float w = s_w1[rc_c * 27 + c0 * 9 + t];
#pragma unroll
                        for (int p = 0; p < 25; ++p) a[p] = fmaf(xin[c0 * 49 + (p / 5 + t / 3) * 7 + p % 5 + t % 3], w, a[p]);
                    }
                float *dst = s_a1 + (rc_r * OD + rc_c) * 25;
#pragma unroll
                for (int p = 0; p < 25; ++p) dst[p] = fmaxf(a[p], 0.0f);
            }
            __syncthreads();
            // B: dW2, db2
#pragma unroll
            for (int i = 0; i < G::NPAIR; ++i) {
                const int u = tid + i * kBlockB;
                if (u < OD * OD) {
                    const int c2 = u / OD, c1 = u - c2 * OD;
#pragma unroll 1
                    for (int r = 0; r < rv; ++r) {
                        float dz[9], a[25];
#pragma unroll
                        for (int k = 0; k < 9; ++k) dz[k] = s_dz[r * G::NDZ + c2 * 9 + k];
#pragma unroll
                        for (int k = 0; k < 25; ++k) a[k] = s_a1[(r * OD + c1) * 25 + k];
#pragma unroll
                        for (int t = 0; t < 9; ++t)
#pragma unroll
                            for (int p = 0; p < 9; ++p) acc2[i][t] = fmaf(dz[p], a[(p / 3 + t / 3) * 5 + p % 3 + t % 3], acc2[i][t]);
                    }
                }
            }
            if (tid < OD)
                for (int r = 0; r < rv; ++r)
#pragma unroll
                    for (int p = 0; p < 9; ++p) accb2 += s_dz[r * G::NDZ + tid * 9 + p];
            // da1 of (row rc_r, channel rc_c): a transposed convolution in scatter form over the 9 output positions
            float da[25];
#pragma unroll
            for (int p = 0; p < 25; ++p) da[p] = 0.0f;
            if (rc_on) {
#pragma unroll 1
                for (int c2 = 0; c2 < OD; ++c2) {
                    float dz[9], w[9];
#pragma unroll
                    for (int k = 0; k < 9; ++k) { dz[k] = s_dz[rc_r * G::NDZ + c2 * 9 + k]; w[k] = s_w2[(c2 * OD + rc_c) * 9 + k]; }
#pragma unroll
                    for (int t = 0; t < 9; ++t)
#pragma unroll
                        for (int p = 0; p < 9; ++p) {
                            float &d = da[(p / 3 + t / 3) * 5 + p % 3 + t % 3];
                            d = fmaf(dz[p], w[t], d);
                        }
                }
            }
            __syncthreads();   // every reader of a1 (dW2) is done
            // C: dz1 = da1 * (a1 > 0) in place; rows past the end stay zero from A's absence: write zeros
            if (tid < G::RB * OD) {
                float *a1 = s_a1 + (rc_r * OD + rc_c) * 25;
#pragma unroll
                for (int p = 0; p < 25; ++p) a1[p] = (rc_on && a1[p] > 0.0f) ? da[p] : 0.0f;
            }
            __syncthreads();
        }
        // D: dW1, db1 from dz1 (fov 7: s_a1, 5x5; fov 5: s_dz, 3x3)
        constexpr int S1 = G::S1, P1 = S1 * S1;
        const float *dz1 = G::TWO ? s_a1 : s_dz;
#pragma unroll
        for (int i = 0; i < G::NITEM; ++i) {
            const int v = tid + i * kBlockB;
            if (v < OD * 27) {
                const int c1 = v / 27, k = v - c1 * 27, c0 = k / 9, kx = (k - c0 * 9) / 3, ky = k % 3;
#pragma unroll 1
                for (int r = 0; r < rv; ++r) {
                    const float *d = dz1 + (r * OD + c1) * P1;
                    const float *xin = s_x + r * G::NPIX + c0 * F2 + kx * FOV + ky;
#pragma unroll
                    for (int p = 0; p < P1; ++p) acc1[i] = fmaf(d[p], xin[(p / S1) * FOV + p % S1], acc1[i]);
                }
            }
        }
        if (tid < OD)
            for (int r = 0; r < rv; ++r)
#pragma unroll
                for (int p = 0; p < P1; ++p) accb1 += dz1[(r * OD + tid) * P1 + p];
    }
    float *pp = part + (size_t)blockIdx.x * G::GRADS;
    if constexpr (G::TWO) {
#pragma unroll
        for (int i = 0; i < G::NPAIR; ++i) {
            const int u = tid + i * kBlockB;
            if (u < OD * OD)
#pragma unroll
                for (int t = 0; t < 9; ++t) pp[u * 9 + t] = acc2[i][t];
        }
        if (tid < OD) pp[OD * OD * 9 + tid] = accb2;
    }
#pragma unroll
    for (int i = 0; i < G::NITEM; ++i) {
        const int v = tid + i * kBlockB;
        if (v < OD * 27) pp[G::N2 + v] = acc1[i];
    }
    if (tid < OD) pp[G::N2 + OD * 27 + tid] = accb1;
}

bool supported(int fov, int od) { return (fov == 5 || fov == 7) && (od == 24 || od == 32); }

}  // namespace

extern "C" {

int crnn_fov_padded_cols(int fov, int od) {
    if (!supported(fov, od)) return CRNN_FOV_ERR_UNSUPPORTED;
    return od == 24 ? GeoF<7, 24>::PAD_COLS : GeoF<7, 32>::PAD_COLS;
}

int crnn_fov_front_forward(int fov, const int8_t *d_obs, int64_t obs_stride, const int8_t *d_onehot, int n_actions, int64_t rows,
                           const float *d_w1, const float *d_b1, const float *d_w2, const float *d_b2, const float *d_mlp_w,
                           const float *d_mlp_b, int od, float *d_out, int64_t out_stride, int out_cols, void *stream) {
    if (!supported(fov, od)) return CRNN_FOV_ERR_UNSUPPORTED;
    if (!crnn_front::forward_args_ok(3 * fov * fov, od * 9, crnn_fov_padded_cols(fov, od), fov == 7, d_obs, obs_stride, n_actions, rows, d_w1,
                                     d_b1, d_w2, d_b2, d_mlp_w, d_mlp_b, d_out, out_stride, out_cols))
        return CRNN_FOV_ERR_BAD_ARG;
    if (rows == 0) return CRNN_FOV_OK;
    hipStream_t s = (hipStream_t)stream;
    // persistent: as many workgroups as the 256 CUs hold at once (LDS-limited), the weights stay in registers
#define FWD(F, O)                                                                                                                    \
    crnn_front::launch_forward<k_front_fov<F, O>, GeoF<F, O>, kBlockF>(                                                              \
        crnn_front::grid_resident((rows + kRB - 1) / kRB, GeoF<F, O>::LDS_FLOATS * sizeof(float)), d_obs, obs_stride, rows, d_w1, d_b1, \
        d_w2, d_b2, d_out, out_stride, out_cols, d_onehot, n_actions, d_mlp_w, d_mlp_b, s)
    if (fov == 7) return od == 24 ? FWD(7, 24) : FWD(7, 32);
    return od == 24 ? FWD(5, 24) : FWD(5, 32);
#undef FWD
}

int crnn_fov_backward_parts(int fov, int od) {
    if (!supported(fov, od)) return CRNN_FOV_ERR_UNSUPPORTED;
    if (fov == 7) return od == 24 ? GeoBF<7, 24>::GRADS : GeoBF<7, 32>::GRADS;
    return od == 24 ? GeoBF<5, 24>::GRADS : GeoBF<5, 32>::GRADS;
}

int crnn_fov_backward(int fov, const int8_t *d_obs, int64_t obs_stride, int64_t rows, const float *d_out, int64_t out_stride,
                      const float *d_grad_out, int64_t grad_stride, const float *d_w1, const float *d_b1, const float *d_w2,
                      int od, float *d_part, int n_part, float *d_grads, void *stream) {
    if (!supported(fov, od)) return CRNN_FOV_ERR_UNSUPPORTED;
    if (!crnn_front::backward_args_ok(3 * fov * fov, od * 9, fov == 7, d_obs, obs_stride, rows, d_out, out_stride, d_grad_out, grad_stride, d_w1,
                                      d_b1, d_w2, d_part, n_part, d_grads))
        return CRNN_FOV_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
#define BWD(F, O)                                                                                                                \
    crnn_front::launch_backward<k_front_fov_bwd<F, O>, GeoBF<F, O>, kBlockB>(d_obs, obs_stride, rows, d_out, out_stride, d_grad_out, \
                                                                             grad_stride, d_w1, d_b1, d_w2, d_part, n_part, d_grads, s)
    if (fov == 7) return od == 24 ? BWD(7, 24) : BWD(7, 32);
    return od == 24 ? BWD(5, 24) : BWD(5, 32);
#undef BWD
}

int crnn_fov_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
