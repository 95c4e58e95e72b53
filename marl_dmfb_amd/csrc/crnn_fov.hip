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
// keeps its weight-gradient sums in registers and writes them once; k_front_fov_bwd_reduce adds the partial vectors in a fixed
// order (deterministic, no atomics).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/crnn_fov.h"

#define HIP_ABI_TAG "crnn_fov"
#define HIP_ABI_ERR CRNN_FOV_ERR_HIP
#include "hip_abi.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlockF = 256;  // forward: 4 waves = (channel half nh = wave & 1, position parity sub = wave >> 1)
constexpr int kRB = 16;       // rows per forward block: lane j of a tile = row j
constexpr int kVec = 18;      // dir_x, dir_y, one-hot (<= 16) per row
constexpr int kMlp = 10 * kVec + 10;

template <int FOV, int OD> struct GeoF {
    static constexpr bool TWO = FOV == 7;             // conv2 follows conv1
    static constexpr int NPIX = 3 * FOV * FOV;        // 147 / 75 pixel bytes (odd: the 16 row lanes of a gather hit 16 banks)
    static constexpr int S1 = FOV - 2;                // conv1 output side: 5 / 3
    static constexpr int P1 = S1 * S1;
    static constexpr int NFEAT = OD * 9;              // 3 x 3 output positions
    static constexpr int PAD_COLS = (NFEAT + 10 + 63) / 64 * 64;  // 256 / 320
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
        // ---- stream the staged rows out: a wave per row, consecutive lanes on consecutive 16-byte chunks
        if (quad_out) {
            for (int rr = wave; rr < rv; rr += kBlockF / 64) {
                float4 *dst = (float4 *)(out + (row0 + rr) * out_stride);
                const float4 *src = (const float4 *)(s_out + rr * G::OUT_STRIDE);
                for (int k = lane; k < n_out / 4; k += 64) dst[k] = src[k];
            }
        } else {
            for (int rr = wave; rr < rv; rr += kBlockF / 64) {
                float *dst = out + (row0 + rr) * out_stride;
                const float *src = s_out + rr * G::OUT_STRIDE;
                for (int k = lane; k < n_out; k += 64) dst[k] = src[k];
            }
        }
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
    if constexpr (G::TWO)
        for (int i = tid; i < OD * OD * 9; i += kBlockB) s_w2[i] = w2[i];
    for (int i = tid; i < OD * 27; i += kBlockB) s_w1[i] = w1[i];
    if (tid < OD) s_w1[OD * 27 + tid] = b1[tid];

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
        for (int i = tid; i < G::RB * G::NPIX; i += kBlockB) {
            const int r = i / G::NPIX, b = i - r * G::NPIX;
            s_x[i] = r < rv ? (float)obs[(row0 + r) * obs_stride + b] : 0.0f;
        }
        for (int i = tid; i < G::RB * G::NDZ; i += kBlockB) {
            const int r = i / G::NDZ, c = i - r * G::NDZ;
            s_dz[i] = (r < rv && y[(row0 + r) * y_stride + c] > 0.0f) ? g[(row0 + r) * g_stride + c] : 0.0f;
        }
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

// grads[i] = sum over the partial vectors b = 0, 1, ... of part[b][i]: one thread per output, fixed order (deterministic)
__global__ __launch_bounds__(256) void k_front_fov_bwd_reduce(const float *__restrict__ part, int n_part, int n, float *__restrict__ grads) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float a0 = 0.0f, a1 = 0.0f;
    int b = 0;
    for (; b + 1 < n_part; b += 2) { a0 += part[(size_t)b * n + i]; a1 += part[(size_t)(b + 1) * n + i]; }
    if (b < n_part) a0 += part[(size_t)b * n + i];
    grads[i] = a0 + a1;
}

template <int FOV, int OD>
int launch_fwd(const int8_t *obs, long obs_stride, long rows, const float *w1, const float *b1, const float *w2, const float *b2,
               float *out, long out_stride, int out_cols, const int8_t *onehot, int n_actions, const float *mlp_w, const float *mlp_b,
               hipStream_t s) {
    using G = GeoF<FOV, OD>;
    const size_t lds = G::LDS_FLOATS * sizeof(float);
    static LdsLimit lds_limit;
    if (const int rc = lds_limit.raise((const void *)k_front_fov<FOV, OD>, lds)) return rc;
    const long n_blocks = (rows + kRB - 1) / kRB;
    // persistent: as many workgroups as the 256 CUs hold at once (LDS-limited), the weights stay in registers
    const long resident = 256L * (long)((size_t)160 * 1024 / lds);
    const int grid = (int)(n_blocks < resident ? n_blocks : resident);
    LAUNCH((k_front_fov<FOV, OD>), dim3(grid), dim3(kBlockF), lds, s, obs, obs_stride, rows, w1, b1, w2, b2, out, out_stride, out_cols,
           onehot, n_actions, mlp_w, mlp_b);
    return CRNN_FOV_OK;
}

template <int FOV, int OD>
int launch_bwd(const int8_t *obs, long obs_stride, long rows, const float *y, long y_stride, const float *g, long g_stride,
               const float *w1, const float *b1, const float *w2, float *part, int n_part, float *grads, hipStream_t s) {
    using G = GeoBF<FOV, OD>;
    const size_t lds = G::LDS_FLOATS * sizeof(float);
    static LdsLimit lds_limit;
    if (const int rc = lds_limit.raise((const void *)k_front_fov_bwd<FOV, OD>, lds)) return rc;
    const long n_blocks = (rows + G::RB - 1) / G::RB;
    const int grid = (int)(n_blocks < n_part ? n_blocks : n_part);
    HIP_TRY(launch_status([&] {
        hipLaunchKernelGGL((k_front_fov_bwd<FOV, OD>), dim3(grid), dim3(kBlockB), lds, s, obs, obs_stride, rows, y, y_stride, g, g_stride,
                           w1, b1, w2, part);
        hipLaunchKernelGGL(k_front_fov_bwd_reduce, dim3((G::GRADS + 255) / 256), dim3(256), 0, s, part, grid, G::GRADS, grads);
    }));
    return CRNN_FOV_OK;
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
    const bool vec = d_mlp_w != nullptr;
    const int n_feat = od * 9 + (vec ? 10 : 0);
    if (!d_obs || !d_w1 || !d_b1 || (fov == 7 && (!d_w2 || !d_b2)) || !d_out || rows < 0 || obs_stride < 3 * fov * fov + (vec ? 2 : 0) ||
        out_stride < n_feat || n_actions < 0 || n_actions > 16 || (vec && !d_mlp_b))
        return CRNN_FOV_ERR_BAD_ARG;
    if (out_cols != 0 && (out_cols < n_feat || out_cols > crnn_fov_padded_cols(fov, od) || out_cols > out_stride)) return CRNN_FOV_ERR_BAD_ARG;
    if (rows == 0) return CRNN_FOV_OK;
    hipStream_t s = (hipStream_t)stream;
#define FWD(F, O) launch_fwd<F, O>(d_obs, obs_stride, rows, d_w1, d_b1, d_w2, d_b2, d_out, out_stride, out_cols, d_onehot, n_actions, d_mlp_w, d_mlp_b, s)
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
    if (!d_obs || !d_out || !d_grad_out || !d_w1 || !d_b1 || (fov == 7 && !d_w2) || !d_part || !d_grads || rows <= 0 || n_part < 1 ||
        n_part > 256 || obs_stride < 3 * fov * fov || out_stride < od * 9 || grad_stride < od * 9)
        return CRNN_FOV_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
#define BWD(F, O) launch_bwd<F, O>(d_obs, obs_stride, rows, d_out, out_stride, d_grad_out, grad_stride, d_w1, d_b1, d_w2, d_part, n_part, d_grads, s)
    if (fov == 7) return od == 24 ? BWD(7, 24) : BWD(7, 32);
    return od == 24 ? BWD(5, 24) : BWD(5, 32);
#undef BWD
}

int crnn_fov_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
