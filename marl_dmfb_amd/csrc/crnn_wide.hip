// crnn_wide.hip -- HIP front end of the reference's CRNN (network/base_net.py:23-71) for fov 11 and 13, hand-written for gfx950.
// See include/crnn_wide.h.
//
// Forward (k_front_wide): blocks of RB rows (5 .. 8, what 160 KiB of LDS hold).  Both convolutions are GEMMs on the matrix cores
// with f32 operands (v_mfma_f32_16x16x4_f32: an exact f32 fma chain), tiled as the fov-9 / fov-19 kernels of crnn_mfma.h /
// crnn_mfma19.h: the 16 M entries of a tile are 16 consecutive (row, output position) pairs of the block, N is a 16-channel half,
// K the (input channel, tap) pairs.  Eight waves = (channel half, tile quarter); the B operands (weights of the lane's output
// channel) stay in registers for the whole persistent kernel.  conv1 writes its activations to LDS, conv2 gathers them from there
// and stages the output row (conv features | vector branch | zero tail), which is streamed out with 16-byte stores, a wave per row.
//   fov 11: 11x11 -> 9x9 -> 7x7, 613 / 1043 kFLOP per row (od 24 / 32);  fov 13: 13x13 -> 11x11 -> 9x9, 997 / 1702 kFLOP per row.
// Backward (k_front_wide_bwd): the VALU scheme of crnn_fov.hip for fov 7 with the positions of a (row, channel) split over
// threads: one persistent workgroup per partial vector walks a contiguous range of 4-row blocks; every thread keeps its
// weight-gradient sums in registers and writes them once; crnn_front::k_front_bwd_reduce adds the partial vectors in a fixed order
// (deterministic, no atomics).
// What is neither tiling nor the vector branch's fmas (mlp1 parameters, B operands, zero tail, stream-out, input staging, reduce
// kernel, launchers, argument contracts): crnn_front.h.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/crnn_wide.h"

#define HIP_ABI_TAG "crnn_wide"
#define HIP_ABI_ERR CRNN_WIDE_ERR_HIP
#include "hip_abi.h"
#include "crnn_front.h"

namespace {

using crnn_front::kVec;
using crnn_front::kMlp;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlockF = 512;  // forward: 8 waves = (channel half nh = wave & 1, tile quarter sub = wave >> 1)
constexpr int kSub = 4;

template <int FOV, int OD> struct GeoW {
    static constexpr int NPIX = 3 * FOV * FOV;        // 363 / 507 pixel bytes (odd)
    static constexpr int S1 = FOV - 2, P1 = S1 * S1;  // conv1 output: 9x9 / 11x11
    static constexpr int S2 = FOV - 4, P2 = S2 * S2;  // conv2 output: 7x7 / 9x9
    static constexpr int NFEAT = OD * P2;
    static constexpr int PAD_COLS = crnn_front::padded_cols(NFEAT);
    static constexpr int OUT_STRIDE = PAD_COLS + 4;   // staged output row (16-byte multiple)
    static constexpr int ROW_A1 = OD * P1 + 1;        // conv1 activations of a row, odd (OD * P1 is even)
    static constexpr int KQ = OD / 4;                 // channel quads: conv2 K steps = KQ * 9
    // rows per block: the most that fit 160 KiB next to the staged rows (fov 11: 8; fov 13: 7 / 5)
    static constexpr int RB = FOV == 11 ? 8 : (OD == 24 ? 7 : 5);
    static constexpr int T1 = (RB * P1 + 15) / 16, T2 = (RB * P2 + 15) / 16;   // M tiles of conv1 / conv2
    static constexpr size_t LDS_FLOATS = (size_t)RB * OUT_STRIDE + (size_t)RB * NPIX + (size_t)RB * ROW_A1 + (size_t)RB * kVec + kMlp;
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "a workgroup holds at most 160 KiB of LDS");
    static_assert(RB * 10 <= kBlockF, "one thread per (row, vector feature)");
};

template <int FOV, int OD>
__global__ __launch_bounds__(kBlockF) void k_front_wide(const int8_t *__restrict__ obs, long obs_stride, long rows,
                                                        const float *__restrict__ w1, const float *__restrict__ b1,
                                                        const float *__restrict__ w2, const float *__restrict__ b2,
                                                        float *__restrict__ out, long out_stride, int out_cols,
                                                        const int8_t *__restrict__ onehot, int n_actions,
                                                        const float *__restrict__ mlp_w, const float *__restrict__ mlp_b) {
    using G = GeoW<FOV, OD>;
    constexpr int RB = G::RB, S1 = G::S1, P1 = G::P1, S2 = G::S2, P2 = G::P2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *s_out = lds;                                         // [RB][OUT_STRIDE] staged output rows (16-byte aligned)
    float *s_in = s_out + RB * G::OUT_STRIDE;                   // [RB][NPIX] float image of the pixel bytes
    float *s_a1 = s_in + RB * G::NPIX;                          // [RB][ROW_A1] conv1 activations, (c, h, w)
    float *s_vec = s_a1 + RB * G::ROW_A1;                       // [RB][18] inputs of the vector branch
    float *s_mlp = s_vec + RB * kVec;                           // [10][nin] weights, then [10] biases
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nh = wave & 1, sub = __builtin_amdgcn_readfirstlane(wave >> 1);
    const int j = lane & 15, kq = lane >> 4;
    const int ch = nh * 16 + j;                                 // this lane's B / D column
    const bool chv = ch < OD;
    const int nin = 2 + n_actions;

    crnn_front::stage_mlp_params<kBlockF>(s_mlp, mlp_w, mlp_b, nin, tid);
    // B operands, in registers for the whole kernel
    float bw1[7], bw2[G::KQ * 9];
    int off1[7];
    crnn_front::load_conv1_b<FOV>(bw1, off1, w1, ch, chv, kq);
    crnn_front::load_conv2_b<OD>(bw2, w2, ch, chv, kq);
    const float bias1 = chv ? b1[ch] : 0.0f, bias2 = chv ? b2[ch] : 0.0f;
    const int n_feat = G::NFEAT + (mlp_w ? 10 : 0);
    const int n_out = out_cols > n_feat ? out_cols : n_feat;   // columns n_feat .. n_out-1 are zeros
    const bool quad_out = (out_stride % 4 == 0) && (((size_t)out) % 16 == 0) && (n_out % 4 == 0);
    crnn_front::zero_tail<kBlockF, RB, G::OUT_STRIDE>(s_out, n_feat, G::OUT_STRIDE, tid);   // of every staged row, once
    const long n_blocks = (rows + RB - 1) / RB;

    for (long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const long row0 = blk * RB;
        const int rv = (int)min((long)RB, rows - row0);
        __syncthreads();   // the previous block's stream-out and gathers are done with s_out / s_in / s_a1 / s_vec
        crnn_front::stage_obs_rows<kBlockF, RB, G::NPIX>(s_in, s_vec, obs, obs_stride, onehot, n_actions, mlp_w != nullptr, row0, rv, tid);
        __syncthreads();
        // ---- conv1: tile t holds the (row, position) pairs 16 t .. 16 t + 15 of the block; wave `sub` of a channel half takes the
        // tiles sub, sub + 4, ..., two per pass.  Entries behind the last pair repeat it and are not stored.
#pragma unroll 1
        for (int t = sub; t < G::T1; t += 2 * kSub) {
            const int tb = t + kSub < G::T1 ? t + kSub : t;   // wave-uniform; tb == t: the second tile is a repeat, not stored
            const int ma = min(t * 16 + j, RB * P1 - 1), mb = min(tb * 16 + j, RB * P1 - 1);
            const int ra = ma / P1, pa = ma - ra * P1, rb = mb / P1, pb = mb - rb * P1;
            const int oa = ra * G::NPIX + (pa / S1) * FOV + pa % S1, ob = rb * G::NPIX + (pb / S1) * FOV + pb % S1;
            float va[7], vb[7];
#pragma unroll
            for (int s = 0; s < 7; ++s) { va[s] = s_in[oa + off1[s]]; vb[s] = s_in[ob + off1[s]]; }
            f32x4 acc_a = {bias1, bias1, bias1, bias1}, acc_b = acc_a;
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                acc_a = __builtin_amdgcn_mfma_f32_16x16x4f32(va[s], bw1[s], acc_a, 0, 0, 0);
                acc_b = __builtin_amdgcn_mfma_f32_16x16x4f32(vb[s], bw1[s], acc_b, 0, 0, 0);
            }
            if (chv) {   // D row 4 kq + q = tile entry
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int da = t * 16 + kq * 4 + q, db = tb * 16 + kq * 4 + q;
                    if (da < RB * P1) s_a1[(da / P1) * G::ROW_A1 + ch * P1 + da % P1] = fmaxf(acc_a[q], 0.0f);
                    if (tb != t && db < RB * P1) s_a1[(db / P1) * G::ROW_A1 + ch * P1 + db % P1] = fmaxf(acc_b[q], 0.0f);
                }
            }
        }
        // ---- vector branch relu(mlp1([dir_x, dir_y, last-action one-hot])) (base_net.py:66): thread (row, output)
        if (mlp_w && tid < RB * 10) {
            const int mr = tid / 10, mc = tid - mr * 10;
            float mv = s_mlp[10 * kVec + mc];
            for (int k = 0; k < nin; ++k) mv = fmaf(s_vec[mr * kVec + k], s_mlp[mc * nin + k], mv);
            s_out[mr * G::OUT_STRIDE + G::NFEAT + mc] = fmaxf(mv, 0.0f);
        }
        __syncthreads();
        // ---- conv2: K = od * 9; the gathers of channel quad cq + 1 are issued before the MFMAs of cq
#pragma unroll 1
        for (int t = sub; t < G::T2; t += 2 * kSub) {
            const int tb = t + kSub < G::T2 ? t + kSub : t;
            const int ma = min(t * 16 + j, RB * P2 - 1), mb = min(tb * 16 + j, RB * P2 - 1);
            const int ra = ma / P2, pa = ma - ra * P2, rb = mb / P2, pb = mb - rb * P2;
            const float *ap = s_a1 + ra * G::ROW_A1 + kq * P1 + (pa / S2) * S1 + pa % S2;
            const float *bp = s_a1 + rb * G::ROW_A1 + kq * P1 + (pb / S2) * S1 + pb % S2;
            f32x4 acc_a = {bias2, bias2, bias2, bias2}, acc_b = acc_a;
            float va[2][9], vb[2][9];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) { va[0][tap] = ap[(tap / 3) * S1 + tap % 3]; vb[0][tap] = bp[(tap / 3) * S1 + tap % 3]; }
#pragma unroll
            for (int cq = 0; cq < G::KQ; ++cq) {
                if (cq + 1 < G::KQ) {
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) {
                        va[(cq + 1) & 1][tap] = ap[(cq + 1) * 4 * P1 + (tap / 3) * S1 + tap % 3];
                        vb[(cq + 1) & 1][tap] = bp[(cq + 1) * 4 * P1 + (tap / 3) * S1 + tap % 3];
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
                    const int da = t * 16 + kq * 4 + q, db = tb * 16 + kq * 4 + q;
                    if (da < RB * P2) s_out[(da / P2) * G::OUT_STRIDE + ch * P2 + da % P2] = fmaxf(acc_a[q], 0.0f);
                    if (tb != t && db < RB * P2) s_out[(db / P2) * G::OUT_STRIDE + ch * P2 + db % P2] = fmaxf(acc_b[q], 0.0f);
                }
            }
        }
        __syncthreads();
        // ---- stream the staged rows out, with 16-byte or 4-byte stores (no 8-byte path)
        crnn_front::stream_rows_out<kBlockF>(s_out, G::OUT_STRIDE, out, out_stride, row0, rv, n_out, quad_out, false, wave, lane);
    }
}

// ---- backward w.r.t. the conv parameters.  Thread roles (512 threads), per block of RB = 4 rows:
//   A  a1[r][c1][P1] = relu(conv1) recomputed, items (r, c1, position) strided over the threads
//   B  dW2[c2][c1][tap] += sum_pos dz2[c2][pos] a1[c1][pos + tap], thread = (c2, c1) pairs; db2 thread c2 (last wave);
//      da1[r][c1][y][.] = sum_c2,tap dz2[c2][y - kh][. - kw] W2[c2][c1][tap] in gather form, thread = (r, c1, y) items: one line
//      of S1 positions in registers
//   C  dz1 = da1 * (a1 > 0) written over a1
//   D  dW1[c1][c0][tap] += sum_pos dz1[c1][pos] in[c0][pos + tap], thread = (c1, c0, tap) items; db1 thread c1 (last wave)
constexpr int kBlockB = 512;

template <int FOV, int OD> struct GeoWB {
    static constexpr int NPIX = 3 * FOV * FOV;
    static constexpr int S1 = FOV - 2, P1 = S1 * S1, S2 = FOV - 4, P2 = S2 * S2;
    static constexpr int RB = 4;
    static constexpr int NDZ = OD * P2;                            // gradient at the stack's output, per row
    static constexpr int NA1 = OD * P1;                            // conv1 activations, per row
    static constexpr int N2 = OD * OD * 9 + OD;                    // dW2 | db2
    static constexpr int GRADS = N2 + OD * 27 + OD;                // ... | dW1 | db1: also the partial vector's length
    static constexpr int NPAIR = (OD * OD + kBlockB - 1) / kBlockB;        // (c2, c1) pairs per thread: 2
    static constexpr int NITEM = (OD * 27 + kBlockB - 1) / kBlockB;        // (c1, c0, tap) items per thread: 2
    static constexpr int NLINE = (RB * OD * S1 + kBlockB - 1) / kBlockB;   // (r, c1, y) lines of da1 per thread: 2 / 3
    static constexpr size_t LDS_FLOATS = (size_t)OD * OD * 9 + (size_t)OD * 28 + (size_t)RB * (NPIX + NDZ + NA1);
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "a workgroup holds at most 160 KiB of LDS");
};

template <int FOV, int OD>
__global__ __launch_bounds__(kBlockB) void k_front_wide_bwd(const int8_t *__restrict__ obs, long obs_stride, long rows,
                                                            const float *__restrict__ y, long y_stride, const float *__restrict__ g,
                                                            long g_stride, const float *__restrict__ w1, const float *__restrict__ b1,
                                                            const float *__restrict__ w2, float *__restrict__ part) {
    using G = GeoWB<FOV, OD>;
    constexpr int F2 = FOV * FOV, S1 = G::S1, P1 = G::P1, S2 = G::S2, P2 = G::P2, RB = G::RB;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *s_w2 = lds;                            // [c2][c1][9]
    float *s_w1 = s_w2 + OD * OD * 9;             // [c1][27], then [od] biases
    float *s_x = s_w1 + OD * 28;                  // [RB][NPIX]
    float *s_dz = s_x + RB * G::NPIX;             // [RB][od][P2]: upstream gradient through the last ReLU
    float *s_a1 = s_dz + RB * G::NDZ;             // [RB][od][P1]: a1, then dz1
    const int tid = threadIdx.x;
    crnn_front::stage_bwd_weights<kBlockB, OD, true>(s_w2, s_w1, w2, w1, b1, tid);

    float acc2[G::NPAIR][9], acc1[G::NITEM], accb2 = 0.0f, accb1 = 0.0f;
#pragma unroll
    for (int i = 0; i < G::NPAIR; ++i)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc2[i][k] = 0.0f;
#pragma unroll
    for (int i = 0; i < G::NITEM; ++i) acc1[i] = 0.0f;
    const int bias_c = tid - (kBlockB - OD);      // the last OD threads sum the bias gradients

    const long n_blocks = (rows + RB - 1) / RB;
    const long per = (n_blocks + gridDim.x - 1) / gridDim.x;
    const long blk0 = (long)blockIdx.x * per, blk1 = min(n_blocks, blk0 + per);
    for (long blk = blk0; blk < blk1; ++blk) {
        const long row0 = blk * RB;
        const int rv = (int)min((long)RB, rows - row0);
        __syncthreads();
        crnn_front::stage_bwd_rows<kBlockB, RB, G::NPIX, G::NDZ>(s_x, s_dz, obs, obs_stride, y, y_stride, g, g_stride, row0, rv, tid);
        __syncthreads();
        // A: conv1 + ReLU, taps in the order of the forward's K (c0, kx, ky); rows past the end are zeros
        for (int i = tid; i < RB * G::NA1; i += kBlockB) {
            const int r = i / G::NA1, rem = i - r * G::NA1, c1 = rem / P1, p = rem - c1 * P1;
            float a = 0.0f;
            if (r < rv) {
                a = s_w1[OD * 27 + c1];
                const float *xin = s_x + r * G::NPIX + (p / S1) * FOV + p % S1;
                const float *w = s_w1 + c1 * 27;
#pragma unroll
                for (int k = 0; k < 27; ++k) a = fmaf(xin[(k / 9) * F2 + ((k % 9) / 3) * FOV + k % 3], w[k], a);
            }
            s_a1[i] = fmaxf(a, 0.0f);
        }
        __syncthreads();
        // B: dW2, one output line of dz2 against the three lines of a1 under it
#pragma unroll
        for (int i = 0; i < G::NPAIR; ++i) {
            const int u = tid + i * kBlockB;
            if (u < OD * OD) {
                const int c2 = u / OD, c1 = u - c2 * OD;
#pragma unroll 1
                for (int r = 0; r < rv; ++r) {
                    const float *dzp = s_dz + r * G::NDZ + c2 * P2, *ap = s_a1 + r * G::NA1 + c1 * P1;
#pragma unroll 1
                    for (int h = 0; h < S2; ++h) {
                        float dz[S2], a[3][S1];
#pragma unroll
                        for (int k = 0; k < S2; ++k) dz[k] = dzp[h * S2 + k];
#pragma unroll
                        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                            for (int k = 0; k < S1; ++k) a[kh][k] = ap[(h + kh) * S1 + k];
#pragma unroll
                        for (int t = 0; t < 9; ++t)
#pragma unroll
                            for (int k = 0; k < S2; ++k) acc2[i][t] = fmaf(dz[k], a[t / 3][k + t % 3], acc2[i][t]);
                    }
                }
            }
        }
        if (bias_c >= 0)
            for (int r = 0; r < rv; ++r)
                for (int p = 0; p < P2; ++p) accb2 += s_dz[r * G::NDZ + bias_c * P2 + p];
        // da1 of the lines (r, c1, y): a transposed convolution in gather form
        float da[G::NLINE][S1];
#pragma unroll
        for (int i = 0; i < G::NLINE; ++i) {
#pragma unroll
            for (int k = 0; k < S1; ++k) da[i][k] = 0.0f;
            const int v = tid + i * kBlockB;
            const int r = v / (OD * S1), rem = v - r * (OD * S1), c1 = rem / S1, yy = rem - c1 * S1;
            if (v < RB * OD * S1 && r < rv) {
#pragma unroll 1
                for (int c2 = 0; c2 < OD; ++c2) {
                    float w[9];
#pragma unroll
                    for (int k = 0; k < 9; ++k) w[k] = s_w2[(c2 * OD + c1) * 9 + k];
#pragma unroll
                    for (int kh = 0; kh < 3; ++kh) {
                        const int h = yy - kh;
                        if (h >= 0 && h < S2) {
                            float dz[S2];
#pragma unroll
                            for (int k = 0; k < S2; ++k) dz[k] = s_dz[r * G::NDZ + c2 * P2 + h * S2 + k];
#pragma unroll
                            for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                                for (int k = 0; k < S2; ++k) da[i][k + kw] = fmaf(dz[k], w[kh * 3 + kw], da[i][k + kw]);
                        }
                    }
                }
            }
        }
        __syncthreads();   // every reader of a1 (dW2) is done
        // C: dz1 = da1 * (a1 > 0) in place (a1 of the rows past the end is zero: they stay zero)
#pragma unroll
        for (int i = 0; i < G::NLINE; ++i) {
            const int v = tid + i * kBlockB;
            if (v < RB * OD * S1) {
                float *a1 = s_a1 + v * S1;   // (r, c1, y) lines are laid out in the order of s_a1
#pragma unroll
                for (int k = 0; k < S1; ++k) a1[k] = a1[k] > 0.0f ? da[i][k] : 0.0f;
            }
        }
        __syncthreads();
        // D: dW1, db1 from dz1
#pragma unroll
        for (int i = 0; i < G::NITEM; ++i) {
            const int v = tid + i * kBlockB;
            if (v < OD * 27) {
                const int c1 = v / 27, k = v - c1 * 27, c0 = k / 9, kx = (k - c0 * 9) / 3, ky = k % 3;
#pragma unroll 1
                for (int r = 0; r < rv; ++r) {
                    const float *d = s_a1 + r * G::NA1 + c1 * P1;
                    const float *xin = s_x + r * G::NPIX + c0 * F2 + kx * FOV + ky;
#pragma unroll 1
                    for (int h = 0; h < S1; ++h)
#pragma unroll
                        for (int q = 0; q < S1; ++q) acc1[i] = fmaf(d[h * S1 + q], xin[h * FOV + q], acc1[i]);
                }
            }
        }
        if (bias_c >= 0)
            for (int r = 0; r < rv; ++r)
                for (int p = 0; p < P1; ++p) accb1 += s_a1[r * G::NA1 + bias_c * P1 + p];
    }
    float *pp = part + (size_t)blockIdx.x * G::GRADS;
#pragma unroll
    for (int i = 0; i < G::NPAIR; ++i) {
        const int u = tid + i * kBlockB;
        if (u < OD * OD)
#pragma unroll
            for (int t = 0; t < 9; ++t) pp[u * 9 + t] = acc2[i][t];
    }
    if (bias_c >= 0) pp[OD * OD * 9 + bias_c] = accb2;
#pragma unroll
    for (int i = 0; i < G::NITEM; ++i) {
        const int v = tid + i * kBlockB;
        if (v < OD * 27) pp[G::N2 + v] = acc1[i];
    }
    if (bias_c >= 0) pp[G::N2 + OD * 27 + bias_c] = accb1;
}

bool supported(int fov, int od) { return (fov == 11 || fov == 13) && (od == 24 || od == 32); }

// one of the four instantiations' constants
#define WIDE_PICK(T, FIELD) (fov == 11 ? (od == 24 ? T<11, 24>::FIELD : T<11, 32>::FIELD) : (od == 24 ? T<13, 24>::FIELD : T<13, 32>::FIELD))

}  // namespace

extern "C" {

int crnn_wide_padded_cols(int fov, int od) {
    if (!supported(fov, od)) return CRNN_WIDE_ERR_UNSUPPORTED;
    return WIDE_PICK(GeoW, PAD_COLS);
}

int crnn_wide_forward_block_rows(int fov, int od) {
    if (!supported(fov, od)) return CRNN_WIDE_ERR_UNSUPPORTED;
    return WIDE_PICK(GeoW, RB);
}

int crnn_wide_backward_block_rows(int fov, int od) {
    if (!supported(fov, od)) return CRNN_WIDE_ERR_UNSUPPORTED;
    return WIDE_PICK(GeoWB, RB);
}

int crnn_wide_front_forward(int fov, const int8_t *d_obs, int64_t obs_stride, const int8_t *d_onehot, int n_actions, int64_t rows,
                            const float *d_w1, const float *d_b1, const float *d_w2, const float *d_b2, const float *d_mlp_w,
                            const float *d_mlp_b, int od, float *d_out, int64_t out_stride, int out_cols, void *stream) {
    if (!supported(fov, od)) return CRNN_WIDE_ERR_UNSUPPORTED;
    if (!crnn_front::forward_args_ok(3 * fov * fov, WIDE_PICK(GeoW, NFEAT), WIDE_PICK(GeoW, PAD_COLS), true, d_obs, obs_stride, n_actions, rows,
                                     d_w1, d_b1, d_w2, d_b2, d_mlp_w, d_mlp_b, d_out, out_stride, out_cols))
        return CRNN_WIDE_ERR_BAD_ARG;
    if (rows == 0) return CRNN_WIDE_OK;
    hipStream_t s = (hipStream_t)stream;
    // persistent: one workgroup per CU (LDS), the weights stay in registers
#define FWD(F, O)                                                                                                                \
    crnn_front::launch_forward<k_front_wide<F, O>, GeoW<F, O>, kBlockF>(                                                         \
        crnn_front::grid_per_cu((rows + GeoW<F, O>::RB - 1) / GeoW<F, O>::RB), d_obs, obs_stride, rows, d_w1, d_b1, d_w2, d_b2, d_out, \
        out_stride, out_cols, d_onehot, n_actions, d_mlp_w, d_mlp_b, s)
    if (fov == 11) return od == 24 ? FWD(11, 24) : FWD(11, 32);
    return od == 24 ? FWD(13, 24) : FWD(13, 32);
#undef FWD
}

int crnn_wide_backward_parts(int fov, int od) {
    if (!supported(fov, od)) return CRNN_WIDE_ERR_UNSUPPORTED;
    return WIDE_PICK(GeoWB, GRADS);
}

int crnn_wide_backward(int fov, const int8_t *d_obs, int64_t obs_stride, int64_t rows, const float *d_out, int64_t out_stride,
                       const float *d_grad_out, int64_t grad_stride, const float *d_w1, const float *d_b1, const float *d_w2,
                       int od, float *d_part, int n_part, float *d_grads, void *stream) {
    if (!supported(fov, od)) return CRNN_WIDE_ERR_UNSUPPORTED;
    if (!crnn_front::backward_args_ok(3 * fov * fov, WIDE_PICK(GeoW, NFEAT), true, d_obs, obs_stride, rows, d_out, out_stride, d_grad_out,
                                      grad_stride, d_w1, d_b1, d_w2, d_part, n_part, d_grads))
        return CRNN_WIDE_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
#define BWD(F, O)                                                                                                                  \
    crnn_front::launch_backward<k_front_wide_bwd<F, O>, GeoWB<F, O>, kBlockB>(d_obs, obs_stride, rows, d_out, out_stride, d_grad_out, \
                                                                              grad_stride, d_w1, d_b1, d_w2, d_part, n_part, d_grads, s)
    if (fov == 11) return od == 24 ? BWD(11, 24) : BWD(11, 32);
    return od == 24 ? BWD(13, 24) : BWD(13, 32);
#undef BWD
}

int crnn_wide_last_hip_error(void) { return g_last_hip; }

}  // extern "C"
