// crnn_front.h -- what the four CRNN front-end kernel families (crnn_mfma.h: fov 9, crnn_mfma19.h: fov 19, crnn_fov.hip: fov 5 / 7,
// crnn_wide.hip: fov 11 / 13) do around their convolution tilings: the parameters of the vector branch relu(mlp1([dir, last action]))
// (network/base_net.py:66), the zero tail of the staged rows and their stream-out, one float32 row per observation; for
// crnn_fov.hip / crnn_wide.hip also the staging of the inputs, the B operands, the LDS staging of the VALU backward and its reduce kernel;
// and the host side: the persistent-grid policies, the launchers and the argument contracts.
// The tilings, LDS layouts, block sizes and launch shapes stay with each kernel.  No helper knows which kernel calls it: what
// differs between callers (block size, geometry) is a template or function argument.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace crnn_front {

constexpr int kVec = 18;               // inputs of the vector branch per row: dir_x, dir_y, one-hot (<= 16)
constexpr int kMlp = 10 * kVec + 10;   // mlp1 in LDS: [10][nin] weights (nin <= kVec), then the [10] biases at 10 * kVec
// A row may be written out zero-padded to a multiple of 64 floats (the GRU input GEMM runs 15-25 % faster on K = 640 than on 610)
constexpr int padded_cols(int n_conv) { return (n_conv + 10 + 63) / 64 * 64; }

// The vector branch's parameters live in LDS: read from global memory at the head of every row block, the wait for them
// was also a wait for the previous block's output stores (one in-order memory counter on gfx9).
template <int BLOCK>
__device__ __forceinline__ void stage_mlp_params(float *s_mlp, const float *mlp_w, const float *mlp_b, int nin, int tid) {
    if (mlp_w) {
        for (int i = tid; i < 10 * nin; i += BLOCK) s_mlp[i] = mlp_w[i];
        if (tid < 10) s_mlp[10 * kVec + tid] = mlp_b[tid];
    }
}

// Zeros in columns col0 .. col1-1 of the ROWS staged rows (STRIDE floats each).  ROWS and STRIDE are template arguments so that
// two kernels of one library never share an instantiation: sharing one changed the register count of k_conv19_mfma
// (profiles/crnn_front/NOTES.md).
template <int BLOCK, int ROWS, int STRIDE>
__device__ __forceinline__ void zero_tail(float *s_out, int col0, int col1, int tid) {
    for (int i = tid; i < ROWS * (col1 - col0); i += BLOCK) {
        const int rr = i / (col1 - col0), k = i - rr * (col1 - col0);
        s_out[rr * STRIDE + col0 + k] = 0.0f;
    }
}

// Streams rv staged rows out: a wave per row, consecutive lanes on consecutive 16-byte chunks (quad_out: the padded rows of the
// rollouts and of VDN.learn), 8-byte chunks (wide_out) or floats.  The caller has checked once that the pointer, the row stride
// and n_out are multiples of the chunk; the staged rows in LDS always are.
template <int BLOCK>
__device__ __forceinline__ void stream_rows_out(const float *s_out, int lds_stride, float *out, long out_stride, long row0, int rv, int n_out,
                                                bool quad_out, bool wide_out, int wave, int lane) {
    if (quad_out) {
        for (int rr = wave; rr < rv; rr += BLOCK / 64) {
            float4 *dst = (float4 *)(out + (row0 + rr) * out_stride);
            const float4 *src = (const float4 *)(s_out + rr * lds_stride);
            for (int k = lane; k < n_out / 4; k += 64) dst[k] = src[k];
        }
    } else if (wide_out) {
        for (int rr = wave; rr < rv; rr += BLOCK / 64) {
            float2 *dst = (float2 *)(out + (row0 + rr) * out_stride);
            const float2 *src = (const float2 *)(s_out + rr * lds_stride);
            for (int k = lane; k < n_out / 2; k += 64) dst[k] = src[k];
        }
    } else {
        for (int rr = wave; rr < rv; rr += BLOCK / 64) {
            float *dst = out + (row0 + rr) * out_stride;
            const float *src = s_out + rr * lds_stride;
            for (int k = lane; k < n_out; k += 64) dst[k] = src[k];
        }
    }
}

// ---- crnn_fov.hip / crnn_wide.hip: the parts of k_front_* and k_front_*_bwd that do not depend on the tiling.  k_front_fov keeps its
// own forward lines (with the three forward helpers below it measured slower at fov 7 / od 32: profiles/crnn_front/NOTES.md).

// The float image of the pixel bytes of RB rows into s_in [RB][NPIX] and, with the vector branch (`vec`: the two direction bytes
// are read only then), its inputs into s_vec [RB][kVec]
template <int BLOCK, int RB, int NPIX>
__device__ __forceinline__ void stage_obs_rows(float *s_in, float *s_vec, const int8_t *obs, long obs_stride, const int8_t *onehot, int n_actions,
                                               bool vec, long row0, int rv, int tid) {
    const int rowb = NPIX + (vec ? 2 : 0);
    for (int i = tid; i < RB * rowb; i += BLOCK) {
        const int r = i / rowb, b = i - r * rowb;
        const float v = r < rv ? (float)obs[(row0 + r) * obs_stride + b] : 0.0f;   // rows past the end: finite zeros
        if (b < NPIX) s_in[r * NPIX + b] = v;
        else s_vec[r * kVec + b - NPIX] = v;
    }
    if (vec) {
        for (int i = tid; i < RB * 16; i += BLOCK) {
            const int r = i >> 4, a = i & 15;
            s_vec[r * kVec + 2 + a] = (r < rv && onehot && a < n_actions) ? (float)onehot[(row0 + r) * n_actions + a] : 0.0f;
        }
    }
}

// B operands of conv1 for the lane's output channel ch: K = 27 (+1 zero) in 7 steps, lane k = 4 s + kq, and the offsets of its
// taps in a FOV x FOV image
template <int FOV>
__device__ __forceinline__ void load_conv1_b(float (&bw1)[7], int (&off1)[7], const float *w1, int ch, bool chv, int kq) {
#pragma unroll
    for (int s = 0; s < 7; ++s) {
        const int k = 4 * s + kq;
        const bool kv = k < 27;
        bw1[s] = (chv && kv) ? w1[ch * 27 + k] : 0.0f;
        const int c0 = k / 9, tap = k - c0 * 9;
        off1[s] = kv ? c0 * FOV * FOV + (tap / 3) * FOV + tap % 3 : 0;  // k = 27: zero weight, any valid address
    }
}

// B operands of conv2: K = (channel quad, tap), lane channel 4 cq + kq
template <int OD>
__device__ __forceinline__ void load_conv2_b(float (&bw2)[OD / 4 * 9], const float *w2, int ch, bool chv, int kq) {
#pragma unroll
    for (int cq = 0; cq < OD / 4; ++cq)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) bw2[cq * 9 + tap] = chv ? w2[(ch * OD + 4 * cq + kq) * 9 + tap] : 0.0f;
}

// backward, once: w2 [c2][c1][9] (with a conv2), w1 [c1][27] and the [od] conv1 biases behind it into LDS
template <int BLOCK, int OD, bool TWO>
__device__ __forceinline__ void stage_bwd_weights(float *s_w2, float *s_w1, const float *w2, const float *w1, const float *b1, int tid) {
    if constexpr (TWO)
        for (int i = tid; i < OD * OD * 9; i += BLOCK) s_w2[i] = w2[i];
    for (int i = tid; i < OD * 27; i += BLOCK) s_w1[i] = w1[i];
    if (tid < OD) s_w1[OD * 27 + tid] = b1[tid];
}

// backward, per row block: s_x [RB][NPIX] pixels, s_dz [RB][NDZ] the upstream gradient through the last ReLU
template <int BLOCK, int RB, int NPIX, int NDZ>
__device__ __forceinline__ void stage_bwd_rows(float *s_x, float *s_dz, const int8_t *obs, long obs_stride, const float *y, long y_stride,
                                               const float *g, long g_stride, long row0, int rv, int tid) {
    for (int i = tid; i < RB * NPIX; i += BLOCK) {
        const int r = i / NPIX, b = i - r * NPIX;
        s_x[i] = r < rv ? (float)obs[(row0 + r) * obs_stride + b] : 0.0f;
    }
    for (int i = tid; i < RB * NDZ; i += BLOCK) {
        const int r = i / NDZ, c = i - r * NDZ;
        s_dz[i] = (r < rv && y[(row0 + r) * y_stride + c] > 0.0f) ? g[(row0 + r) * g_stride + c] : 0.0f;
    }
}

namespace {

// grads[i] = sum over the partial vectors b = 0, 1, ... of part[b][i]: one thread per output, fixed order (deterministic).
// A template, so that a library that does not launch it (crnn_ops) does not carry it.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_front_bwd_reduce(const float *__restrict__ part, int n_part, int n, float *__restrict__ grads) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    float a0 = 0.0f, a1 = 0.0f;
    int b = 0;
    for (; b + 1 < n_part; b += 2) { a0 += part[(size_t)b * n + i]; a1 += part[(size_t)(b + 1) * n + i]; }
    if (b < n_part) a0 += part[(size_t)b * n + i];
    grads[i] = a0 + a1;
}

}  // namespace

}  // namespace crnn_front

// ---- host side, for the libraries (they define HIP_ABI_TAG / HIP_ABI_ERR; a stand-alone probe of one kernel does not)
#if defined(HIP_ABI_TAG) && defined(HIP_ABI_ERR)
#include "hip_abi.h"

namespace crnn_front {

// Grids of the persistent forward kernels (the weights stay in a workgroup's registers) over n_blocks row blocks:
// as many workgroups as the 256 CUs hold at once, which the dynamic LDS of one limits
inline int grid_resident(long n_blocks, size_t lds) {
    const long resident = 256L * (long)((size_t)160 * 1024 / lds);
    return (int)(n_blocks < resident ? n_blocks : resident);
}
// one workgroup per CU
inline int grid_per_cu(long n_blocks) { return (int)(n_blocks < 256 ? n_blocks : 256); }

// k_front_fov / k_front_wide (Kernel) with G::LDS_FLOATS of dynamic LDS on `grid` workgroups of BLOCK threads
template <auto Kernel, class G, int BLOCK>
int launch_forward(int grid, const int8_t *obs, long obs_stride, long rows, const float *w1, const float *b1, const float *w2, const float *b2,
                   float *out, long out_stride, int out_cols, const int8_t *onehot, int n_actions, const float *mlp_w, const float *mlp_b,
                   hipStream_t s) {
    const size_t lds = G::LDS_FLOATS * sizeof(float);
    static LdsLimit lds_limit;
    if (const int rc = lds_limit.raise((const void *)Kernel, lds)) return rc;
    LAUNCH(Kernel, dim3(grid), dim3(BLOCK), lds, s, obs, obs_stride, rows, w1, b1, w2, b2, out, out_stride, out_cols, onehot, n_actions,
           mlp_w, mlp_b);
    return 0;
}

// k_front_fov_bwd / k_front_wide_bwd (Kernel), one persistent workgroup per partial vector, and the reduce, under one status
template <auto Kernel, class G, int BLOCK>
int launch_backward(const int8_t *obs, long obs_stride, long rows, const float *y, long y_stride, const float *g, long g_stride,
                    const float *w1, const float *b1, const float *w2, float *part, int n_part, float *grads, hipStream_t s) {
    const size_t lds = G::LDS_FLOATS * sizeof(float);
    static LdsLimit lds_limit;
    if (const int rc = lds_limit.raise((const void *)Kernel, lds)) return rc;
    const long n_blocks = (rows + G::RB - 1) / G::RB;
    const int grid = (int)(n_blocks < n_part ? n_blocks : n_part);
    HIP_TRY(launch_status([&] {
        hipLaunchKernelGGL(Kernel, dim3(grid), dim3(BLOCK), lds, s, obs, obs_stride, rows, y, y_stride, g, g_stride, w1, b1, w2, part);
        hipLaunchKernelGGL(k_front_bwd_reduce<256>, dim3((G::GRADS + 255) / 256), dim3(256), 0, s, part, grid, G::GRADS, grads);
    }));
    return 0;
}

// The argument contract of *_front_forward for a supported (fov, od): npix pixel bytes and n_conv conv features per row, rows
// padded to at most pad_cols columns, `two`: the stack has a conv2.  False: the library's *_ERR_BAD_ARG.
inline bool forward_args_ok(int npix, int n_conv, int pad_cols, bool two, const int8_t *d_obs, int64_t obs_stride, int n_actions, int64_t rows,
                            const float *d_w1, const float *d_b1, const float *d_w2, const float *d_b2, const float *d_mlp_w,
                            const float *d_mlp_b, const float *d_out, int64_t out_stride, int out_cols) {
    const bool vec = d_mlp_w != nullptr;
    const int n_feat = n_conv + (vec ? 10 : 0);
    if (!d_obs || !d_w1 || !d_b1 || (two && (!d_w2 || !d_b2)) || !d_out || rows < 0 || obs_stride < npix + (vec ? 2 : 0) ||
        out_stride < n_feat || n_actions < 0 || n_actions > 16 || (vec && !d_mlp_b))
        return false;
    return out_cols == 0 || (out_cols >= n_feat && out_cols <= pad_cols && out_cols <= out_stride);
}

// The same for *_backward: a row shorter than what the kernel reads of it (a stride of 0 is what an expanded gradient has) is
// refused, not launched
inline bool backward_args_ok(int npix, int n_conv, bool two, const int8_t *d_obs, int64_t obs_stride, int64_t rows, const float *d_out,
                             int64_t out_stride, const float *d_grad_out, int64_t grad_stride, const float *d_w1, const float *d_b1,
                             const float *d_w2, const float *d_part, int n_part, const float *d_grads) {
    return d_obs && d_out && d_grad_out && d_w1 && d_b1 && (!two || d_w2) && d_part && d_grads && rows > 0 && n_part >= 1 && n_part <= 256 &&
           obs_stride >= npix && out_stride >= n_conv && grad_stride >= n_conv;
}

}  // namespace crnn_front
#endif
