/*
 * crnn_wide.h -- C ABI of the HIP front end of the reference's per-agent Q-network `CRNN` (network/base_net.py:23-71)
 * for the two wide fields of view of the reference's conv_str besides fov 19:
 *   fov 11: Conv2d(3->od,k3,s1)+ReLU 11x11->9x9,   Conv2d(od->od,k3,s1)+ReLU 9x9->7x7,   flatten (c,h,w): od*49 features
 *   fov 13: Conv2d(3->od,k3,s1)+ReLU 13x13->11x11, Conv2d(od->od,k3,s1)+ReLU 11x11->9x9, flatten (c,h,w): od*81 features
 * The fov is an explicit argument; only fov 11 and 13 with od 24 or 32 are accepted (fov 5 / 7: crnn_fov.h, fov 9 / 19:
 * crnn_ops.h): anything else returns CRNN_WIDE_ERR_UNSUPPORTED before any argument is looked at and without launching.
 * fp32 arithmetic throughout (v_mfma_f32_16x16x4_f32 in the forward, plain fmaf in the backward): the same products as
 * torch.nn.functional.conv2d, another summation order.  The conventions are those of crnn_fov.h with od*9 replaced by
 * n_conv = od*P2, P2 = 49 (fov 11) or 81 (fov 13).
 */
#ifndef CRNN_WIDE_H
#define CRNN_WIDE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRNN_WIDE_OK 0
#define CRNN_WIDE_ERR_BAD_ARG (-1)
#define CRNN_WIDE_ERR_UNSUPPORTED (-6) /* fov other than 11 / 13, od other than 24 / 32 */
#define CRNN_WIDE_ERR_HIP (-100)

/* The non-recurrent front end of CRNN.forward (network/base_net.py:59-68) for fov 11 / 13 in one launch:
 *   d_obs:   int8 [rows][obs_stride], the first 3*fov*fov bytes of a row = pixel block (3,fov,fov) in (c,x,y) order, then
 *            dir_x, dir_y at offset 3*fov*fov
 *   d_w1:    float32 [od][3][3][3]  d_b1: [od];   d_w2: float32 [od][od][3][3]  d_b2: [od]
 *   d_out[r][0 .. n_conv)            conv features, index c*P2 + h*S2 + w, S2 = 7 / 9
 *   d_out[r][n_conv .. n_conv+10)    relu(mlp1(vec)), vec = [dir_x, dir_y, onehot[r][0..n_actions)]
 * d_onehot: int8 [rows][n_actions] (may be NULL = all zeros); d_mlp_w: float32 [10][2+n_actions], d_mlp_b: [10]; n_actions <= 16.
 * d_mlp_w == NULL: pixel features only (obs_stride >= 3*fov*fov, out_stride >= n_conv).
 * out_cols: 0, or n_feat <= out_cols <= crnn_wide_padded_cols(fov, od) (and <= out_stride), n_feat = n_conv (+10 with the vector
 * branch): columns n_feat .. out_cols-1 of every row are written as zeros (the GRU input GEMM runs on K = padded_cols).
 * Rows are written with 16-byte stores when d_out and out_stride are 16-byte multiples and the columns written a multiple of 4,
 * with 4-byte stores otherwise. */
int crnn_wide_front_forward(int fov, const int8_t *d_obs, int64_t obs_stride, const int8_t *d_onehot, int n_actions, int64_t rows,
                            const float *d_w1, const float *d_b1, const float *d_w2, const float *d_b2, const float *d_mlp_w,
                            const float *d_mlp_b, int od, float *d_out, int64_t out_stride, int out_cols, void *stream);
/* n_conv+10 rounded up to a multiple of 64 (fov 11: 1216 / 1600 for od 24 / 32; fov 13: 1984 / 2624), or
 * CRNN_WIDE_ERR_UNSUPPORTED. */
int crnn_wide_padded_cols(int fov, int od);
/* Rows per workgroup pass of the forward / backward kernel as built for (fov, od), or CRNN_WIDE_ERR_UNSUPPORTED: the row counts
 * at which a launch changes shape (a ragged last block, a second pass of the persistent loop). */
int crnn_wide_forward_block_rows(int fov, int od);
int crnn_wide_backward_block_rows(int fov, int od);
/* Gradients of the conv tensors for the eval network of VDN.learn (policy/vdn.py:123-128 backward through
 * network/base_net.py:63-65); the observation needs none.  Nothing is saved by the forward: the conv1 activations are recomputed
 * inside the kernel.  d_out is the forward's output (its sign is the last ReLU's mask), d_grad_out the gradient w.r.t. it (the
 * first n_conv columns of a row are read).  One persistent workgroup per partial vector (n_part <= 256) accumulates over a
 * contiguous range of rows into d_part float32[n_part][crnn_wide_backward_parts(fov, od)] (scratch); a second small kernel adds
 * the partial vectors in a fixed order (deterministic, no atomics) into d_grads:
 *   float32[od*od*9 + od + od*27 + od] = dW2[od][od][3][3] | db2[od] | dW1[od][3][3][3] | db1[od]
 * The vector branch's gradients come from crnn_mlp_backward (crnn_ops.h) with dir_offset = 3*fov*fov and col0 = n_conv. */
int crnn_wide_backward_parts(int fov, int od);
int crnn_wide_backward(int fov, const int8_t *d_obs, int64_t obs_stride, int64_t rows, const float *d_out, int64_t out_stride,
                       const float *d_grad_out, int64_t grad_stride, const float *d_w1, const float *d_b1, const float *d_w2,
                       int od, float *d_part, int n_part, float *d_grads, void *stream);
int crnn_wide_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif
