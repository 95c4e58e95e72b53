/*
 * crnn_fov.h -- C ABI of the HIP front end of the reference's per-agent Q-network `CRNN` (network/base_net.py:23-71)
 * for the two small fields of view the reference trains besides fov 9 (multiTrain.py: fov 5 and 7):
 *   fov 7: Conv2d(3->od,k3,s1)+ReLU 7x7->5x5, Conv2d(od->od,k3,s1)+ReLU 5x5->3x3, flatten (c,h,w)
 *   fov 5: Conv2d(3->od,k3,s1)+ReLU 5x5->3x3, flatten (c,h,w)
 * Both stacks end in od x 3 x 3 = od*9 features.  The fov is an explicit argument; only fov 5 and 7 with od 24 or 32 are
 * accepted (fov 9 and 19 have their own entry points in crnn_ops.h): anything else returns CRNN_FOV_ERR_UNSUPPORTED before
 * any argument is looked at and without launching.  fp32 arithmetic throughout (v_mfma_f32_16x16x4_f32 in the forward,
 * plain fmaf in the backward): the same products as torch.nn.functional.conv2d, another summation order.
 */
#ifndef CRNN_FOV_H
#define CRNN_FOV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRNN_FOV_OK 0
#define CRNN_FOV_ERR_BAD_ARG (-1)
#define CRNN_FOV_ERR_UNSUPPORTED (-6) /* fov other than 5 / 7, od other than 24 / 32 */
#define CRNN_FOV_ERR_HIP (-100)

/* The non-recurrent front end of CRNN.forward (network/base_net.py:59-68) for fov 5 / 7 in one launch, with the contract of
 * crnn_front9_forward (crnn_ops.h):
 *   d_obs:   int8 [rows][obs_stride], the first 3*fov*fov bytes of a row = pixel block (3,fov,fov) in (c,x,y) order, then
 *            dir_x, dir_y at offset 3*fov*fov
 *   d_w1:    float32 [od][3][3][3]  d_b1: [od];   d_w2: float32 [od][od][3][3]  d_b2: [od]  (fov 7 only; ignored for fov 5)
 *   d_out[r][0 .. od*9)            conv features, index c*9 + h*3 + w
 *   d_out[r][od*9 .. od*9+10)      relu(mlp1(vec)), vec = [dir_x, dir_y, onehot[r][0..n_actions)]
 * d_onehot: int8 [rows][n_actions] (may be NULL = all zeros); d_mlp_w: float32 [10][2+n_actions], d_mlp_b: [10]; n_actions <= 16.
 * d_mlp_w == NULL: pixel features only (obs_stride >= 3*fov*fov, out_stride >= od*9).
 * out_cols: 0, or n_feat <= out_cols <= crnn_fov_padded_cols(fov, od) (and <= out_stride), n_feat = od*9 (+10 with the vector
 * branch): columns n_feat .. out_cols-1 of every row are written as zeros (the GRU input GEMM runs on K = 256 / 320). */
int crnn_fov_front_forward(int fov, const int8_t *d_obs, int64_t obs_stride, const int8_t *d_onehot, int n_actions, int64_t rows,
                           const float *d_w1, const float *d_b1, const float *d_w2, const float *d_b2, const float *d_mlp_w,
                           const float *d_mlp_b, int od, float *d_out, int64_t out_stride, int out_cols, void *stream);
/* od*9+10 rounded up to a multiple of 64 (256 for od 24, 320 for od 32), or CRNN_FOV_ERR_UNSUPPORTED. */
int crnn_fov_padded_cols(int fov, int od);
/* Gradients of the conv tensors for the eval network of VDN.learn (policy/vdn.py:123-128 backward through
 * network/base_net.py:63-65); the observation needs none.  Nothing is saved by the forward: for fov 7 the conv1 activations are
 * recomputed inside the kernel.  d_out is the forward's output (its sign is the last ReLU's mask), d_grad_out the gradient
 * w.r.t. it (the first od*9 columns of a row are read).  One persistent workgroup per partial vector (n_part <= 256) accumulates
 * over a contiguous range of rows into d_part float32[n_part][crnn_fov_backward_parts(fov, od)] (scratch); a second small
 * kernel adds the partial vectors in a fixed order (deterministic) into d_grads:
 *   fov 7: float32[od*od*9 + od + od*27 + od] = dW2[od][od][3][3] | db2[od] | dW1[od][3][3][3] | db1[od]
 *   fov 5: float32[od*27 + od]                = dW1[od][3][3][3] | db1[od]
 * d_w2 is read for fov 7 only (may be NULL for fov 5).  The vector branch's gradients come from crnn_mlp_backward (crnn_ops.h)
 * with dir_offset = 3*fov*fov and col0 = od*9. */
int crnn_fov_backward_parts(int fov, int od);
int crnn_fov_backward(int fov, const int8_t *d_obs, int64_t obs_stride, int64_t rows, const float *d_out, int64_t out_stride,
                      const float *d_grad_out, int64_t grad_stride, const float *d_w1, const float *d_b1, const float *d_w2,
                      int od, float *d_part, int n_part, float *d_grads, void *stream);
int crnn_fov_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif
