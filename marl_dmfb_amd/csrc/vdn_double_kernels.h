// vdn_double_kernels.h -- the kernels of include/vdn_double.h: the one-step TD block and the lambda walk of the VDN learn with
// double-Q targets.  Included by vdn_ops.hip behind vdn_lambda_kernels.h.  Nothing here but four kernel shells: the selector operand
// is QSel of td_rules.h, the pick lives in td_row (its Sel::on variant), the row-parallel body in td_forward_rows and the walk in
// td_lambda_episode / td_lambda_packed, each instantiated with QSel where the kernels of vdn_ops.h and vdn_lambda.h pass NoSel.  No
// LDS beyond what those bodies hold: a lane reads its selector rows from global memory, at most 127 actions per agent, and writes
// its picks itself.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vdn_double.h"

namespace {

template <class Index>
__global__ __launch_bounds__(256) void k_td_double_forward(const Index ix, const TdIn in, const TdOut out, const QSel sel) {
    td_forward_rows(ix, in, out, sel, blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void k_td_double_lambda_forward(const PaddedIndex ix, const TdIn in, float lam, const TdOut out, const QSel sel) {
    const int ep = blockIdx.x * kLamEp + (threadIdx.x >> 6);
    td_lambda_episode(ix, ep, ep < ix.B ? ix.T : 0, in, lam, out, sel);
}

__global__ __launch_bounds__(256) void k_td_double_lambda_forward_packed(PackedIndex ix, int E, int n_steps, const TdIn in, float lam,
                                                                         const TdOut out, const LambdaOff lo, const QSel sel) {
    td_lambda_packed(ix, E, n_steps, in, lam, out, lo, sel);
}

}  // namespace
