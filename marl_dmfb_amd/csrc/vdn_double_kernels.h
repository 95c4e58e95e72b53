// vdn_double_kernels.h -- the kernels of include/vdn_double.h: the one-step TD block and the lambda walk of the VDN learn with
// double-Q targets.  Included by vdn_ops.hip behind vdn_lambda_kernels.h.  Nothing here but the selector and four kernel shells:
// the pick lives in td_row (its Sel::on variant), the row-parallel body in td_forward_rows and the walk in td_lambda_episode /
// td_lambda_packed, each instantiated with TdSel where the kernels of vdn_ops.h and vdn_lambda.h pass NoSel.  No LDS beyond what
// those bodies hold: a lane reads its selector rows from global memory, at most 127 actions per agent, and writes its picks itself.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vdn_double.h"

namespace {

// the selector operand.  qs: [T][B][n][A] beside the padded Q tensors, [n_sel][n][A] in the packed form, where sel_units[row] names
// the selector unit of output row `row` (NULL: the row's own unit, which the host has checked to exist)
struct TdSel {
    static constexpr bool on = true;
    const float *qs;
    const int32_t *sel_units;
    int n_sel;
    int8_t *picks;   // [rows][n] or NULL
    // false: sel_units[row] lies outside [0, n_sel) and is not used as an index; td_row then reads no selector at all
    __device__ __forceinline__ bool place(int row, int n, int A, At &at) const {
        if (!sel_units) return true;
        const int32_t k = sel_units[row];
        if ((uint32_t)k >= (uint32_t)n_sel) return false;
        at.s0 = (size_t)k * n * A;
        return true;
    }
};

template <class Index>
__global__ __launch_bounds__(256) void k_td_double_forward(const Index ix, const TdIn in, const TdOut out, const TdSel sel) {
    td_forward_rows(ix, in, out, sel, blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void k_td_double_lambda_forward(const PaddedIndex ix, const TdIn in, float lam, const TdOut out, const TdSel sel) {
    const int ep = blockIdx.x * kLamEp + (threadIdx.x >> 6);
    td_lambda_episode(ix, ep, ep < ix.B ? ix.T : 0, in, lam, out, sel);
}

__global__ __launch_bounds__(256) void k_td_double_lambda_forward_packed(PackedIndex ix, int E, int n_steps, const TdIn in, float lam,
                                                                         const TdOut out, const LambdaOff lo, const TdSel sel) {
    td_lambda_packed(ix, E, n_steps, in, lam, out, lo, sel);
}

}  // namespace
