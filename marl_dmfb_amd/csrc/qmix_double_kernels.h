// qmix_double_kernels.h -- the selector of include/qmix_double.h: the target side of k_mix_forward (qmix_ops.hip) with double-Q
// targets.  Included by qmix_ops.hip in front of k_mix_forward, which takes MixNoSel (the maximum over the target network's own
// row: the kernels of qmix_ops.h, qmix_packed.h and qmix_lambda.h) or MixSel as a compile-time parameter.  Nothing here but the two
// operand structs: the pick itself stands in k_mix_forward beside the maximum it replaces, the mixers and the TD rule behind it are
// the one row body, and the lambda walk of qmix_lambda_kernels.h runs unchanged on the totals.  No LDS: a lane reads its selector
// rows from global memory, at most 16 actions per agent.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/qmix_double.h"

namespace {

struct MixNoSel {
    static constexpr bool on = false;
};

// the selector operand.  qs: [T][B][n][A] beside the padded Q tensors, [n_sel][n][A] in the packed form, where sel_units[row] names
// the selector unit of output row `row` (NULL: the row's own block, the one of q_target, which the host has checked to exist)
struct MixSel {
    static constexpr bool on = true;
    const float *qs;
    const int32_t *sel_units;
    int n_sel;
    int8_t *picks;    // [rows][n] or NULL
    float *targets;   // one-step form: [rows] or NULL (under lambda the walk writes the targets)
    // false: sel_units[row] lies outside [0, n_sel) and is not used as an index; the row then reads no selector at all
    __device__ __forceinline__ bool place(long row, int n, int A, size_t &s0) const {
        if (!sel_units) return true;
        const int32_t k = sel_units[row];
        if ((uint32_t)k >= (uint32_t)n_sel) return false;
        s0 = (size_t)k * n * A;
        return true;
    }
};

}  // namespace
