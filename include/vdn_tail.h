/*
 * vdn_tail.h -- C ABI of the small-launch savers of the packed VDN learn (built into libvdn_ops.so beside vdn_ops.h, whose
 * conventions and error codes apply): the two scalar sums of the loss formed inside the TD forward launch, the TD backward that
 * writes its own zero padding rows, and the learn's input gathers as one launch.
 */
#ifndef VDN_TAIL_H
#define VDN_TAIL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* vdn_td_forward (vdn_ops.h) that also leaves the two scalars of the loss in d_sums float32[2] when it is not NULL:
 * d_sums[0] = num = sum(d_mtd ** 2), d_sums[1] = sum(d_mask), in the same launch.  Every workgroup adds its slots in a fixed
 * order and the workgroup that finishes last adds the per-workgroup pairs (d_part: float32[vdn_td_sum_parts(B * T)] of scratch) in
 * a fixed order: deterministic, no float atomics, no second launch.  The hand-off goes through one device word per device, so
 * launches of the *_sums entry points on one device must be ordered on ONE stream; the word resets itself with the last
 * arrival (repeated launches and graph replay are fine).  d_sums == NULL: exactly vdn_td_forward. */
int vdn_td_sum_parts(int64_t n_slots);
int vdn_td_forward_sums(const float *d_q_eval, const float *d_q_target, const int8_t *d_u, const float *d_r,
                        const int8_t *d_avail_next, const uint8_t *d_terminated, const uint8_t *d_padded, int32_t B, int32_t T,
                        int32_t t_limit, int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd, float *d_mask,
                        int32_t *d_bad_actions, float *d_part, float *d_sums, void *stream);
/* vdn_td_forward_packed with the same sums (d_part: float32[vdn_td_sum_parts(n_units)]). */
int vdn_td_forward_packed_sums(const float *d_q_eval, const float *d_q_target, const int32_t *d_units, int32_t n_units,
                               const int8_t *d_u, const float *d_r, const int8_t *d_avail_next, const uint8_t *d_terminated,
                               const uint8_t *d_padded, int32_t n_agents, int32_t n_actions, float gamma, float *d_mtd, float *d_mask,
                               int32_t *d_bad_actions, float *d_part, float *d_sums, void *stream);

/* vdn_td_backward_packed with the zero rows behind the last unit: d_grad_q float32[rows_pad][A], rows n_units*n .. rows_pad-1
 * are written as zeros by the same launch (the packed learn pads its row count for the GEMMs that follow). */
int vdn_td_backward_packed_pad(const float *d_mtd, const float *d_mask, const int32_t *d_units, int32_t n_units, const int8_t *d_u,
                               const float *d_grad_num, int32_t n_agents, int32_t n_actions, int64_t rows_pad, float *d_grad_q,
                               void *stream);

/* Up to VDN_GATHER_MAX copies of vdn_gather_units over ONE unit list in one launch: HOST arrays of n_gathers sources, unit
 * sizes, shifts, zero_below counts and destinations.  Destination i is dst_bytes[i] >= n_units * unit_bytes[i] bytes long; the
 * bytes behind its last unit are zero-filled (the padding rows of the packed learn).  The units' bytes are exactly those
 * vdn_gather_units writes.  A thread moves four destination words (bytes, where a unit size, a destination size or a start
 * address is no multiple of 4), its source loads in flight together, as one 16-byte (4-byte) store where the destination starts
 * on such a boundary -- a fresh allocation always does; any other start is served with single stores. */
#define VDN_GATHER_MAX 4
int vdn_gather_units_batch(int32_t n_gathers, const void *const *d_src, const int32_t *unit_bytes, const int32_t *unit_shift,
                           const int32_t *zero_below, void *const *d_dst, const int64_t *dst_bytes, const int32_t *d_units,
                           int32_t n_units, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VDN_TAIL_H */
