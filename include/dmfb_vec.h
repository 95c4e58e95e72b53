/*
 * dmfb_vec.h -- C ABI of the MI355X-native vectorised DMFB droplet-routing environment.
 *
 * The reference (jesselasse/MARL-DMFB) is pure Python and has no FFI; its boundary for this
 * path is the Python object protocol of `DMFBenv` (env/DMFB/dmfb.py:474-640).  Each entry
 * point below names the reference interface it replaces.  A handle owns E independent chips
 * ("envs") resident in HBM on one GPU and advances all of them in lock-step.
 *
 * Conventions
 *   - plain C types only; every `d_*` pointer is a DEVICE pointer owned by the caller
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream)
 *   - every call is asynchronous on `stream`; no call synchronises the host, none allocates
 *     device memory after dmfb_vec_create
 *   - return value: 0 on success, negative DMFB_ERR_* otherwise (dmfb_vec_strerror)
 *   - thread-compatible, not thread-safe: one handle, one stream at a time
 *   - coordinates are (x, y) with x in [0,width) indexing the FIRST map axis, as in the
 *     reference (`m_health[x][y]`, dmfb.py:362)
 */
#ifndef DMFB_VEC_H
#define DMFB_VEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMFB_OK 0
#define DMFB_ERR_BAD_ARG (-1)
#define DMFB_ERR_FOV_TOO_LARGE (-2)     /* RuntimeError('Fov is too large')         dmfb.py:139-140 */
#define DMFB_ERR_TOO_MANY_DROPLETS (-3) /* TypeError('Too many droplets for DMFB')  dmfb.py:144-146 */
#define DMFB_ERR_CHIP_TOO_SMALL (-4)    /* assert width >= 5 and length >= 5        dmfb.py:489 */
#define DMFB_ERR_NO_AGENTS (-5)         /* assert n_agents > 0                      dmfb.py:490 */
#define DMFB_ERR_UNSUPPORTED (-6)       /* outside the build limits (see DMFB_MAX_*) */
#define DMFB_ERR_BAD_ACTION (-7)        /* TypeError('action is illegal')           dmfb.py:116 (host wrappers only) */
#define DMFB_ERR_NO_MAPS (-8)           /* map access on a handle created without maps */
#define DMFB_ERR_HIP (-100)             /* a HIP runtime call failed; see dmfb_vec_last_hip_error */

#define DMFB_MAX_AGENTS 16  /* droplets per chip the kernels are instantiated for */
#define DMFB_MAX_DIM 255    /* width/length limit (positions are packed in bytes) */
#define DMFB_MAX_BLOCKS 64  /* 2x2 obstacle blocks per chip (one wave lane holds one block during generation) */

/* dmfb_vec_step flags */
#define DMFB_STEP_RECORD 1u     /* DMFBenv.step(record=True): addUsage                dmfb.py:570-571 */
#define DMFB_STEP_AUTORESET 2u  /* envs whose episode ended this step get reset(new=False) inside the
                                   same launch; their obs row is the FIRST obs of the new episode */
#define DMFB_ACT_I32 0u         /* d_actions is int32[E][n] */
#define DMFB_ACT_I8 16u         /* d_actions is int8 [E][n] */
#define DMFB_ACT_I64 32u        /* d_actions is int64[E][n] (torch argmax output) */

/* map selector for dmfb_vec_get_map / dmfb_vec_set_map */
#define DMFB_MAP_HEALTH 0   /* RoutingTaskManager.m_health   dmfb.py:147 */
#define DMFB_MAP_USAGE 1    /* RoutingTaskManager.m_usage    dmfb.py:148 */
#define DMFB_MAP_DEGRADE 2  /* RoutingTaskManager.m_degrade  dmfb.py:151 */

typedef struct dmfb_vec dmfb_vec;

/* Constructor arguments of DMFBenv(width, length, n_agents, n_blocks, fov, stall, b_degrade,
 * per_degrade) (dmfb.py:487) plus what a batch of chips on a GPU needs. */
typedef struct {
    int32_t width, length, n_agents, n_blocks, fov;
    int32_t stall;       /* bool */
    int32_t b_degrade;   /* bool */
    int32_t with_maps;   /* bool: keep health/usage/degrade maps even when !b_degrade */
    double per_degrade;
    int32_t n_envs;      /* E: chips owned by this handle */
    uint32_t env_id0;    /* global index of env 0 (rank offset when the batch is sharded) */
    uint64_t seed;       /* Philox key (DESIGN.md "RNG contract") */
    int32_t device;      /* HIP device ordinal */
} dmfb_vec_config;

/* Outputs of one lock-step transition; any pointer may be NULL to skip that output. */
typedef struct {
    double *d_rewards;      /* [E][n] per-agent rewards, float64 as returned by step()   dmfb.py:573-574 */
    uint8_t *d_dones;       /* [E][n] per-agent dones                                    dmfb.py:577-585 */
    int32_t *d_constraints; /* [E]    info['constraints'] of THIS step                   dmfb.py:586 */
    uint8_t *d_success;     /* [E]    info['success']                                    dmfb.py:579-580 */
    int8_t *d_obs;          /* [E][n][3*fov*fov+2] observation after the step            dmfb.py:576 */
    double *d_team_reward;  /* [E]    np.sum(rewards)/n in numpy's pairwise order        common/rollout.py:33 */
    uint8_t *d_terminated;  /* [E]    all(dones)                                         common/rollout.py:34-35 */
    int8_t *d_obs_terminal; /* [E][n][3*fov*fov+2] or NULL.  With DMFB_STEP_AUTORESET the d_obs row of an env whose episode ended is
                               the FIRST observation of its next episode; the observation the reference returns for that step (the
                               terminal one, `o_next` of the episode's last transition, common/rollout.py:38,118) is written here --
                               rows of envs that did not end in this call are left untouched.  Fused launch only (n_envs below
                               dmfb_vec_launch_shape()[2]); DMFB_ERR_UNSUPPORTED otherwise. */
} dmfb_vec_step_out;

/* The guards of DMFBenv.__init__ / RoutingTaskManager.__init__ (dmfb.py:489-490, 139-146). */
int dmfb_vec_check_config(const dmfb_vec_config *cfg);

/* DMFBenv.__init__ (dmfb.py:487-511): allocates all state in HBM, draws the degradation map
 * (dmfb.py:157-166) and the first task (Generate_task, dmfb.py:155). */
int dmfb_vec_create(const dmfb_vec_config *cfg, void *stream, dmfb_vec **out);
int dmfb_vec_destroy(dmfb_vec *h);

size_t dmfb_vec_state_bytes(const dmfb_vec *h); /* HBM held by the handle */
int dmfb_vec_obs_len(const dmfb_vec *h);        /* 3*fov*fov+2, get_env_info()['obs_shape'][-1]  dmfb.py:633-640 */
int dmfb_vec_max_step(const dmfb_vec *h);       /* 2*(width+length), 'episode_limit'            dmfb.py:508 */
int dmfb_vec_n_envs(const dmfb_vec *h);
int dmfb_vec_n_agents(const dmfb_vec *h);

/* DMFBenv.reset(new) (dmfb.py:589-597) for the envs whose mask byte is non-zero (d_mask NULL =
 * all): new task, counters zeroed, then maps re-initialised (new) or updateHealth (dmfb.py:465-471).
 * If d_obs is non-NULL the rows of the reset envs are overwritten with their first observation. */
int dmfb_vec_reset(dmfb_vec *h, const uint8_t *d_mask, int new_flag, int8_t *d_obs, void *stream);

/* DMFBenv.restart() (dmfb.py:599-605): droplets back to the stored starts, same task. */
int dmfb_vec_restart(dmfb_vec *h, const uint8_t *d_mask, int8_t *d_obs, void *stream);

/* Task injection = assigning routing_manager.starts/ends then restart() (dmfb.py:185-190):
 * d_starts, d_ends int32[E][n][2] (x, y). */
int dmfb_vec_set_task(dmfb_vec *h, const int32_t *d_starts, const int32_t *d_ends, void *stream);
int dmfb_vec_get_task(const dmfb_vec *h, int32_t *d_starts, int32_t *d_ends, void *stream);

/* Obstacle injection = assigning routing_manager.blocks (dmfb.py:34-41,138): d_blocks int32[E][nb][4] =
 * (x_min, x_max, y_min, y_max), nb <= the n_blocks the handle was created with; every chip gets nb blocks.
 * get returns the current per-chip count through *nb_out (host int) and fills int32[E][n_blocks][4]. */
int dmfb_vec_set_blocks(dmfb_vec *h, const int32_t *d_blocks, int nb, void *stream);
int dmfb_vec_get_blocks(const dmfb_vec *h, int32_t *d_blocks, int *nb_out, void *stream);

/* DMFBenv.step(actions, record) (dmfb.py:560-587) for all E envs.
 * d_uniforms: float64[E][n], entry [e][i] is the random.random() draw droplet i of env e
 * takes if it draws (dmfb.py:335), or NULL to use the handle's Philox stream.
 * d_active: uint8[E] or NULL (= all).  Envs whose byte is 0 are NOT stepped (their episode is
 * over and the caller has not reset them yet, common/rollout.py:46): state untouched, outputs
 * rewards 0 / dones 1 / constraints 0 / success 0 / team_reward 0 / terminated 1, obs row rewritten
 * with the unchanged observation. */
int dmfb_vec_step(dmfb_vec *h, const void *d_actions, const double *d_uniforms, const uint8_t *d_active,
                  uint32_t flags, const dmfb_vec_step_out *out, void *stream);

/* DMFBenv.getObs() (dmfb.py:622-626): int8[E][n][3*fov*fov+2]; d_mask as in reset. */
int dmfb_vec_observe(const dmfb_vec *h, const uint8_t *d_mask, int8_t *d_obs, void *stream);

/* Introspection used by the parity tests and the single-env facade: positions int32[E][n][2],
 * distances int32[E][n] (RoutingTaskManager.distances), step_count int32[E],
 * cumulative constraints int64[E] (DMFBenv.constraints). Any pointer may be NULL. */
int dmfb_vec_get_state(const dmfb_vec *h, int32_t *d_pos, int32_t *d_dist, int32_t *d_step_count,
                       int64_t *d_constraints, void *stream);

/* RoutingTaskManager.getglobalobs() (dmfb.py:368-391), the global state QMIX mixes on: int8[3][width][length] per chip,
 * indexed [layer][x][y] and zero everywhere else.  Layer 2 = 1 on every cell of every obstacle block (x_min..x_max x
 * y_min..y_max, inclusive), written first; then for droplet i = 0, 1, ... in ascending order: layer 0 = i + 1 at its
 * position, layer 1 = i + 1 at its goal (the last writer wins on a shared cell).  state_len = 3 * width * length; a chip
 * whose state row exceeds 64 KiB returns DMFB_ERR_UNSUPPORTED. */
int dmfb_vec_state_len(const dmfb_vec *h);
/* Dense form: d_out int8[E][3][width][length]; rows of envs whose mask byte is 0 are left untouched (d_mask NULL = all). */
int dmfb_vec_global_obs(const dmfb_vec *h, const uint8_t *d_mask, int8_t *d_out, void *stream);
/* Episode append of lock-step t of a T-step rollout (one launch, the padding rule of rollout_post_step in rollout_ops.h), with
 * d_alive uint8[E] the alive flags BEFORE the step and d_term uint8[E] the step's terminated flags; d_s / d_s_next are
 * int8[E][T][state_len] episode tensors, zero-initialised by the caller:
 *   s_next[e][t] = state  if alive[e];    s[e][t+1] = state  if alive[e] && !term[e] && t + 1 < T
 * Frozen chips (alive 0) are not touched. */
int dmfb_vec_global_obs_append(const dmfb_vec *h, const uint8_t *d_alive, const uint8_t *d_term, int32_t t, int32_t T, int8_t *d_s,
                               int8_t *d_s_next, void *stream);
/* Global state of the continuous rollout (rollout_stream_step in rollout_ops.h).  d_stage int8[E][T+1][state_len] is caller-owned
 * and laid out like one slot of the replay ring's state tensor (slot 0 = s[0], slot t + 1 = s_next[t]).  Per lock-step, in the
 * unfused order: Q-net + pick, dmfb_vec_step (no autoreset), rollout_stream_step with parity p, _stage_close, dmfb_vec_reset with
 * the step's terminated flags as mask, _stage_first with the same mask.
 * _stage_first: stage[e][0] = state(e) for the chips whose mask byte is non-zero (d_mask NULL = all); after every reset.
 * _stage_close: for every chip e, t = d_t_ep[e] (row p of rollout_stage::d_t_ep: the row rollout_stream_step read, which it does
 *   not write):  stage[e][t + 1] = state(e);  then if 0 <= d_close_slot[e] < slots, rows 0 .. t + 1 of stage[e] are copied into
 *   d_ring_s + d_close_slot[e] * (T + 1) * state_len and rows t + 2 .. T of that slot are zeroed.  A chip whose t lies outside
 *   [0, T) is not touched, and a slot outside [0, slots) is not written.
 * DMFB_ERR_BAD_ARG, before anything is launched, for a NULL pointer (d_mask excepted), T < 1, slots < n_envs (every chip may close
 * in the same lock-step, as in rollout_stream_step) or a state row over 64 KiB. */
int dmfb_vec_global_obs_stage_first(const dmfb_vec *h, const uint8_t *d_mask, int32_t T, int8_t *d_stage, void *stream);
int dmfb_vec_global_obs_stage_close(const dmfb_vec *h, const int32_t *d_t_ep, const int32_t *d_close_slot, int32_t T,
                                    int8_t *d_stage, int8_t *d_ring_s, int32_t slots, void *stream);

/* Route record of a lock-step episode (no reference counterpart: its evaluate.py --show draws the routes one chip at a time):
 * d_route uint8[E][T+1][n][2], caller-owned, 2-byte aligned.  Slot t + 1 = every chip's droplet positions (x, y) after
 * lock-step t; t == -1 writes slot 0 (the positions after reset / restart).  Frozen chips are written too: the env leaves their
 * state alone, so their last position repeats up to slot T.  One launch, graph-capturable.  DMFB_ERR_BAD_ARG, before anything
 * is launched, for a NULL or odd d_route, T < 1 or t outside [-1, T). */
int dmfb_vec_route_append(const dmfb_vec *h, int32_t t, int32_t T, uint8_t *d_route, void *stream);

/* Action shield (no reference counterpart; the rule in numpy: marl_dmfb_amd/shield.py: shield_reference, the argument:
 * DESIGN.md section 10).  Called after the Q-network's pick and before dmfb_vec_step, it replaces every pick that could break a
 * constraint of moveDroplets (dmfb.py:254-271) by that droplet's best-Q action that cannot.  It reads the handle's own state
 * (positions, goals, blocks, stall).  Per chip whose d_active byte is non-zero (NULL = all), droplets in index order i = 0 .. n-1:
 *   exec(i, u) = old_i if stall and droplet i is on its goal; else old_i + delta(u), each axis clamped onto the chip, and old_i
 *     again if that cell lies in a block.  Actions: 0 STALL, 1 RIGHT, 2 LEFT, 3 DOWN, 4 UP.
 *   candidates: first d_actions[e][i] if it lies in [0, 5), then the remaining actions by descending d_q[e][i][a] (float `>`, ties
 *     to the lower action, a NaN below every number).
 *   a candidate u with c = exec(i, u) is safe iff cheb(c, old_j) >= 2 for every j != i and cheb(c, new_j) >= 2 for every j < i.
 *   Droplet i takes its first safe candidate, new_i = c.  With none safe (the chip was not conflict-free before the step) its
 *   pick stays, new_i = exec(i, pick), and d_unsafe[e] is set to 1.
 * d_overrides[e] += the droplets whose action changed.  For every droplet of an active chip d_actions int32[E*n] and its row of
 * d_last_onehot int8[E*n][5] hold the final action; when d_ep_u int8[E][T][n] and d_ep_onehot int8[E][T][n][5] are given (T =
 * episode_limit) slot d_t_ep ? d_t_ep[e] : t holds it too (the slot the pick kernels of rollout_ops.h staged into); a d_t_ep[e]
 * outside [0, T) skips that chip's staging.  Nothing else is written.  One asynchronous launch, graph-capturable.
 * DMFB_ERR_BAD_ARG, before anything is launched, for a NULL h, d_q, d_actions or d_last_onehot, for only one pointer of the
 * d_ep_* pair, and, when the pair is given, for episode_limit < 1 or t outside [0, T) with d_t_ep NULL. */
int dmfb_vec_shield(const dmfb_vec *h, const float *d_q /*[E*n][5]*/, const uint8_t *d_active /*[E] or NULL*/,
                    int32_t *d_actions /*[E*n] in/out*/, int8_t *d_last_onehot /*[E*n][5]*/,
                    int8_t *d_ep_u /*[E][T][n]*/, int8_t *d_ep_onehot /*[E][T][n][5]*/, int32_t episode_limit, int32_t t,
                    const int32_t *d_t_ep /*[E] or NULL*/, int32_t *d_overrides /*[E] or NULL*/, uint8_t *d_unsafe /*[E] or NULL*/,
                    void *stream);

/* routing_manager.m_health / m_usage / m_degrade as float64[E][width][length]. */
int dmfb_vec_get_map(const dmfb_vec *h, int which, double *d_buf, void *stream);
int dmfb_vec_set_map(dmfb_vec *h, int which, const double *d_buf, void *stream);

/* How the handle maps chips to workgroups (profiling aid; no reference counterpart): out[0] = chips per 256-thread
 * workgroup of the fused step+observe launch, out[1] = chips per tile of the observation kernel, out[2] = batch size
 * from which dmfb_vec_step issues a step-only launch followed by the observation kernel, out[3] = chips per workgroup of
 * that step-only launch, out[4] = workgroups of the (persistent) observation kernel, out[5] = its threads per workgroup. */
int dmfb_vec_launch_shape(const dmfb_vec *h, int32_t out[6]);

/* Measurement aid (no reference counterpart): while enabled, every launch of the observation kernel (standalone or as the
 * second launch of dmfb_vec_step at large batches) carries a HIP event pair that receives the dispatch's own start and end
 * time stamps -- the duration rocprofv3 --kernel-trace reports.  _read waits for the timed launches (host-synchronising),
 * returns their summed duration in microseconds and their count (at most 256 per read) and starts a new series. */
int dmfb_vec_observe_timing(dmfb_vec *h, int enable);
int dmfb_vec_observe_timing_read(dmfb_vec *h, double *total_us, int *launches);

/* Direction-vector zoom table (dmfb.py:444-453) the handle was built with: int8[2][511], host memory. */
int dmfb_vec_zoom_lut(const dmfb_vec *h, int8_t *host_out);

const char *dmfb_vec_strerror(int code);
int dmfb_vec_last_hip_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DMFB_VEC_H */
