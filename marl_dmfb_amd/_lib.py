"""ctypes loader for the HIP libraries built in-tree (marl_dmfb_amd/lib/*.so).

Every function of the twenty C ABI headers (include/*.h; thirteen libraries: rollout_route.h, vdn_tail.h, vdn_lambda.h,
vdn_double.h, qmix_packed.h, qmix_lambda.h and qmix_double.h are built into librollout_ops.so, libvdn_ops.so and libqmix_ops.so) is declared once, in SIGNATURES.  `dmfb_vec()` ...
`vdn_ops()` return the raw typed library (return codes are the caller's); `checked(name)` returns a
second view of the same library whose status functions raise on a non-zero return code.

Fails loudly when a library is missing: the product path has no CPU fallback."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, 'lib')
_CACHE = {}
# binding table -> the library file that exports it, where the two differ
_FILE = {'rollout_route': 'rollout_ops', 'vdn_tail': 'vdn_ops', 'vdn_lambda': 'vdn_ops', 'vdn_double': 'vdn_ops',
         'qmix_packed': 'qmix_ops', 'qmix_lambda': 'qmix_ops', 'qmix_double': 'qmix_ops'}


class HipLibraryMissing(RuntimeError):
    pass


def load(name):
    if name in _CACHE:
        return _CACHE[name]
    # MARL_DMFB_VARIANT_<NAME>=_tag loads lib<name>_tag.so instead: same-box A/B timing of a kernel variant (development aid)
    stem = _FILE.get(name, name)
    path = os.path.join(LIB_DIR, 'lib%s%s.so' % (stem, os.environ.get('MARL_DMFB_VARIANT_' + stem.upper(), '')))
    if not os.path.exists(path):
        raise HipLibraryMissing(
            '%s not found: build the HIP extension first (python -c "import __graft_entry__ as g; g.build()" '
            'or make -C marl_dmfb_amd/csrc). There is no CPU fallback.' % path)
    # PyTorch bundles its own HIP runtime (SONAME libamdhip64.so.7).  It must be in the process
    # BEFORE our library is opened, so that the library's NEEDED entry binds to that same runtime:
    # two HIP runtimes in one process cannot share devices, streams or pointers.
    import torch  # noqa: F401
    lib = C.CDLL(path)
    _CACHE[name] = lib
    return lib


class DmfbVecConfig(C.Structure):
    """include/dmfb_vec.h: dmfb_vec_config"""
    _fields_ = [('width', C.c_int32), ('length', C.c_int32), ('n_agents', C.c_int32), ('n_blocks', C.c_int32),
                ('fov', C.c_int32), ('stall', C.c_int32), ('b_degrade', C.c_int32), ('with_maps', C.c_int32),
                ('per_degrade', C.c_double), ('n_envs', C.c_int32), ('env_id0', C.c_uint32), ('seed', C.c_uint64),
                ('device', C.c_int32)]


class DmfbVecStepOut(C.Structure):
    """include/dmfb_vec.h: dmfb_vec_step_out"""
    _fields_ = [('d_rewards', C.c_void_p), ('d_dones', C.c_void_p), ('d_constraints', C.c_void_p),
                ('d_success', C.c_void_p), ('d_obs', C.c_void_p), ('d_team_reward', C.c_void_p),
                ('d_terminated', C.c_void_p), ('d_obs_terminal', C.c_void_p)]


class MedaVecConfig(C.Structure):
    """include/meda_vec.h: meda_vec_config"""
    _fields_ = [('width', C.c_int32), ('length', C.c_int32), ('n_agents', C.c_int32), ('fov', C.c_int32),
                ('b_degrade', C.c_int32), ('with_maps', C.c_int32), ('per_degrade', C.c_double), ('n_envs', C.c_int32),
                ('env_id0', C.c_uint32), ('seed', C.c_uint64), ('device', C.c_int32), ('obs_version', C.c_int32)]


class MedaVecStepOut(C.Structure):
    """include/meda_vec.h: meda_vec_step_out"""
    _fields_ = [('d_rewards', C.c_void_p), ('d_dones', C.c_void_p), ('d_fail', C.c_void_p), ('d_success', C.c_void_p),
                ('d_obs', C.c_void_p), ('d_team_reward', C.c_void_p), ('d_terminated', C.c_void_p)]


# include/rollout_ops.h: ROLLOUT_STREAM_MAX_ENVS, the most chips rollout_stream_step takes
ROLLOUT_STREAM_MAX_ENVS = 32768


class RolloutStage(C.Structure):
    """include/rollout_ops.h: rollout_stage"""
    _fields_ = [('d_t_ep', C.c_void_p), ('d_o0', C.c_void_p), ('d_o_next', C.c_void_p), ('d_u', C.c_void_p),
                ('d_onehot', C.c_void_p), ('d_r', C.c_void_p), ('d_ep_acc', C.c_void_p), ('d_chip_acc', C.c_void_p),
                ('d_close_slot', C.c_void_p), ('d_state_alt', C.c_void_p)]


class RolloutRing(C.Structure):
    """include/rollout_ops.h: rollout_ring"""
    _fields_ = [('slots', C.c_int32), ('d_o', C.c_void_p), ('d_o_next', C.c_void_p), ('d_u', C.c_void_p),
                ('d_u_onehot', C.c_void_p), ('d_avail_u', C.c_void_p), ('d_avail_u_next', C.c_void_p), ('d_r', C.c_void_p),
                ('d_padded', C.c_void_p), ('d_terminated', C.c_void_p), ('d_len', C.c_void_p), ('d_stats', C.c_void_p),
                ('d_state', C.c_void_p)]


class QmixMixer(C.Structure):
    """include/qmix_ops.h: qmix_mixer"""
    _fields_ = [('w1', C.c_void_p), ('b1', C.c_void_p), ('w2', C.c_void_p), ('b2', C.c_void_p), ('wb', C.c_void_p),
                ('bb', C.c_void_p)]


vp, i32, u32, i64, u64, f32, f64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_float, C.c_double
_dmfb_cfg, _meda_cfg = C.POINTER(DmfbVecConfig), C.POINTER(MedaVecConfig)
_i32p, _f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)

# library -> {function: argtypes} for the status functions (int return code, 0 = ok: checked() raises on anything else),
# {function: (argtypes, restype)} for the functions that return a value
SIGNATURES = {
    'dmfb_vec': {  # include/dmfb_vec.h
        'dmfb_vec_check_config': [_dmfb_cfg],
        'dmfb_vec_create': [_dmfb_cfg, vp, C.POINTER(vp)],
        'dmfb_vec_destroy': [vp],
        'dmfb_vec_state_bytes': ([vp], C.c_size_t),
        'dmfb_vec_obs_len': ([vp], i32),
        'dmfb_vec_max_step': ([vp], i32),
        'dmfb_vec_n_envs': ([vp], i32),
        'dmfb_vec_n_agents': ([vp], i32),
        'dmfb_vec_reset': [vp, vp, i32, vp, vp],
        'dmfb_vec_restart': [vp, vp, vp, vp],
        'dmfb_vec_set_task': [vp, vp, vp, vp],
        'dmfb_vec_get_task': [vp, vp, vp, vp],
        'dmfb_vec_set_blocks': [vp, vp, i32, vp],
        'dmfb_vec_get_blocks': [vp, vp, _i32p, vp],
        'dmfb_vec_step': [vp, vp, vp, vp, u32, C.POINTER(DmfbVecStepOut), vp],
        'dmfb_vec_observe': [vp, vp, vp, vp],
        'dmfb_vec_get_state': [vp, vp, vp, vp, vp, vp],
        'dmfb_vec_state_len': ([vp], i32),
        'dmfb_vec_global_obs': [vp, vp, vp, vp],
        'dmfb_vec_global_obs_append': [vp, vp, vp, i32, i32, vp, vp, vp],
        'dmfb_vec_global_obs_stage_first': [vp, vp, i32, vp, vp],
        'dmfb_vec_global_obs_stage_close': [vp, vp, vp, i32, vp, vp, i32, vp],
        'dmfb_vec_route_append': [vp, i32, i32, vp, vp],
        'dmfb_vec_shield': [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp],
        'dmfb_vec_get_map': [vp, i32, vp, vp],
        'dmfb_vec_set_map': [vp, i32, vp, vp],
        'dmfb_vec_launch_shape': [vp, C.POINTER(C.c_int32 * 6)],
        'dmfb_vec_observe_timing': [vp, i32],
        'dmfb_vec_observe_timing_read': [vp, _f64p, _i32p],
        'dmfb_vec_zoom_lut': [vp, vp],
        'dmfb_vec_strerror': ([i32], C.c_char_p),
        'dmfb_vec_last_hip_error': ([], i32),
    },
    'meda_vec': {  # include/meda_vec.h
        'meda_vec_check_config': [_meda_cfg],
        'meda_vec_create': [_meda_cfg, vp, C.POINTER(vp)],
        'meda_vec_destroy': [vp],
        'meda_vec_state_bytes': ([vp], C.c_size_t),
        'meda_vec_obs_len': ([vp], i32),
        'meda_vec_max_step': ([vp], i32),
        'meda_vec_n_envs': ([vp], i32),
        'meda_vec_n_agents': ([vp], i32),
        'meda_vec_reset': [vp, vp, vp, vp],
        'meda_vec_restart': [vp, vp, vp, vp],
        'meda_vec_set_task': [vp, vp, vp, vp],
        'meda_vec_get_task': [vp, vp, vp, vp],
        'meda_vec_step': [vp, vp, vp, vp, u32, C.POINTER(MedaVecStepOut), vp],
        'meda_vec_observe': [vp, vp, vp, vp],
        'meda_vec_get_state': [vp, vp, vp, vp, vp, vp],
        'meda_vec_state_len': ([vp], i32),
        'meda_vec_global_obs': [vp, vp, vp, vp],
        'meda_vec_global_obs_append': [vp, vp, vp, i32, i32, vp, vp, vp],
        'meda_vec_global_obs_stage_first': [vp, vp, i32, vp, vp],
        'meda_vec_global_obs_stage_close': [vp, vp, vp, i32, vp, vp, i32, vp],
        'meda_vec_route_append': [vp, i32, i32, vp, vp],
        'meda_vec_shield': [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp],
        'meda_vec_get_map': [vp, i32, vp, vp],
        'meda_vec_set_map': [vp, i32, vp, vp],
        'meda_vec_launch_shape': [vp, C.POINTER(C.c_int32 * 4)],
        'meda_vec_observe_timing': [vp, i32],
        'meda_vec_observe_timing_read': [vp, _f64p, _i32p],
        'meda_vec_strerror': ([i32], C.c_char_p),
        'meda_vec_last_hip_error': ([], i32),
    },
    'crnn_fov': {  # include/crnn_fov.h: the front end for fov 5 and 7
        'crnn_fov_front_forward': [i32, vp, i64, vp, i32, i64, vp, vp, vp, vp, vp, vp, i32, vp, i64, i32, vp],
        'crnn_fov_padded_cols': ([i32, i32], i32),
        'crnn_fov_backward_parts': ([i32, i32], i32),
        'crnn_fov_backward': [i32, vp, i64, i64, vp, i64, vp, i64, vp, vp, vp, i32, vp, i32, vp, vp],
        'crnn_fov_last_hip_error': ([], i32),
    },
    'crnn_wide': {  # include/crnn_wide.h: the front end for fov 11 and 13
        'crnn_wide_front_forward': [i32, vp, i64, vp, i32, i64, vp, vp, vp, vp, vp, vp, i32, vp, i64, i32, vp],
        'crnn_wide_padded_cols': ([i32, i32], i32),
        'crnn_wide_forward_block_rows': ([i32, i32], i32),
        'crnn_wide_backward_block_rows': ([i32, i32], i32),
        'crnn_wide_backward_parts': ([i32, i32], i32),
        'crnn_wide_backward': [i32, vp, i64, i64, vp, i64, vp, i64, vp, vp, vp, i32, vp, i32, vp, vp],
        'crnn_wide_last_hip_error': ([], i32),
    },
    'crnn_ops': {  # include/crnn_ops.h (crnn_ops.hip and gru_ops.hip)
        'crnn_conv9_forward': [vp, i64, i64, vp, vp, vp, vp, i32, vp, i64, vp],
        'crnn_front9_forward': [vp, i64, vp, i32, i64, vp, vp, vp, vp, vp, vp, i32, vp, i64, i32, vp],
        'crnn_front9_forward_live': [vp, i64, vp, i32, i64, vp, vp, vp, vp, vp, vp, i32, vp, i64, i32, vp, vp, i32, vp],
        'crnn_front19_forward': [vp, i64, vp, i32, i64, vp, vp, vp, vp, vp, vp, i32, vp, i64, i32, vp],
        'crnn_front_padded_cols': ([i32], i32),
        'crnn_conv9_backward_parts': ([i32], i32),
        'crnn_conv9_backward': [vp, i64, i64, vp, i64, vp, i64, vp, vp, vp, i32, vp, i32, vp, vp],
        'crnn_mlp_backward_parts': ([], i32),
        'crnn_mlp_backward': [vp, i64, i32, vp, i32, i64, vp, i64, vp, i64, i32, vp, vp, vp, vp],
        'crnn_conv19_backward_parts': ([i32], i32),
        'crnn_conv19_backward': [vp, i64, i64, vp, i64, vp, i64, vp, vp, vp, vp, i32, vp, i32, vp, vp],
        'crnn_last_hip_error': ([], i32),
        'gru_seq_forward': [vp, vp, vp, vp, vp, i32, i64, i32, vp, vp, vp],
        'gru_seq_backward': [vp, vp, vp, vp, vp, i32, i64, i32, vp, vp, vp, vp, vp],
        'gru_seq_forward_packed': [vp, vp, vp, vp, vp, i32, i64, i32, _i32p, vp, vp, vp],
        'gru_seq_forward_packed_pair': [vp] * 14 + [i32, i64, i32, _i32p, vp],
        'gru_seq_backward_packed': [vp, vp, vp, vp, vp, i32, i64, i32, _i32p, vp, vp, vp, vp, vp, vp],
        'gru_seq_row_blocks': ([i64], i64),
        'gru_last_hip_error': ([], i32),
    },
    'rollout_ops': {  # include/rollout_ops.h
        'rollout_select_actions': [vp, i32, i32, i32, vp, i32, u64, vp, vp, vp, vp, vp, i32, i32, vp],
        'rollout_gru_head_select': [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, u64, vp, vp, vp, vp, vp, i32, i32, vp, vp],
        'rollout_gru_head_select_live': [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, u64, vp, vp, vp, vp, vp, i32, i32, vp, vp,
                                         vp, vp],
        'rollout_compact_alive': [i32, vp, vp, vp, vp],
        'rollout_post_step': [i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, f32, vp, vp, vp, i32, vp, vp,
                              vp],
        'rollout_gru_head_select_stream': [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, u64, vp, vp, vp, vp, vp, i32, vp, vp,
                                           vp],
        'rollout_stream_step': [i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, C.POINTER(RolloutStage),
                                C.POINTER(RolloutRing), i32, vp, vp, vp, f32, f32, vp, vp],
        'rollout_last_hip_error': ([], i32),
    },
    'rollout_route': {  # include/rollout_route.h (built into librollout_ops.so)
        'rollout_route_select': [i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp],
        'rollout_last_hip_error': ([], i32),
    },
    'route_plan': {  # include/route_plan.h
        'route_plan_dmfb': [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        'route_follow_dmfb': [i32] * 6 + [vp] * 16,
        'route_plan_dmfb_opt': [i32] * 5 + [vp] * 10 + [i32, i32, vp],
        'route_follow_dmfb_opt': [i32] * 6 + [vp] * 15 + [i32, i32, vp],
        'route_plan_max_dim': ([], i32),
        'route_plan_lds_bytes': ([i32, i32, i32], i32),
        'route_plan_last_hip_error': ([], i32),
    },
    'meda_plan': {  # include/meda_plan.h
        'meda_plan_route': [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        'meda_plan_max_dim': ([], i32),
        'meda_plan_lds_bytes': ([i32, i32, i32], i32),
        'meda_plan_last_hip_error': ([], i32),
    },
    'meda_follow': {  # include/meda_follow.h
        'meda_follow_plan': [i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        'meda_follow_step': [i32] * 5 + [vp] * 16,
        'meda_follow_max_dim': ([], i32),
        'meda_follow_lds_bytes': ([i32, i32, i32], i32),
        'meda_follow_last_hip_error': ([], i32),
    },
    'meda_plan_wide': {  # include/meda_plan_wide.h: chips up to 128 x 128
        'meda_plan_wide_route': [i32] * 5 + [vp] * 10 + [i64, i32, vp],
        'meda_plan_wide_max_dim': ([], i32),
        'meda_plan_wide_max_groups': ([], i32),
        'meda_plan_wide_lds_levels': ([i32, i32, i32], i32),
        'meda_plan_wide_lds_bytes': ([i32, i32, i32, i32], i32),
        'meda_plan_wide_work_bytes': ([i32, i32, i32, i32, i32], i64),
        'meda_plan_wide_last_hip_error': ([], i32),
    },
    'meda_follow_wide': {  # include/meda_follow_wide.h: the closed loop on chips up to 128 x 128
        'meda_follow_wide_step': [i32] * 5 + [vp] * 16 + [i64, i32, vp],
        'meda_follow_wide_max_dim': ([], i32),
        'meda_follow_wide_max_groups': ([], i32),
        'meda_follow_wide_lds_levels': ([i32, i32, i32], i32),
        'meda_follow_wide_lds_bytes': ([i32, i32, i32, i32], i32),
        'meda_follow_wide_work_bytes': ([i32, i32, i32, i32, i32], i64),
        'meda_follow_wide_last_hip_error': ([], i32),
    },
    'vdn_ops': {  # include/vdn_ops.h
        'vdn_td_forward': [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp],
        'vdn_td_backward': [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp],
        'vdn_td_forward_packed': [vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, f32, vp, vp, vp, vp],
        'vdn_td_backward_packed': [vp, vp, vp, i32, vp, vp, i32, i32, vp, vp],
        'vdn_gather_units': [vp, i32, vp, i32, i32, i32, vp, vp],
        'vdn_clip_adam_step': [i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), f32, f64, f64, f64,
                               f64, f64, f64, vp, vp, vp, vp],
        'vdn_last_hip_error': ([], i32),
    },
    'vdn_tail': {  # include/vdn_tail.h (built into libvdn_ops.so)
        'vdn_td_sum_parts': ([i64], i32),
        'vdn_td_forward_sums': [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp],
        'vdn_td_forward_packed_sums': [vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, f32, vp, vp, vp, vp, vp, vp],
        'vdn_td_backward_packed_pad': [vp, vp, vp, i32, vp, vp, i32, i32, i64, vp, vp],
        'vdn_gather_units_batch': [i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(vp), C.POINTER(i64), vp,
                                   i32, vp],
    },
    'vdn_lambda': {  # include/vdn_lambda.h (built into libvdn_ops.so)
        'vdn_td_lambda_sum_parts': ([i64], i32),
        'vdn_td_lambda_forward_sums': [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, f32, vp, vp],
        'vdn_td_lambda_forward_packed_sums': [vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, f32, vp, vp, vp, vp, vp, f32, vp, i32,
                                              _i32p, vp],
    },
    'vdn_double': {  # include/vdn_double.h (built into libvdn_ops.so): the lambda forwards + q_sel [, n_sel_units, sel_units], picks
        'vdn_td_double_forward_sums': [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, f32, vp, vp, vp, vp],
        'vdn_td_double_forward_packed_sums': [vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, f32, vp, vp, vp, vp, vp, f32, vp, i32,
                                              _i32p, vp, i32, vp, vp, vp],
    },
    'qmix_ops': {  # include/qmix_ops.h
        'qmix_mix_td_forward': [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, vp, i32, i32, i32, i32,
                                C.POINTER(QmixMixer), C.POINTER(QmixMixer), f32, vp, vp, vp, vp],
        'qmix_mix_td_backward': [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, i32, i32, C.POINTER(QmixMixer), vp, vp, vp,
                                 vp, vp, vp],
        'qmix_last_hip_error': ([], i32),
    },
    'qmix_packed': {  # include/qmix_packed.h (built into libqmix_ops.so)
        'qmix_mix_td_forward_packed': [vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, i32, C.POINTER(QmixMixer),
                                       C.POINTER(QmixMixer), f32, vp, vp, vp, vp],
        'qmix_mix_td_backward_packed': [vp, vp, vp, vp, i32, vp, i32, i32, i32, vp, i32, i32, C.POINTER(QmixMixer), vp, vp, vp, vp, vp,
                                        vp],
        'qmix_gather_states': [vp, i64, i32, vp, i32, vp, vp],
    },
    'qmix_lambda': {  # include/qmix_lambda.h (built into libqmix_ops.so): the one-step forwards + lam, q_tot_eval, q_tot_target, targets
        'qmix_mix_td_lambda_forward': [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, vp, i32, i32, i32, i32,
                                       C.POINTER(QmixMixer), C.POINTER(QmixMixer), f32, vp, vp, vp, f32, vp, vp, vp, vp],
        'qmix_mix_td_lambda_forward_packed': [vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, i32, C.POINTER(QmixMixer),
                                              C.POINTER(QmixMixer), f32, vp, vp, vp, f32, vp, vp, vp, i32, _i32p, vp],
    },
    'qmix_double': {  # include/qmix_double.h (built into libqmix_ops.so): the lambda forwards + q_sel [, n_sel_units, sel_units], picks
        'qmix_mix_td_double_forward': [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i32, i32, vp, i32, i32, i32, i32,
                                       C.POINTER(QmixMixer), C.POINTER(QmixMixer), f32, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp],
        'qmix_mix_td_double_forward_packed': [vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, i32, C.POINTER(QmixMixer),
                                              C.POINTER(QmixMixer), f32, vp, vp, vp, f32, vp, vp, vp, i32, _i32p, vp, i32, vp, vp, vp],
    },
}

DMFB_VEC_SYMBOLS = list(SIGNATURES['dmfb_vec'])
MEDA_VEC_SYMBOLS = list(SIGNATURES['meda_vec'])

# error code -> the exception the reference raises for the same condition (what checked() raises for the env libraries)
ENV_ERRORS = {
    'dmfb_vec': {
        -1: (ValueError, 'bad argument'),
        -2: (RuntimeError, 'Fov is too large'),             # env/DMFB/dmfb.py:139-140
        -3: (TypeError, 'Too many droplets for DMFB'),       # env/DMFB/dmfb.py:144-146
        -4: (AssertionError, 'width >= 5 and length >= 5'),  # env/DMFB/dmfb.py:489
        -5: (AssertionError, 'n_agents > 0'),                # env/DMFB/dmfb.py:490
        -6: (NotImplementedError, 'configuration outside the build limits (include/dmfb_vec.h)'),
        -7: (TypeError, 'action is illegal'),                # env/DMFB/dmfb.py:116
        -8: (RuntimeError, 'env was created without health/usage/degrade maps (pass with_maps=True)'),
    },
    'meda_vec': {
        -1: (ValueError, 'bad argument'),
        -3: (RuntimeError, 'Too many droplets in the MEDA array'),   # env/MEDA/meda.py:151-154
        -4: (AssertionError, 'w > 0 and l > 0'),                     # env/MEDA/meda.py:472
        -5: (AssertionError, 'n_agents > 0'),                        # env/MEDA/meda.py:473
        -6: (NotImplementedError, 'configuration outside the build limits (include/meda_vec.h)'),
        -8: (RuntimeError, 'env was created without health/usage/degrade maps (pass with_maps=True)'),
    },
    'route_plan': {
        -1: (ValueError, 'bad argument'),
        -6: (NotImplementedError, 'chip larger than the planner takes (include/route_plan.h: ROUTE_PLAN_MAX_DIM)'),
    },
    'meda_plan': {
        -1: (ValueError, 'bad argument'),
        -6: (NotImplementedError, 'chip larger or more droplets than the planner takes (include/meda_plan.h: MEDA_PLAN_MAX_DIM, '
                                  'MEDA_PLAN_MAX_AGENTS)'),
    },
    'meda_plan_wide': {
        -1: (ValueError, 'bad argument'),
        -6: (NotImplementedError, 'chip larger or more droplets than the wide planner takes (include/meda_plan_wide.h: '
                                  'MEDA_PLAN_WIDE_MAX_DIM, MEDA_PLAN_WIDE_MAX_AGENTS)'),
    },
    'meda_follow': {
        -1: (ValueError, 'bad argument'),
        -6: (NotImplementedError, 'chip larger or more droplets than the follower takes (include/meda_follow.h: MEDA_FOLLOW_MAX_DIM, '
                                  'MEDA_FOLLOW_MAX_AGENTS)'),
    },
    'meda_follow_wide': {
        -1: (ValueError, 'bad argument'),
        -6: (NotImplementedError, 'chip larger or more droplets than the wide follower takes (include/meda_follow_wide.h: '
                                  'MEDA_FOLLOW_WIDE_MAX_DIM, MEDA_FOLLOW_WIDE_MAX_AGENTS)'),
    },
}
HIP_ERROR = -100  # *_ERR_HIP of every library
# function prefix -> the function that returns the last HIP error of its translation unit
_LAST_ERROR = {'dmfb_vec_': 'dmfb_vec_last_hip_error', 'meda_vec_': 'meda_vec_last_hip_error',
               'meda_plan_wide_': 'meda_plan_wide_last_hip_error', 'meda_plan_': 'meda_plan_last_hip_error',
               'meda_follow_wide_': 'meda_follow_wide_last_hip_error', 'meda_follow_': 'meda_follow_last_hip_error',
               'crnn_fov_': 'crnn_fov_last_hip_error', 'crnn_wide_': 'crnn_wide_last_hip_error', 'crnn_': 'crnn_last_hip_error',
               'gru_': 'gru_last_hip_error', 'rollout_': 'rollout_last_hip_error', 'route_plan_': 'route_plan_last_hip_error', 'route_follow_': 'route_plan_last_hip_error', 'vdn_': 'vdn_last_hip_error',
               'qmix_': 'qmix_last_hip_error'}


def _typed(lib, name):
    for fn, sig in SIGNATURES[name].items():
        f = getattr(lib, fn)
        if isinstance(sig, tuple):
            f.argtypes, f.restype = sig
        else:
            f.argtypes = sig
    return lib


def _raiser(name, lib):
    """errcheck of the status functions of library `name`: raises on a non-zero return code."""
    errors = ENV_ERRORS.get(name)

    def errcheck(rc, func, args):
        if rc == 0:
            return rc
        fn = func.__name__
        last = getattr(lib, _LAST_ERROR[next(p for p in _LAST_ERROR if fn.startswith(p))])
        if errors is None:
            raise RuntimeError('%s failed: %d (hip %d)' % (fn, rc, last()))
        if rc == HIP_ERROR:
            raise RuntimeError('HIP runtime error %d in %s' % (last(), name))
        exc, msg = errors.get(rc, (RuntimeError, '%s error %d' % (name, rc)))
        raise exc(msg)
    return errcheck


def _library(name):
    lib = load(name)
    if not getattr(lib, '_typed', False):
        _typed(lib, name)
        lib._typed = True
    return lib


def checked(name):
    """The library `name` with every status function raising on failure: RuntimeError('<function> failed: <code>
    (hip <error>)') for the op libraries, the reference's exception (ENV_ERRORS) for the environment libraries."""
    key = name + ':checked'
    if key not in _CACHE:
        raw = _library(name)
        lib = _typed(C.CDLL(raw._name), name)
        errcheck = _raiser(name, raw)
        for fn, sig in SIGNATURES[name].items():
            if not isinstance(sig, tuple):
                getattr(lib, fn).errcheck = errcheck
        _CACHE[key] = lib
    return _CACHE[key]


def dmfb_vec():
    return _library('dmfb_vec')


def meda_vec():
    return _library('meda_vec')


def crnn_ops():
    return _library('crnn_ops')


def crnn_fov():
    return _library('crnn_fov')


def crnn_wide():
    return _library('crnn_wide')


def rollout_ops():
    return _library('rollout_ops')


def rollout_route():
    return _library('rollout_route')


def route_plan():
    return _library('route_plan')


def meda_plan():
    return _library('meda_plan')


def meda_follow():
    return _library('meda_follow')


def meda_plan_wide():
    return _library('meda_plan_wide')


def meda_follow_wide():
    return _library('meda_follow_wide')


def vdn_ops():
    return _library('vdn_ops')


def vdn_tail():
    return _library('vdn_tail')


def vdn_lambda():
    return _library('vdn_lambda')


def vdn_double():
    return _library('vdn_double')


def qmix_ops():
    return _library('qmix_ops')


def qmix_packed():
    return _library('qmix_packed')


def qmix_lambda():
    return _library('qmix_lambda')


def qmix_double():
    return _library('qmix_double')
