"""Host side of closed-loop planner routing for MEDA on chips up to 128 x 128 (marl_dmfb_amd.plan.MedaWideFollower /
MedaWideFollowPlanner, include/meda_follow_wide.h): the header against the binding table, the limits, the size queries, the argument
guards without a GPU, and the cases of tests/test_gpu_meda_follow_wide.py through follow_reference_meda with the CPU oracle as
judge.  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from marl_dmfb_amd import _lib
from meda_follow_helpers import judge, parking_never_takes_a_droplet_inside_its_disc, partial_plans
from meda_follow_wide_helpers import CASES, FEW_LEVELS, case, reference
from meda_plan_wide_helpers import LDS_BUDGET, lds_levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- C ABI
def test_meda_follow_wide_header_matches_the_binding_table():
    txt = open(os.path.join(ROOT, 'include', 'meda_follow_wide.h')).read()
    define = lambda name: int(re.search(r'#define MEDA_FOLLOW_WIDE_%s\s+(\d+)' % name, txt).group(1))
    limit, least, most, groups = define('MAX_DIM'), define('MIN_DIM'), define('MAX_AGENTS'), define('MAX_GROUPS')
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    txt = re.sub(r'^\s*#.*$', '', txt, flags=re.M)
    declared = {name: (0 if p.strip() in ('', 'void') else p.count(',') + 1)
                for name, p in re.findall(r'\b([a-z][a-z_0-9]*)\s*\(([^()]*)\)\s*;', txt)}
    assert declared == {'meda_follow_wide_step': 24, 'meda_follow_wide_max_dim': 0, 'meda_follow_wide_max_groups': 0,
                        'meda_follow_wide_lds_levels': 3, 'meda_follow_wide_lds_bytes': 4, 'meda_follow_wide_work_bytes': 5,
                        'meda_follow_wide_last_hip_error': 0}
    table = _lib.SIGNATURES['meda_follow_wide']
    assert sorted(table) == sorted(declared)
    raw = _lib.meda_follow_wide()
    for name, n in declared.items():
        sig = table[name]
        argtypes = sig[0] if isinstance(sig, tuple) else sig
        assert len(argtypes) == n and len(getattr(raw, name).argtypes) == n, name
    # the lock-step is meda_follow_step's argument list with (d_work, work_bytes, lds_levels) before the stream
    narrow = _lib.SIGNATURES['meda_follow']['meda_follow_step']
    assert table['meda_follow_wide_step'] == narrow[:-1] + [_lib.vp, _lib.i64, _lib.i32] + narrow[-1:]
    from marl_dmfb_amd import plan
    assert raw.meda_follow_wide_max_dim() == limit == 128 == plan.MEDA_WIDE_MAX_DIM and least == 5 and most == 16
    assert raw.meda_follow_wide_max_groups() == groups == 512 == _lib.meda_plan_wide().meda_plan_wide_max_groups()
    assert plan.MEDA_MAX_DIM == 64 == _lib.meda_follow().meda_follow_max_dim()      # the narrow follower keeps its limit
    assert plan.MedaWideFollower.max_dim == 128 and plan.MedaWideFollower.library == 'meda_follow_wide'
    assert plan.MedaWideFollower.constraints_dtype == 'float64'


def test_the_prefix_table_and_the_error_classes():
    # the prefix table is matched in order: the wide library's functions must not fall to the narrow one's slot
    for fn, want in (('meda_follow_wide_step', 'meda_follow_wide_last_hip_error'), ('meda_follow_step', 'meda_follow_last_hip_error'),
                     ('meda_follow_plan', 'meda_follow_last_hip_error'), ('meda_plan_wide_route', 'meda_plan_wide_last_hip_error')):
        first = next(p for p in _lib._LAST_ERROR if fn.startswith(p))
        assert _lib._LAST_ERROR[first] == want, fn
    keys = list(_lib._LAST_ERROR)
    assert keys.index('meda_follow_wide_') < keys.index('meda_follow_')
    errors = _lib.ENV_ERRORS['meda_follow_wide']
    assert errors[-1][0] is ValueError and errors[-6][0] is NotImplementedError and 'include/meda_follow_wide.h' in errors[-6][1]


def test_size_queries():
    raw, plan = _lib.meda_follow_wide(), _lib.meda_plan_wide()
    groups = raw.meda_follow_wide_max_groups()
    paths = lambda w, l, n: ((w + l + 1) * n * 2 + 15) // 16 * 16
    shapes = ((128, 128, 16), (80, 80, 10), (65, 20, 1), (20, 65, 1), (5, 5, 1), (64, 64, 16), (63, 64, 3), (64, 65, 3), (30, 30, 4),
              (128, 5, 3), (100, 128, 7))
    for w, l, n in shapes:
        T = w + l
        H = min(T - 2, (LDS_BUDGET - paths(w, l, n) - 16 * w) // (16 * w))
        assert raw.meda_follow_wide_lds_levels(w, l, n) == H == lds_levels(w, l, n) == plan.meda_plan_wide_lds_levels(w, l, n), (w, l, n)
        for cap in (0, -3, 1, 8, H, H + 1, 1000):
            h = min(H, cap) if cap > 0 else H
            assert raw.meda_follow_wide_lds_bytes(w, l, n, cap) == (h + 1) * w * 16 + paths(w, l, n), (w, l, n, cap)
            for B in (0, 1, 7, groups, groups + 3, 4096):
                assert raw.meda_follow_wide_work_bytes(B, w, l, n, cap) == min(B, groups) * (T - 2 - h) * w * 16, (w, l, n, cap, B)
    for w, l, n in ((128, 128, 16), (80, 80, 10), (65, 20, 1)):
        assert 0 < raw.meda_follow_wide_lds_bytes(w, l, n, 0) <= 160 * 1024 - 1024
    assert raw.meda_follow_wide_work_bytes(64, 65, 20, 1, 0) == 0
    assert raw.meda_follow_wide_work_bytes(64, 128, 128, 16, 0) > 0 and raw.meda_follow_wide_work_bytes(64, 65, 20, 1, 8) > 0
    for fn, more in ((raw.meda_follow_wide_lds_levels, ()), (raw.meda_follow_wide_lds_bytes, (0,))):
        assert fn(129, 30, 4, *more) == -6 and fn(30, 129, 4, *more) == -6 and fn(30, 30, 17, *more) == -6
        assert fn(4, 30, 4, *more) == -1 and fn(30, 4, 4, *more) == -1 and fn(30, 30, 0, *more) == -1
    assert raw.meda_follow_wide_work_bytes(4, 129, 30, 4, 0) == -6 and raw.meda_follow_wide_work_bytes(-1, 30, 30, 4, 0) == -1
    # the cases that run with fewer levels than fit: 12 and 1 are below what fits, so levels move to the workspace
    for name in FEW_LEVELS:
        c = CASES[name]
        w, l, n = c['width'], c['length'], c['n_agents']
        need = [raw.meda_follow_wide_work_bytes(c['B'], w, l, n, cap) for cap in (0, 12, 1)]
        assert lds_levels(w, l, n) > 12 and 0 <= need[0] < need[1] < need[2], name


def test_meda_follow_wide_argument_guards_need_no_gpu():
    """Dummy non-null pointers in a child process that sees no GPU: a launch there would come back as a HIP error (-100), never as
    -1, -6 or 0."""
    child = r'''
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from marl_dmfb_amd import _lib
lib = _lib.meda_follow_wide()
host = C.create_string_buffer(4096)
p = C.addressof(host) + 15 & ~15
names = ('goals', 'avoid', 'positions', 'terminated', 'route', 'route_u', 'cursor', 'partial', 'replans', 'gave_up', 'active',
         'steps', 'lower', 'actions', 'u')
def step(B=4, W=30, L=30, n=4, t=0, work=None, wb=0, levels=0, **ptr):
    a = dict({k: p for k in names}, avoid=None)
    a.update(ptr)
    return lib.meda_follow_wide_step(B, W, L, n, t, *[a[k] for k in names], work, wb, levels, None)
M = lib.meda_follow_wide_max_dim()
need = lib.meda_follow_wide_work_bytes(4, 65, 20, 1, 8)
print(step(B=-1), step(W=0), step(L=-3), step(W=4), step(L=4), step(n=0), step(t=-1), step(t=60), step(W=M, L=M, t=2 * M),
      step(positions=p + 1), step(route=p + 1), *[step(**{k: None}) for k in names if k != 'avoid'])
print(step(W=65, L=20, n=1, levels=8), step(W=65, L=20, n=1, levels=8, work=p, wb=need - 1), step(W=65, L=20, n=1, levels=8, wb=need),
      step(W=M, L=M, n=16), step(W=M, L=M, n=16, work=p, wb=4096), step(W=65, L=20, n=1, levels=8, work=p + 8, wb=need))
print(step(W=M + 1), step(L=M + 1), step(n=17), step(W=M + 1, L=M + 1, n=16), step(W=M + 1, goals=None))
print(step(B=0), step(B=0, W=M, L=M, n=16, avoid=p, t=2 * M - 1), step(B=0, W=65, L=20, n=1, levels=8), need)
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1')
    out = subprocess.run([sys.executable, '-c', child, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == ['-1'] * (11 + 14), out.stdout
    assert lines[1].split() == ['-1'] * 6, out.stdout
    assert lines[2].split() == ['-6'] * 5, out.stdout
    assert lines[3].split() == ['0'] * 3 + [str(4 * (85 - 2 - 8) * 65 * 16)], out.stdout


def test_checked_library_and_follower_raise_the_documented_exceptions():
    import ctypes as C
    from marl_dmfb_amd.plan import MedaWideFollower, MedaWideFollowPlanner, MedaWidePlanner
    lib = _lib.checked('meda_follow_wide')
    host = C.create_string_buffer(64)
    p = C.addressof(host)
    with pytest.raises(NotImplementedError, match='MEDA_FOLLOW_WIDE_MAX_DIM'):
        lib.meda_follow_wide_step(1, 129, 30, 4, 0, *[p] * 15, None, 0, 0, None)
    with pytest.raises(NotImplementedError):
        lib.meda_follow_wide_step(1, 30, 30, 17, 0, *[p] * 15, None, 0, 0, None)
    with pytest.raises(ValueError):
        lib.meda_follow_wide_step(1, 30, 30, 4, 60, *[p] * 15, None, 0, 0, None)

    class TooWide:      # nothing of it but the sizes may be read: the limit is checked before the device is touched
        width, length = 129, 30

        def __getattr__(self, name):
            raise AssertionError('the follower read env.%s' % name)
    with pytest.raises(NotImplementedError, match='MEDA_FOLLOW_WIDE_MAX_DIM'):
        MedaWideFollower(TooWide())
    TooWide.width, TooWide.length = 30, 129
    with pytest.raises(NotImplementedError):
        MedaWideFollower(TooWide())
    with pytest.raises(ValueError, match='lds_levels'):
        MedaWideFollower(TooWide(), lds_levels=-1)
    # the open-loop class stays as it was; the closed loop is the subclass's
    assert not hasattr(MedaWidePlanner, 'follow') and callable(MedaWideFollowPlanner.follow)
    assert issubclass(MedaWideFollowPlanner, MedaWidePlanner)


# ---------------------------------------------------------------------------------------------------- the fixtures of the GPU file
@pytest.mark.parametrize('name', sorted(CASES))
def test_the_oracle_plays_every_followed_episode(name):
    c, s, g, health, uniforms = case(name)
    W, L = c['width'], c['length']
    res = reference(name)
    judge(res, W, L, s, g, health, uniforms)
    parking_never_takes_a_droplet_inside_its_disc(res, g)
    assert res.replans.dtype == np.int32 and res.lower_bound.dtype == np.int32 and res.steps.dtype == np.int64
    assert (res.replans[~res.gave_up | (res.steps > 0)] >= 1).all()
    assert (res.positions[np.arange(len(res)), np.minimum(res.steps, W + L)] == res.positions[:, -1]).all()
    assert max(W, L) > 64
    for axis in c['seam']:      # recorded centres beyond the seam: the second word of a row, the second row of a lane
        assert res.positions[..., axis].max() >= 64, (name, axis)


def test_every_branch_of_the_loop_is_taken_by_the_cases():
    """Counted on the reference, so that no later change of a seed or a case can empty a branch unnoticed."""
    seen = {}
    for name in sorted(CASES):
        c, s, g, health, uniforms = case(name)
        res = reference(name)
        seen[name] = (int(res.success.sum()), int((res.replans > 1).sum()), int(partial_plans(res, c['width'], c['length'], g).sum()),
                      int(res.gave_up.sum()), int((res.lower_bound < 0).sum()), int(res.steps.max()))
        print(name, 'success %d, replans > 1 %d, partial plans %d, gave up %d, a goal out of reach %d, steps up to %d, of %d'
              % (seen[name] + (len(res),)))
    for name, (success, replanned, partial, gave_up, unreachable, steps) in seen.items():
        assert success > 0 and replanned > 0, name
    total = lambda k: sum(v[k] for v in seen.values())
    assert total(0) > 0 and total(2) > 0 and total(3) > 0
    for name in ('20x100_4_min_health', '100x20_4_min_health'):      # blocked centres: parking has work to do, some chips are given up
        assert seen[name][3] > 0, name
    assert seen['20x100_4_min_health'][2] > 0 and seen['20x72_3_many'][2] > 0 and seen['20x72_3_many'][3] > 0
    # more chips than a launch has workgroups, and not a multiple of them
    B, groups = CASES['20x72_3_many']['B'], _lib.meda_follow_wide().meda_follow_wide_max_groups()
    assert 2 * groups < B < 3 * groups
