"""Host side of the wide MEDA planner (marl_dmfb_amd.plan.MedaWidePlanner, include/meda_plan_wide.h; chips up to 128 x 128): the
header against the binding table, the limits, the size queries, the argument guards without a GPU, and the task sets and hand
cases of tests/test_gpu_meda_plan_wide.py through plan_reference_meda and the CPU oracle.  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from marl_dmfb_amd import _lib
from meda_plan_helpers import MAX_UNROUTED, consistent, judge, no_conflict
from meda_plan_wide_helpers import (FORCED_LEVELS, LDS_BUDGET, REHOSTED, SEAM_LENGTHS, SEAM_WIDTHS, SERPENTINES, WIDE_SETS, lds_levels,
                                    many_tasks_case, reference, rehosted, seam_case, serpentine_case, set_case, walled_goal_80,
                                    workspace_case)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- C ABI
def test_meda_plan_wide_header_matches_the_binding_table():
    txt = open(os.path.join(ROOT, 'include', 'meda_plan_wide.h')).read()
    define = lambda name: int(re.search(r'#define MEDA_PLAN_WIDE_%s\s+(\d+)' % name, txt).group(1))
    limit, least, most, groups = define('MAX_DIM'), define('MIN_DIM'), define('MAX_AGENTS'), define('MAX_GROUPS')
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    txt = re.sub(r'^\s*#.*$', '', txt, flags=re.M)
    declared = {name: (0 if p.strip() in ('', 'void') else p.count(',') + 1)
                for name, p in re.findall(r'\b([a-z][a-z_0-9]*)\s*\(([^()]*)\)\s*;', txt)}
    assert declared == {'meda_plan_wide_route': 18, 'meda_plan_wide_max_dim': 0, 'meda_plan_wide_max_groups': 0,
                        'meda_plan_wide_lds_levels': 3, 'meda_plan_wide_lds_bytes': 4, 'meda_plan_wide_work_bytes': 5,
                        'meda_plan_wide_last_hip_error': 0}
    table = _lib.SIGNATURES['meda_plan_wide']
    assert sorted(table) == sorted(declared)
    raw = _lib.meda_plan_wide()
    for name, n in declared.items():
        sig = table[name]
        argtypes = sig[0] if isinstance(sig, tuple) else sig
        assert len(argtypes) == n and len(getattr(raw, name).argtypes) == n, name
    from marl_dmfb_amd import plan
    assert raw.meda_plan_wide_max_dim() == limit == 128 == plan.MEDA_WIDE_MAX_DIM and least == 5 and most == 16
    assert raw.meda_plan_wide_max_groups() == groups == 512
    assert plan.MEDA_MAX_DIM == 64                       # the narrow planner keeps its limit
    # the prefix table is matched in order: the wide library's functions must not fall to the narrow one's slot
    first = next(p for p in _lib._LAST_ERROR if 'meda_plan_wide_route'.startswith(p))
    assert _lib._LAST_ERROR[first] == 'meda_plan_wide_last_hip_error'
    first = next(p for p in _lib._LAST_ERROR if 'meda_plan_route'.startswith(p))
    assert _lib._LAST_ERROR[first] == 'meda_plan_last_hip_error'
    assert _lib.ENV_ERRORS['meda_plan_wide'][-1][0] is ValueError and _lib.ENV_ERRORS['meda_plan_wide'][-6][0] is NotImplementedError


def test_size_queries():
    raw = _lib.meda_plan_wide()
    groups = raw.meda_plan_wide_max_groups()
    paths = lambda w, l, n: ((w + l + 1) * n * 2 + 15) // 16 * 16
    shapes = ((128, 128, 16), (80, 80, 10), (65, 20, 1), (20, 65, 1), (5, 5, 1), (64, 64, 16), (30, 30, 4), (128, 5, 3), (100, 128, 7))
    for w, l, n in shapes:
        T = w + l
        H = min(T - 2, (LDS_BUDGET - paths(w, l, n) - 16 * w) // (16 * w))
        assert raw.meda_plan_wide_lds_levels(w, l, n) == H == lds_levels(w, l, n), (w, l, n)
        for cap in (0, -3, 1, 8, H, H + 1, 1000):
            h = min(H, cap) if cap > 0 else H
            assert raw.meda_plan_wide_lds_bytes(w, l, n, cap) == (h + 1) * w * 16 + paths(w, l, n), (w, l, n, cap)
            for B in (0, 1, 7, groups, groups + 3, 4096):
                assert raw.meda_plan_wide_work_bytes(B, w, l, n, cap) == min(B, groups) * (T - 2 - h) * w * 16, (w, l, n, cap, B)
    assert lds_levels(80, 80, 10) == 123 and lds_levels(128, 128, 16) == 74           # the figures of the header's arithmetic
    for w, l, n in ((128, 128, 16), (80, 80, 10), (65, 20, 1)):
        assert 0 < raw.meda_plan_wide_lds_bytes(w, l, n, 0) <= 160 * 1024 - 1024
    assert raw.meda_plan_wide_work_bytes(64, 65, 20, 1, 0) == 0
    assert raw.meda_plan_wide_work_bytes(64, 128, 128, 16, 0) > 0 and raw.meda_plan_wide_work_bytes(64, 65, 20, 1, 8) > 0
    for fn, more in ((raw.meda_plan_wide_lds_levels, ()), (raw.meda_plan_wide_lds_bytes, (0,))):
        assert fn(129, 30, 4, *more) == -6 and fn(30, 129, 4, *more) == -6 and fn(30, 30, 17, *more) == -6
        assert fn(4, 30, 4, *more) == -1 and fn(30, 4, 4, *more) == -1 and fn(30, 30, 0, *more) == -1
    assert raw.meda_plan_wide_work_bytes(4, 129, 30, 4, 0) == -6 and raw.meda_plan_wide_work_bytes(-1, 30, 30, 4, 0) == -1


def test_meda_plan_wide_argument_guards_need_no_gpu():
    """Dummy non-null pointers in a child process that sees no GPU: a launch there would come back as a HIP error (-100), never as
    -1, -6 or 0."""
    child = r'''
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from marl_dmfb_amd import _lib
lib = _lib.meda_plan_wide()
host = C.create_string_buffer(4096)
p = C.addressof(host) + 15 & ~15
def call(B=4, W=30, L=30, n=4, safe=0, s=p, g=p, avoid=None, route=p, u=p, steps=p, success=p, attempt=p, lower=p, work=None, wb=0,
         levels=0):
    return lib.meda_plan_wide_route(B, W, L, n, safe, s, g, avoid, route, u, steps, success, attempt, lower, work, wb, levels, None)
M = lib.meda_plan_wide_max_dim()
need = lib.meda_plan_wide_work_bytes(4, 65, 20, 1, 8)
print(call(B=-1), call(W=0), call(L=-3), call(W=4), call(L=4), call(n=0), call(s=None), call(g=None), call(route=None), call(u=None),
      call(steps=None), call(success=None), call(attempt=None), call(lower=None), call(safe=1, lower=None))
print(call(W=65, L=20, n=1, levels=8), call(W=65, L=20, n=1, levels=8, work=p, wb=need - 1), call(W=65, L=20, n=1, levels=8, wb=need),
      call(W=M, L=M, n=16), call(W=M, L=M, n=16, work=p, wb=4096), call(W=65, L=20, n=1, levels=8, work=p + 8, wb=need))
print(call(W=M + 1), call(L=M + 1), call(n=17), call(W=M + 1, L=M + 1, n=16), call(W=M + 1, s=None))
print(call(B=0), call(B=0, W=M, L=M, n=16, avoid=p), call(B=0, W=65, L=20, n=1, levels=8), call(B=0, safe=1), need)
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1')
    out = subprocess.run([sys.executable, '-c', child, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == ['-1'] * 15, out.stdout
    assert lines[1].split() == ['-1'] * 6, out.stdout
    assert lines[2].split() == ['-6'] * 5, out.stdout
    assert lines[3].split() == ['0'] * 4 + [str(4 * (85 - 2 - 8) * 65 * 16)], out.stdout


def test_checked_library_raises_the_documented_exceptions():
    import ctypes as C
    lib = _lib.checked('meda_plan_wide')
    host = C.create_string_buffer(64)
    p = C.addressof(host)
    with pytest.raises(NotImplementedError, match='MEDA_PLAN_WIDE_MAX_DIM'):
        lib.meda_plan_wide_route(1, 129, 30, 4, 0, p, p, None, p, p, p, p, p, p, None, 0, 0, None)
    with pytest.raises(NotImplementedError):
        lib.meda_plan_wide_route(1, 30, 30, 17, 1, p, p, None, p, p, p, p, p, p, None, 0, 0, None)
    with pytest.raises(ValueError):
        lib.meda_plan_wide_route(1, 30, 30, 4, 0, None, p, None, p, p, p, p, p, p, None, 0, 0, None)


# ---------------------------------------------------------------------------------------------------- the fixtures of the GPU file
@pytest.mark.parametrize('safe', [False, True], ids=['plain', 'safe'])
@pytest.mark.parametrize('name', sorted(WIDE_SETS))
def test_the_reference_routes_the_wide_sets_and_the_oracle_follows(name, safe):
    c = set_case(name)
    res = reference(name, c, safe)
    W, L, s, g = c['width'], c['length'], c['starts'], c['goals']
    print('%s %s: steps up to %d, steps / lower bound %.3f' % (name, 'safe' if safe else 'plain', res.steps.max(),
                                                                (res.steps / res.lower_bound).mean()))
    assert float((~res.success).mean()) <= MAX_UNROUTED
    assert res.success.all()                                  # nothing is left out on these sets
    assert (res.lower_bound >= 1).all() and (res.steps >= res.lower_bound).all() and (res.constraints == 0).all()
    assert judge(res, W, L, s, g) == len(res)
    for k in range(min(len(res), 4)):
        consistent(res, W, L, k)
        no_conflict(res, k)
    assert max(W, L) > 64


def test_seam_and_clamp_cases_take_the_steps_that_were_worked_out():
    for sizes, transposed in ((SEAM_LENGTHS, False), (SEAM_WIDTHS, True)):
        for size in sizes:
            c = seam_case(size, transposed)
            for safe in (False, True):
                res = reference(('seam', size, transposed), c, safe)
                assert res.success.all() and tuple(res.steps.tolist()) == c['steps'] == tuple(res.lower_bound.tolist()), (size, transposed)
            assert judge(res, c['width'], c['length'], c['starts'], c['goals']) == 3


def test_avoid_maps_beyond_row_and_column_63():
    c = walled_goal_80()
    for safe in (False, True):
        res = reference('walled_80', c, safe)
        assert not res.success[0] and res.lower_bound[0] == -1 and res.attempt[0] == -1 and res.steps[0] == 0
    routed = 0
    for axis in (0, 1):
        for name in REHOSTED:
            c = rehosted(name, axis)
            assert (c['starts'][..., axis] >= 66).all() and (c['goals'][..., axis] >= 66).all()
            res = reference(('rehosted', name, axis), c, False)
            routed += int(res.success.sum())
            if res.success.any():
                assert (res.positions[res.success][..., axis] >= 66).all()      # the whole route lies beyond the seam
                assert judge(res, c['width'], c['length'], c['starts'], c['goals']) == int(res.success.sum())
    assert routed > 50


@pytest.mark.parametrize('shape', SERPENTINES, ids=lambda s: '%dx%d' % s)
def test_every_arrival_level_exists_on_the_winding_corridor(shape):
    W, L = shape
    T = W + L
    c = serpentine_case(W, L)
    assert set(range(T - 1)) <= set(c['all_levels']) and max(c['all_levels']) > T - 2
    assert c['levels'][-3:] == (T - 3, T - 2, T - 1) and all({h - 1, h, h + 1} <= set(c['levels']) for h in FORCED_LEVELS)
    for safe in (False, True):
        res = reference(('serpentine', W, L), c, safe)
        want = [k + 1 for k in c['levels'][:-1]]
        assert res.success[:-1].all() and res.steps[:-1].tolist() == want == res.lower_bound[:-1].tolist()
        assert not res.success[-1] and res.lower_bound[-1] == -1 and res.steps[-1] == 0
    assert judge(res, W, L, c['starts'], c['goals']) == len(want)


def test_the_workspace_case_arrives_on_both_sides_of_the_lds_levels():
    c = workspace_case()
    H = lds_levels(128, 128, 2)
    for safe in (False, True):
        res = reference('workspace', c, safe)
        assert res.success.all() and tuple(res.steps.tolist()) == c['steps']
    assert min(c['steps']) - 1 < H < max(c['steps']) - 1 and 60 < H < 90
    assert judge(res, 128, 128, c['starts'], c['goals']) == 3


def test_more_tasks_than_workgroups_are_distinct_tasks():
    B = _lib.meda_plan_wide().meda_plan_wide_max_groups() + 3
    c = many_tasks_case(B)
    res = reference('many', c, False)
    assert len(res) == B and res.success.all()
    assert len({tuple(p) for p in c['starts'][:, 0].tolist()}) == B and len({tuple(p) for p in c['goals'][:, 0].tolist()}) == B
    assert len(set(res.steps.tolist())) > 10 and res.steps.max() - 1 > 8          # arrivals beyond the 8 levels kept in LDS
