"""Host side of the two opt-in parameters of the DMFB planning rule (marl_dmfb_amd.plan: `reserve`, `retries`; DESIGN.md section
10): the defaults change nothing, the tasks the default rule cannot route under any order route with reservations, the routed
counts of the rule in numpy, the CPU oracle as judge of every routed task, the retries' attempt numbers and the guards of the two
new entry points of include/route_plan.h.  No GPU needed."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from marl_dmfb_amd.plan import follow_reference, plan_reference

import follow_helpers
from plan_helpers import SETS, equal, judge, oracle_tasks
from plan_reserve_helpers import CORNERED_GOALS, CORNERED_STARTS, CORNERED_STEPS, RETRY_GOALS, RETRY_STARTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (chip, reserve, retries) -> tasks routed, of oracle_tasks(width, length, n, seed=3, B)
COUNTED = {'10x10_4': dict(width=10, length=10, n_agents=4, seed=3, B=1024), '20x20_10': dict(width=20, length=20, n_agents=10, seed=3, B=256)}
ROUTED = {('10x10_4', 0, 0): 955, ('10x10_4', 1, 0): 1023, ('10x10_4', 2, 0): 1024,
          ('20x20_10', 0, 0): 217, ('20x20_10', 1, 0): 255, ('20x20_10', 1, 10): 256}


@functools.lru_cache(maxsize=None)
def counted(name, reserve, retries):
    """(tasks, plan_reference of them), computed once per process."""
    c = COUNTED[name]
    s, g, _ = oracle_tasks(**c)
    return (s, g), plan_reference(c['width'], c['length'], s, g, reserve=reserve, retries=retries)


@functools.lru_cache(maxsize=None)
def degraded(reserve):
    """The follower case of the issue: 10x10 / 4 with 2 blocks, 256 chips, health 0.6 .. 1.0."""
    s, g, b = oracle_tasks(10, 10, 4, 2, seed=5, B=256)
    rng = np.random.default_rng(7)
    health = 0.6 + 0.4 * rng.random((256, 10, 10))
    u = rng.random((40, 256, 4))
    return (s, g, b, health, u), follow_reference(10, 10, s, g, blocks=b, health=health, uniforms=u, reserve=reserve)


# ---------------------------------------------------------------------------------------------------- the defaults
@pytest.mark.parametrize('name', sorted(SETS))
def test_plan_reference_with_zero_reserve_and_retries_is_the_default_rule(name):
    c = SETS[name]
    s, g, b = oracle_tasks(**c)
    want = plan_reference(c['width'], c['length'], s, g, blocks=b)
    equal(plan_reference(c['width'], c['length'], s, g, blocks=b, reserve=0, retries=0), want)
    assert want.attempt.max() < c['n_agents']


@pytest.mark.parametrize('name', sorted(follow_helpers.CASES))
def test_follow_reference_with_zero_reserve_and_retries_is_the_default_rule(name):
    c, s, g, b, health, uniforms = follow_helpers.case(name)
    want = follow_helpers.reference(name)
    B = c['B']
    # distinct tasks (chips are independent of each other), fewer of the costly ones
    idx = np.arange(0, B, B // c.get('unique', B))[:24 if c['n_agents'] <= 5 else 6]
    sub = lambda a, axis=0: None if a is None else np.take(a, idx, axis=axis)
    got = follow_reference(c['width'], c['length'], sub(s), sub(g), blocks=sub(b), health=sub(health),
                           min_health=c.get('min_health', 0.0), uniforms=sub(uniforms, 1), reserve=0, retries=0)
    for k in follow_helpers.FIELDS:
        np.testing.assert_array_equal(getattr(got, k), getattr(want, k)[idx], err_msg=k)


def test_the_parameters_are_checked():
    for kw in (dict(reserve=-1), dict(retries=-1), dict(reserve=256), dict(retries=256)):
        with pytest.raises(ValueError, match='0 .. 255'):
            plan_reference(10, 10, CORNERED_STARTS, CORNERED_GOALS, **kw)
        with pytest.raises(ValueError, match='0 .. 255'):
            follow_reference(10, 10, CORNERED_STARTS, CORNERED_GOALS, **kw)


# ---------------------------------------------------------------------------------------------------- reservations
def test_cornered_tasks_fail_today_and_route_with_one_reserved_level():
    today = plan_reference(10, 10, CORNERED_STARTS, CORNERED_GOALS)
    assert today.attempt.tolist() == [-1, -1, -1] and not today.success.any()
    res = plan_reference(10, 10, CORNERED_STARTS, CORNERED_GOALS, reserve=1)
    assert res.success.all() and res.attempt.tolist() == [0, 0, 0]
    assert res.steps.tolist() == CORNERED_STEPS
    np.testing.assert_array_equal(res.lower_bound, today.lower_bound)      # the bound is that of the droplets alone
    assert judge(res, 10, 10, CORNERED_STARTS, CORNERED_GOALS, None, True) == 3


@pytest.mark.parametrize('name,reserve,retries', sorted(ROUTED))
def test_routed_counts_and_the_oracle_finds_no_conflict(name, reserve, retries):
    c = COUNTED[name]
    (s, g), res = counted(name, reserve, retries)
    assert int(res.success.sum()) == ROUTED[name, reserve, retries]
    np.testing.assert_array_equal(res.attempt >= 0, res.success)
    assert res.attempt.max() < c['n_agents'] + retries
    assert (res.steps[res.success] >= res.lower_bound[res.success]).all()
    np.testing.assert_array_equal(res.lower_bound, counted(name, 0, 0)[1].lower_bound)
    assert judge(res, c['width'], c['length'], s, g, None, True) == ROUTED[name, reserve, retries]


def test_reservations_only_add_routed_tasks_here():
    """Not a law of the rule (a reservation can also close the one path an order had), but what these sets show: every task the
    default rule routes is still routed."""
    for name in COUNTED:
        assert not (counted(name, 0, 0)[1].success & ~counted(name, 1, 0)[1].success).any()


def test_the_follower_with_reservations_abandons_at_most_one_chip():
    (s, g, b, health, u), today = degraded(0)
    _, res = degraded(1)
    assert today.constraints.sum() == 0 and int(today.gave_up.sum()) == 12 and int(today.success.sum()) == 242
    assert res.constraints.sum() == 0
    assert int(res.gave_up.sum()) <= 1
    assert int(res.success.sum()) == 253
    follow_helpers.judge(res, 10, 10, s, g, b, health, u)


# ---------------------------------------------------------------------------------------------------- retries
def test_a_task_routed_only_by_a_retry_reports_its_attempt():
    n = RETRY_STARTS.shape[1]
    assert plan_reference(20, 20, RETRY_STARTS, RETRY_GOALS).attempt.tolist() == [-1]
    assert plan_reference(20, 20, RETRY_STARTS, RETRY_GOALS, retries=1).attempt.tolist() == [-1]
    res = plan_reference(20, 20, RETRY_STARTS, RETRY_GOALS, retries=10)
    assert res.success.all() and res.attempt.tolist() == [n + 1] and res.steps.tolist() == [18]
    equal(plan_reference(20, 20, RETRY_STARTS, RETRY_GOALS, retries=2), res)      # the retries after the kept one are never made
    assert judge(res, 20, 20, RETRY_STARTS, RETRY_GOALS, None, True) == 1


def test_retries_come_after_the_rotations():
    """A task that a rotation routes keeps that rotation, whatever `retries` is."""
    (s, g), want = counted('20x20_10', 1, 0)
    _, got = counted('20x20_10', 1, 10)
    ok = want.success
    for k in ('positions', 'actions', 'steps', 'attempt'):
        np.testing.assert_array_equal(getattr(got, k)[ok], getattr(want, k)[ok], err_msg=k)
    assert (got.attempt[~ok] >= 10).all()


# ---------------------------------------------------------------------------------------------------- C ABI
def test_the_opt_entry_points_guard_reserve_and_retries_without_a_gpu():
    """Dummy non-null pointers in a child process that sees no GPU: a launch there would come back as a HIP error (-100), never as
    -1 or 0."""
    child = r'''
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from marl_dmfb_amd import _lib
lib = _lib.route_plan()
host = C.create_string_buffer(4096)
p = C.addressof(host)
def plan(B=4, W=10, L=10, n=4, reserve=0, retries=0):
    return lib.route_plan_dmfb_opt(B, W, L, n, 0, p, p, None, None, p, p, p, p, p, p, reserve, retries, None)
def follow(B=4, W=10, L=10, n=4, t=0, reserve=0, retries=0):
    return lib.route_follow_dmfb_opt(B, W, L, n, 0, t, p, None, None, *[p] * 12, reserve, retries, None)
for f in (plan, follow):
    print(f(reserve=-1), f(retries=-1), f(reserve=256), f(retries=256), f(reserve=-1, retries=-1), f(B=0, reserve=256),
          f(B=0, retries=-2), f(n=0, reserve=1), f(B=-1, reserve=1, retries=1))
    print(f(W=65, reserve=1, retries=1))
    print(f(B=0), f(B=0, reserve=255, retries=255), f(B=0, reserve=1), f(B=0, retries=4))
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1')
    out = subprocess.run([sys.executable, '-c', child, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == 6, out.stdout
    for k in (0, 3):
        assert lines[k].split() == ['-1'] * 9, out.stdout
        assert lines[k + 1].split() == ['-6'], out.stdout
        assert lines[k + 2].split() == ['0'] * 4, out.stdout


def test_the_device_classes_check_the_parameters_before_any_launch():
    from marl_dmfb_amd import plan
    for kw in (dict(reserve=-1), dict(retries=256)):
        with pytest.raises(ValueError, match='0 .. 255'):
            plan.Planner(10, 10, 4, device='cpu', **kw)
    p = plan.Planner(10, 10, 4, device='cpu', reserve=1, retries=4)
    assert (p.reserve, p.retries) == (1, 4)
    assert (plan.Planner(10, 10, 4, device='cpu').reserve, plan.Planner(10, 10, 4, device='cpu').retries) == (0, 0)


# ---------------------------------------------------------------------------------------------------- CLIs
def test_the_clis_take_reserve_and_retries(tmp_path, monkeypatch):
    """--planner only with --reserve 1 routes the cornered tasks (the planner stubbed by plan_reference: no GPU here)."""
    from marl_dmfb_amd import evaluate, plan
    from marl_dmfb_amd.common.arguments import get_evaluate_args, get_route_args
    a = get_route_args(['dmfb'])
    assert (a.reserve, a.retries) == (0, 0)
    a = get_evaluate_args(['dmfb', '--router', 'follow', '--reserve', '2', '--retries', '3'])
    assert (a.reserve, a.retries) == (2, 3)
    assert (get_evaluate_args(['dmfb']).reserve, get_evaluate_args(['dmfb']).retries) == (0, 0)
    np.savez(tmp_path / 'tasks.npz', starts=CORNERED_STARTS, goals=CORNERED_GOALS)
    made = []

    class FakePlanner:
        def __init__(self, width, length, n_agents, device=None, **rule):
            self.w, self.l, self.rule = width, length, rule
            made.append(rule)

        def plan(self, starts, goals, blocks=None, avoid=None, health=None):
            return plan_reference(self.w, self.l, starts, goals, blocks=blocks, avoid=avoid, health=health, **self.rule)

    monkeypatch.setattr(plan, 'Planner', FakePlanner)
    out = tmp_path / 'routes.npz'
    for flags, routed in (([], [0, 0, 0]), (['--reserve', '1', '--retries', '2'], [1, 1, 1])):
        evaluate.main(['dmfb', '--chip_size', '10', '--tasks', str(tmp_path / 'tasks.npz'), '--routes', str(out), '--planner', 'only']
                      + flags)
        with np.load(out) as f:
            assert f['source'].tolist() == routed and f['success'].tolist() == [bool(v) for v in routed]
    assert made == [{}, {'reserve': 1, 'retries': 2}]
