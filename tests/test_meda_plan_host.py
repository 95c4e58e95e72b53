"""Host side of the MEDA space-time planner (marl_dmfb_amd.plan.plan_reference_meda): the CPU oracle as judge of every planned
route, hand cases of the rule, degraded electrodes, the C ABI of include/meda_plan.h and Router's `planner=` argument.  No GPU
needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from marl_dmfb_amd import _lib
from marl_dmfb_amd.plan import PlanResult, _meda_blocked, plan_reference_meda
from meda_plan_helpers import (DENSE, DENSER, MAX_UNROUTED, SETS, box_cells, consistent, dense_tasks, first_entry, hand_cases,
                               judge, no_conflict, oracle_tasks, serpentine)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(c):
    return plan_reference_meda(c['width'], c['length'], c['starts'], c['goals'], avoid=c['avoid'])


def _judged(res, width, length, s, g):
    """The oracle's verdict on a whole set, with the cap on what may be left out."""
    unrouted = float((~res.success).mean())
    ok = res.success & (res.lower_bound > 0)
    print('%dx%d / %d: %.4f of %d tasks unrouted, mean steps %.2f, steps / lower bound %.3f'
          % (width, length, s.shape[1], unrouted, len(res), res.steps[res.success].mean(),
             (res.steps[ok] / res.lower_bound[ok]).mean()))
    assert unrouted <= MAX_UNROUTED
    routed = res.success
    assert (res.lower_bound[routed] >= 1).all() and (res.steps[routed] >= res.lower_bound[routed]).all()
    assert (res.constraints == 0).all() and res.constraints.dtype == np.float64
    assert judge(res, width, length, s, g) == int(routed.sum())
    for k in np.nonzero(routed)[0][:16]:
        consistent(res, width, length, k)
        no_conflict(res, k)


# ---------------------------------------------------------------------------------------------------- the oracle as judge
@pytest.mark.parametrize('name', sorted(SETS))
def test_the_oracle_follows_every_planned_route(name):
    c = SETS[name]
    s, g = oracle_tasks(**c)
    _judged(plan_reference_meda(c['width'], c['length'], s, g), c['width'], c['length'], s, g)


def test_the_oracle_follows_the_routes_of_a_denser_set():
    """Starts 6 apart and goals 6 apart, where the env keeps 9: judged as the oracle sets if the reference stays within the cap
    (it leaves 0.8 % unrouted); 30x30 / 6, which the env refuses to build, is checked in numpy alone."""
    s, g = dense_tasks(**DENSE)
    res = plan_reference_meda(DENSE['width'], DENSE['length'], s, g)
    assert (res.attempt > 0).any()
    _judged(res, DENSE['width'], DENSE['length'], s, g)
    s, g = dense_tasks(**DENSER)
    res = plan_reference_meda(DENSER['width'], DENSER['length'], s, g)
    print('30x30 / 6: %.4f unrouted' % (~res.success).mean())
    assert res.success.mean() > 0.5
    for k in np.nonzero(res.success)[0]:
        consistent(res, 30, 30, k)
        no_conflict(res, k)


# ---------------------------------------------------------------------------------------------------- hand cases
def test_result_layout_of_a_single_droplet():
    res = plan_reference_meda(30, 30, np.array([[[5, 5]]]), np.array([[[20, 5]]]))
    # (5, 5) -E-> (8, 5) -> (11, 5) -> (14, 5) -> (17, 5): d2 to (20, 5) is 9 < 16, arrival 4, snapped by step 5
    assert res.success[0] and res.steps[0] == 5 and res.lower_bound[0] == 5 and res.attempt[0] == 0 and res.constraints[0] == 0
    assert res.actions[0, :, 0].tolist() == [1, 1, 1, 1, 8] + [-1] * 55
    assert res.positions[0, :6, 0].tolist() == [[5, 5], [8, 5], [11, 5], [14, 5], [17, 5], [20, 5]]
    assert (res.positions[0, 5:, 0] == [20, 5]).all()
    assert res.positions.shape == (1, 61, 1, 2) and res.positions.dtype == np.uint8 and res.actions.dtype == np.int8
    assert res.actions.shape == (1, 60, 1) and res.steps.dtype == np.int64 and res.success.dtype == bool
    assert res.attempt.dtype == np.int32 and res.lower_bound.dtype == np.int32 and res.constraints.dtype == np.float64
    assert isinstance(res, PlanResult)


def test_the_lowest_action_and_then_the_lowest_source_are_walked_back():
    # (10, 10) -> G of (15, 10) in one step by E (1), NE (4) or SE (5); the arrival cell is the lowest (y, x) of reach & G:
    # (12, 8), reached by NE alone
    res = plan_reference_meda(30, 30, np.array([[[10, 10]]]), np.array([[[15, 10]]]))
    assert res.steps[0] == 2 and res.actions[0, :2, 0].tolist() == [4, 8]
    assert res.positions[0, :3, 0].tolist() == [[10, 10], [12, 8], [15, 10]]


def test_corridor_swap_fails_without_a_bay_and_waits_with_one():
    cases = hand_cases()
    res = _case(cases['corridor_swap'])
    assert not res.success[0] and res.attempt[0] == -1 and res.steps[0] == 0 and res.lower_bound[0] == 9
    assert (res.actions == -1).all() and (res.positions[0] == cases['corridor_swap']['starts'][0]).all()
    c = cases['corridor_swap_bay']
    res = _case(c)
    assert res.success[0] and res.steps[0] > res.lower_bound[0] == 9
    assert judge(res, 30, 30, c['starts'], c['goals']) == 1
    consistent(res, 30, 30)
    no_conflict(res)
    blocked = _meda_blocked(30, 30, c['avoid'][0])
    p = res.positions[0].astype(int)
    assert not blocked[p[..., 1], p[..., 0]].any()


def test_two_droplets_share_the_ring_along_the_border():
    c = hand_cases()['ring_pair']
    res = _case(c)
    print('ring_pair: success %s steps %s lower bound %s attempt %s' % (res.success, res.steps, res.lower_bound, res.attempt))
    assert res.success.any()
    assert judge(res, 30, 30, c['starts'], c['goals']) == int(res.success.sum())
    for b in np.nonzero(res.success)[0]:
        consistent(res, 30, 30, b)
        no_conflict(res, b)


def test_a_start_inside_the_goal_disc_takes_one_step():
    c = hand_cases()['start_in_goal']
    res = _case(c)
    assert res.success[0] and res.steps[0] == 1 and res.lower_bound[0] == 1
    assert res.actions[0, 0].tolist() == [8, 8] and (res.actions[0, 1:] == -1).all()
    assert res.positions[0, 1].tolist() == [[12, 12], [20, 23]]
    assert judge(res, 30, 30, c['starts'], c['goals']) == 1


def test_goals_closer_than_6_fail_and_a_walled_goal_has_no_bound():
    cases = hand_cases()
    res = _case(cases['goals_closer_than_6'])
    assert not res.success[0] and res.attempt[0] == -1 and res.lower_bound[0] > 0
    res = _case(cases['goal_walled_off'])
    assert not res.success[0] and res.lower_bound[0] == -1 and res.attempt[0] == -1 and res.steps[0] == 0
    assert (res.actions == -1).all() and (res.positions[0] == cases['goal_walled_off']['starts'][0]).all()


@pytest.mark.parametrize('name', ['edges_and_corners', 'edges_64', 'ring', 'ring_64'])
def test_clamped_moves_at_every_edge_and_corner(name):
    c = hand_cases()[name]
    res = _case(c)
    assert res.success.all()
    np.testing.assert_array_equal(res.steps, res.lower_bound)
    assert judge(res, c['width'], c['length'], c['starts'], c['goals']) == len(res)
    clamped = 0
    hi = np.array([c['length'] - 3, c['width'] - 3])
    from meda_plan_helpers import DELTA
    for b in range(len(res)):
        consistent(res, c['width'], c['length'], b)
        # against the independent search: no route into the goal disc is shorter
        blocked = _meda_blocked(c['width'], c['length'], None if c['avoid'] is None else c['avoid'][b])
        assert res.steps[b] == first_entry(c['width'], c['length'], c['starts'][b, 0], c['goals'][b, 0], blocked) + 1
        for t in range(int(res.steps[b]) - 1):
            raw = res.positions[b, t, 0].astype(int) + DELTA[res.actions[b, t, 0]]
            clamped += bool(((raw < 2) | (raw > hi)).any())
    print('%s: %d clamped moves walked back' % (name, clamped))
    assert clamped > 0 or name == 'edges_64'
    # a droplet hugging an edge: every move out of the corner (2, 2) is clamped
    res = plan_reference_meda(30, 30, np.array([[[3, 3]]]), np.array([[[2, 9]]]))
    assert res.success[0] and judge(res, 30, 30, np.array([[[3, 3]]]), np.array([[[2, 9]]])) == 1


def test_steps_T_minus_1_are_accepted_and_a_longer_need_is_refused():
    """A corridor winding through a 40x40 chip (T = 80).  An independent search gives the first entry into the goal disc of
    goals along its end; an entry at T-2 is the last one the env can reward (success at step T-1 < max_step)."""
    W = L = 40
    T = W + L
    avoid, rows = serpentine(W, L)
    blocked = _meda_blocked(W, L, avoid)
    start = (2, 2)
    entry = {}
    for gy in range(rows[-1], W - 2):
        for gx in range(2, L - 2):
            e = first_entry(W, L, start, (gx, gy), blocked)
            entry.setdefault(e, (gx, gy))
    assert T - 2 in entry and T - 3 in entry, sorted(k for k in entry if k)
    late = [k for k in entry if k is not None and k > T - 2]
    goals = [entry[T - 3], entry[T - 2]] + [entry[k] for k in late[:1]]
    s = np.array([[start]] * len(goals))
    g = np.array([[q] for q in goals])
    res = plan_reference_meda(W, L, s, g, avoid=np.repeat(avoid[None], len(goals), 0))
    assert res.success[:2].all() and res.steps[:2].tolist() == [T - 2, T - 1] and res.lower_bound[:2].tolist() == [T - 2, T - 1]
    assert judge(res, W, L, s, g) == 2
    if late:
        assert not res.success[2] and res.lower_bound[2] == -1


def test_lower_bound_attempt_and_padding_wherever_routed():
    s, g = dense_tasks(**dict(DENSE, B=32, seed=11))
    res = plan_reference_meda(30, 60, s, g)
    T = 90
    for b in range(len(res)):
        if res.success[b]:
            assert 1 <= res.lower_bound[b] <= res.steps[b] <= T - 1 and 0 <= res.attempt[b] < 8
            st = int(res.steps[b])
            assert (res.actions[b, st:] == -1).all() and (res.actions[b, :st] >= 0).all()
            assert (res.positions[b, st:] == g[b]).all()
        else:
            assert res.attempt[b] == -1 and res.steps[b] == 0 and (res.actions[b] == -1).all()
            assert (res.positions[b] == s[b]).all()
    # alone, the lower bound is what the independent search finds
    blocked = _meda_blocked(30, 60, None)
    for b in range(8):
        want = max(first_entry(30, 60, s[b, i], g[b, i], blocked) for i in range(8)) + 1
        assert res.lower_bound[b] == want


def test_inputs_are_validated():
    with pytest.raises(ValueError, match='task 0: start'):
        plan_reference_meda(30, 30, np.array([[[1, 5]]]), np.array([[[20, 5]]]))
    with pytest.raises(ValueError, match='avoid must have shape'):
        plan_reference_meda(30, 30, np.array([[[5, 5]]]), np.array([[[20, 5]]]), avoid=np.zeros((1, 30, 29)))
    empty = plan_reference_meda(30, 30, np.zeros((0, 4, 2), int), np.zeros((0, 4, 2), int))
    assert len(empty) == 0 and empty.positions.shape == (0, 61, 4, 2) and empty.constraints.dtype == np.float64


# ---------------------------------------------------------------------------------------------------- health
def test_degraded_electrodes_are_avoided_and_the_plan_stays_exact():
    """No box a droplet moves from or arrives on covers a degraded cell, so every planned move has probability 1.0; the oracle
    replays the routes with move draws just below 1.  The one box that may cover such a cell is the goal's after the snap, which
    the env sets without a draw."""
    c = SETS['30x30_4']
    s, g = oracle_tasks(**c)
    B = len(s)
    rng = np.random.default_rng(5)
    health = np.where(rng.random((B, 30, 30)) < 0.01, rng.uniform(0.1, 0.9, (B, 30, 30)), 1.0)
    res = plan_reference_meda(30, 30, s, g, health=health)
    same = plan_reference_meda(30, 30, s, g, avoid=health < 1)
    np.testing.assert_array_equal(res.lower_bound, same.lower_bound)
    low = health < 1
    weak = np.array([box_cells(low[b], s[b]).any() for b in range(B)])
    assert weak.any() and not res.success[weak].any() and same.success[weak].any()
    assert (res.lower_bound[weak] == same.lower_bound[weak]).all() and (res.lower_bound[weak] > 0).any()
    for k in ('positions', 'actions', 'steps', 'success', 'attempt'):
        np.testing.assert_array_equal(getattr(res, k)[~weak], getattr(same, k)[~weak])
    ok = np.nonzero(res.success)[0]
    assert len(ok) > B // 4
    for b in ok:
        p = res.positions[b].astype(int)                                    # (T+1, n, 2)
        in_g = ((p - g[b]) ** 2).sum(axis=-1) < 16
        arrival = in_g.argmax(axis=0)                                       # per droplet: the first level inside its goal disc
        upto = np.arange(p.shape[0])[:, None] <= arrival[None]              # the start, every move and the arrival cell
        assert not (box_cells(low[b], p) & upto).any()
    assert judge(res, 30, 30, s, g, health=health, uniforms=0.999999) == len(ok)


# ---------------------------------------------------------------------------------------------------- C ABI
def test_meda_plan_header_matches_the_binding_table():
    txt = open(os.path.join(ROOT, 'include', 'meda_plan.h')).read()
    limit = int(re.search(r'#define MEDA_PLAN_MAX_DIM (\d+)', txt).group(1))
    most = int(re.search(r'#define MEDA_PLAN_MAX_AGENTS (\d+)', txt).group(1))
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    txt = re.sub(r'^\s*#.*$', '', txt, flags=re.M)
    declared = {name: (0 if p.strip() in ('', 'void') else p.count(',') + 1)
                for name, p in re.findall(r'\b([a-z][a-z_0-9]*)\s*\(([^()]*)\)\s*;', txt)}
    assert declared == {'meda_plan_route': 14, 'meda_plan_max_dim': 0, 'meda_plan_lds_bytes': 3, 'meda_plan_last_hip_error': 0}
    table = _lib.SIGNATURES['meda_plan']
    assert sorted(table) == sorted(declared)
    raw = _lib.meda_plan()
    for name, n in declared.items():
        sig = table[name]
        argtypes = sig[0] if isinstance(sig, tuple) else sig
        assert len(argtypes) == n and len(getattr(raw, name).argtypes) == n, name
    from marl_dmfb_amd import plan
    assert raw.meda_plan_max_dim() == limit == plan.MEDA_MAX_DIM and most == plan.MEDA_MAX_AGENTS == 16
    # blocked rows + (T - 2) src levels of `width` words, and the paths rounded up to 16 bytes; T = width + length
    formula = lambda w, l, n: (w + l - 1) * w * 8 + (((w + l + 1) * n * 2 + 15) // 16) * 16
    for w, l, n in ((30, 30, 4), (30, 60, 8), (60, 30, 8), (60, 60, 16), (45, 45, 9), (5, 5, 1), (64, 64, 16)):
        assert raw.meda_plan_lds_bytes(w, l, n) == formula(w, l, n), (w, l, n)
    assert raw.meda_plan_lds_bytes(30, 30, 4) == 14160 + 496
    assert 0 < raw.meda_plan_lds_bytes(limit, limit, most) <= 160 * 1024 - 1024
    assert raw.meda_plan_lds_bytes(limit + 1, 30, 4) == -6 and raw.meda_plan_lds_bytes(30, 30, most + 1) == -6
    assert raw.meda_plan_lds_bytes(4, 30, 4) == -1 and raw.meda_plan_lds_bytes(30, 30, 0) == -1
    assert any(p.startswith('meda_plan_') for p in _lib._LAST_ERROR) and 'meda_plan' in _lib.ENV_ERRORS


def test_meda_plan_argument_guards_need_no_gpu():
    """Dummy non-null pointers in a child process that sees no GPU: a launch there would come back as a HIP error (-100), never as
    -1, -6 or 0."""
    child = r'''
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from marl_dmfb_amd import _lib
lib = _lib.meda_plan()
host = C.create_string_buffer(4096)
p = C.addressof(host)
def call(B=4, W=30, L=30, n=4, s=p, g=p, avoid=None, route=p, u=p, steps=p, success=p, attempt=p, lower=p):
    return lib.meda_plan_route(B, W, L, n, s, g, avoid, route, u, steps, success, attempt, lower, None)
M = lib.meda_plan_max_dim()
print(call(B=-1), call(W=0), call(L=-3), call(W=4), call(n=0), call(s=None), call(g=None), call(route=None), call(u=None),
      call(steps=None), call(success=None), call(attempt=None), call(lower=None))
print(call(W=M + 1), call(L=M + 1), call(n=17), call(W=M + 1, L=M + 1, n=16))
print(call(B=0), call(B=0, W=M, L=M, n=16, avoid=p))
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1')
    out = subprocess.run([sys.executable, '-c', child, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == ['-1'] * 13, out.stdout
    assert lines[1].split() == ['-6'] * 4, out.stdout
    assert lines[2].split() == ['0'] * 2, out.stdout


def test_checked_library_raises_the_documented_exceptions():
    lib = _lib.checked('meda_plan')
    host = C.create_string_buffer(64)
    p = C.addressof(host)
    with pytest.raises(NotImplementedError):
        lib.meda_plan_route(1, 65, 30, 4, p, p, None, p, p, p, p, p, p, None)
    with pytest.raises(NotImplementedError):
        lib.meda_plan_route(1, 30, 30, 17, p, p, None, p, p, p, p, p, p, None)
    with pytest.raises(ValueError):
        lib.meda_plan_route(1, 30, 30, 4, None, p, None, p, p, p, p, p, p, None)


# ---------------------------------------------------------------------------------------------------- Router
class _FakePlanner:
    """plan_reference_meda behind the interface of MedaPlanner (no GPU here)."""

    def __init__(self, width, length, n_agents):
        self.width, self.length, self.n_agents, self.calls = width, length, n_agents, 0

    def plan(self, starts, goals, avoid=None, health=None):
        self.calls += 1
        return plan_reference_meda(self.width, self.length, starts, goals, avoid=avoid, health=health)


def test_router_checks_the_planner_before_any_launch():
    from marl_dmfb_amd.route import Router
    m = Router(None, name='meda', width=30, length=30, n_agents=4, fov=19, device='cpu')
    s, g = oracle_tasks(**dict(SETS['30x30_4'], B=4))
    for bad in (_FakePlanner(30, 60, 4), _FakePlanner(60, 30, 4), _FakePlanner(30, 30, 8)):
        with pytest.raises(ValueError, match='planner is for'):
            m.route(s, g, fallback='plan', planner=bad)
        with pytest.raises(ValueError, match='planner is for'):
            m.route(s, g, lower_bound=True, planner=bad)
        assert bad.calls == 0
    with pytest.raises(ValueError, match='plan'):
        m.route(s, g, fallback='plan', planner=object())
    with pytest.raises(ValueError, match='DMFB only'):
        m.route(s, g, fallback='plan')
    assert m.rounds == 0 and not m._slots
    empty = m.route(np.zeros((0, 4, 2), int), np.zeros((0, 4, 2), int), fallback='plan', planner=_FakePlanner(30, 30, 4))
    assert len(empty) == 0 and empty.lower_bound.shape == (0,) and empty.constraints.dtype == np.float64


def test_router_substitutes_only_the_failed_tasks_with_a_given_planner():
    """Router._plan with a result as a policy would leave it: every second task failed."""
    from marl_dmfb_amd.route import RouteResult, Router
    m = Router(None, name='meda', width=30, length=30, n_agents=4, fov=19, device='cpu')
    s, g = oracle_tasks(**dict(SETS['30x30_4'], B=16))
    T, B = 60, 16
    rng = np.random.default_rng(0)
    failed = np.arange(B) % 2 == 1

    def policy():
        return RouteResult(rng.integers(2, 27, (B, T + 1, 4, 2)).astype(np.uint8), rng.integers(0, 9, (B, T, 4)).astype(np.int8),
                           np.where(failed, T, 12).astype(np.int64), ~failed, np.where(failed, -1.2, 0.0),
                           np.arange(B, dtype=np.int32) % 3)
    rng = np.random.default_rng(0)
    before = policy()
    rng = np.random.default_rng(0)
    res = policy()
    fake = _FakePlanner(30, 30, 4)
    out = m._plan(res, s, g, None, None, True, fake)
    plan = plan_reference_meda(30, 30, s, g)
    assert out is res and fake.calls == 1 and plan.success.all()
    np.testing.assert_array_equal(res.source, failed.astype(np.int8))
    np.testing.assert_array_equal(res.lower_bound, plan.lower_bound)
    for k in ('positions', 'actions', 'steps', 'success', 'constraints'):
        np.testing.assert_array_equal(getattr(res, k)[failed], getattr(plan, k)[failed], err_msg=k)
        np.testing.assert_array_equal(getattr(res, k)[~failed], getattr(before, k)[~failed], err_msg=k)
        assert getattr(res, k).dtype == getattr(before, k).dtype
    assert (res.try_index[failed] == -1).all()
    np.testing.assert_array_equal(res.try_index[~failed], before.try_index[~failed])
    # the bound alone substitutes nothing
    rng = np.random.default_rng(0)
    res = m._plan(policy(), s, g, None, None, False, fake)
    for k in ('positions', 'actions', 'steps', 'success', 'constraints', 'try_index'):
        np.testing.assert_array_equal(getattr(res, k), getattr(before, k), err_msg=k)
    assert (res.source == 0).all()
    np.testing.assert_array_equal(res.lower_bound, plan.lower_bound)
