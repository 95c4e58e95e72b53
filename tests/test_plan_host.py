"""Host side of the space-time planner (marl_dmfb_amd.plan): hand cases of the rule in numpy, the CPU oracle as judge of every
planned route, degraded electrodes, the C ABI of include/route_plan.h and Router's argument checks.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from marl_dmfb_amd import _lib
from marl_dmfb_amd.plan import plan_reference
from plan_helpers import MAX_UNROUTED, SETS, judge, oracle_tasks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = np.array([(0, 0), (1, 0), (-1, 0), (0, -1), (0, 1)])


def _one(width, length, starts, goals, **kw):
    return plan_reference(width, length, np.array([starts]), np.array([goals]), **kw)


def _consistent(res, b=0):
    """positions follow from the actions; STALL after arrival, -1 from `steps` on; the last position repeated."""
    steps = int(res.steps[b])
    pos, act = res.positions[b].astype(int), res.actions[b]
    assert (act[:steps] >= 0).all() and (act[steps:] == -1).all()
    np.testing.assert_array_equal(pos[1:steps + 1], pos[:steps] + DELTA[act[:steps]])
    assert (pos[steps:] == pos[steps]).all()


def _no_conflict(res, b=0):
    """No pair within Chebyshev distance 1 at the same step (static) nor new-against-old across a step (dynamic)."""
    pos = res.positions[b].astype(int)
    n = pos.shape[1]
    for i in range(n):
        for j in range(n):
            if i != j:
                assert (np.abs(pos[:, i] - pos[:, j]).max(axis=1) >= 2).all()
                assert (np.abs(pos[1:, i] - pos[:-1, j]).max(axis=1) >= 2).all()


# ---------------------------------------------------------------------------------------------------- hand cases
def test_one_droplet_takes_the_manhattan_path_with_the_lowest_action_walked_back():
    res = _one(10, 10, [[0, 0]], [[3, 2]])
    assert res.success[0] and res.steps[0] == 5 and res.lower_bound[0] == 5 and res.attempt[0] == 0 and res.constraints[0] == 0
    # walked back from the goal the lowest action number wins: RIGHT (1) before UP (4), so the route ends with its RIGHT moves
    assert res.actions[0, :, 0].tolist() == [4, 4, 1, 1, 1] + [-1] * 35
    assert res.positions[0, :6, 0].tolist() == [[0, 0], [0, 1], [0, 2], [1, 2], [2, 2], [3, 2]]
    assert res.positions.shape == (1, 41, 1, 2) and res.positions.dtype == np.uint8 and res.actions.dtype == np.int8
    assert res.steps.dtype == np.int64 and res.attempt.dtype == np.int32 and res.lower_bound.dtype == np.int32
    _consistent(res)
    left_down = _one(10, 10, [[5, 5]], [[3, 4]])
    assert left_down.actions[0, :3, 0].tolist() == [3, 2, 2]


def test_a_block_across_the_straight_line_forces_the_detour():
    # a wall x = 4, y = 0 .. 6 between (1, 2) and (8, 2): up to y = 7, across, and down again: 7 + 2 * 5 = 17 steps
    res = _one(10, 10, [[1, 2]], [[8, 2]], blocks=np.array([[[4, 4, 0, 6]]]))
    assert res.success[0] and res.steps[0] == 17 and res.lower_bound[0] == 17
    pos = res.positions[0, :, 0].astype(int)
    assert not ((pos[:, 0] == 4) & (pos[:, 1] <= 6)).any()
    _consistent(res)
    free = _one(10, 10, [[1, 2]], [[8, 2]])
    assert free.steps[0] == 7 and free.actions[0, :7, 0].tolist() == [1] * 7


def test_head_on_in_a_corridor_one_waits_or_the_task_fails_never_a_conflict():
    # the corridor y = 2 between two blocks, 10 cells long, droplets at its ends heading for each other's end: no way past
    walls = np.array([[[0, 9, 0, 1], [0, 9, 3, 9]]])
    res = _one(10, 10, [[0, 2], [9, 2]], [[9, 2], [0, 2]], blocks=walls)
    assert not res.success[0] and res.attempt[0] == -1 and res.steps[0] == 0 and res.lower_bound[0] == 9
    assert (res.actions == -1).all() and (res.positions[0] == np.array([[0, 2], [9, 2]])).all()
    # with a bay at (5, 3) one droplet can step aside and wait: routed, later than the lower bound, and never a conflict
    bay = np.array([[[0, 9, 0, 1], [0, 4, 3, 9], [6, 9, 3, 9], [5, 5, 5, 9]]])
    res = _one(10, 10, [[0, 2], [9, 2]], [[9, 2], [0, 2]], blocks=bay)
    if res.success[0]:
        assert res.steps[0] > res.lower_bound[0] == 9
        _consistent(res)
        _no_conflict(res)
    # two droplets that pass each other on an open chip
    res = _one(10, 10, [[0, 4], [9, 4]], [[9, 4], [0, 4]])
    assert res.success[0] and res.steps[0] >= res.lower_bound[0] == 9
    _consistent(res)
    _no_conflict(res)


def test_an_enclosed_goal_fails_with_lower_bound_minus_one():
    ring = np.array([[[4, 6, 4, 4], [4, 6, 6, 6], [4, 4, 5, 5], [6, 6, 5, 5]]])
    res = _one(10, 10, [[0, 0], [9, 9]], [[5, 5], [0, 9]], blocks=ring)
    assert not res.success[0] and res.lower_bound[0] == -1 and res.attempt[0] == -1 and res.steps[0] == 0
    assert (res.actions == -1).all() and (res.positions[0] == np.array([[0, 0], [9, 9]])).all()
    # the same through an avoid mask
    avoid = np.zeros((1, 10, 10), bool)
    avoid[0, 4:7, 4:7] = True
    avoid[0, 5, 5] = False
    res = _one(10, 10, [[0, 0], [9, 9]], [[5, 5], [0, 9]], avoid=avoid)
    assert not res.success[0] and res.lower_bound[0] == -1


def test_a_droplet_that_starts_on_its_goal_stays_there():
    res = _one(10, 10, [[2, 2], [7, 7]], [[2, 2], [7, 2]])
    assert res.success[0] and res.steps[0] == 5 and res.lower_bound[0] == 5
    assert (res.positions[0, :, 0] == [2, 2]).all() and res.actions[0, :5, 0].tolist() == [0] * 5
    assert res.actions[0, :5, 1].tolist() == [3] * 5
    alone = _one(10, 10, [[2, 2]], [[2, 2]])
    assert alone.success[0] and alone.steps[0] == 0 and alone.lower_bound[0] == 0 and (alone.actions == -1).all()
    # another droplet has to pass the parked one at a distance
    res = _one(10, 10, [[4, 4], [0, 4]], [[4, 4], [9, 4]])
    assert res.success[0] and res.steps[0] > 9
    _no_conflict(res)


def test_priority_order_and_rotation():
    # the farthest droplet is planned first and gets its shortest path; ties go to the lower index
    res = _one(12, 12, [[0, 0], [11, 0], [5, 11]], [[0, 3], [0, 11], [5, 2]])
    assert res.success[0] and res.attempt[0] == 0
    assert np.abs(np.diff(res.positions[0, :23, 1].astype(int), axis=0)).sum() == 22    # |11| + |11|: no detour, no wait


def test_inputs_are_validated():
    with pytest.raises(ValueError, match='task 0: start'):
        _one(10, 10, [[10, 0]], [[3, 2]])
    with pytest.raises(ValueError, match='avoid must have shape'):
        _one(10, 10, [[1, 0]], [[3, 2]], avoid=np.zeros((1, 10, 9)))
    empty = plan_reference(10, 10, np.zeros((0, 4, 2), int), np.zeros((0, 4, 2), int))
    assert len(empty) == 0 and empty.positions.shape == (0, 41, 4, 2)


# ---------------------------------------------------------------------------------------------------- the oracle as judge
@pytest.mark.parametrize('name', sorted(SETS))
def test_the_oracle_follows_every_planned_route(name):
    c = SETS[name]
    s, g, b = oracle_tasks(**c)
    res = plan_reference(c['width'], c['length'], s, g, blocks=b)
    unrouted = float((~res.success).mean())
    print('%s: %.4f of %d tasks unrouted' % (name, unrouted, len(res)))
    assert unrouted <= MAX_UNROUTED
    routed = res.success
    assert (res.steps[routed] >= res.lower_bound[routed]).all() and (res.lower_bound[routed] >= 0).all()
    assert (res.constraints == 0).all()
    for stall in (True, False):
        assert judge(res, c['width'], c['length'], s, g, b, stall) == int(routed.sum())
    for k in np.nonzero(routed)[0][:32]:
        _consistent(res, k)
        _no_conflict(res, k)


def test_degraded_electrodes_are_avoided_and_the_plan_stays_exact():
    c = SETS['10x10_4_2b']
    s, g, b = oracle_tasks(**c)
    rng = np.random.default_rng(5)
    B = len(s)
    health = np.where(rng.random((B, 10, 10)) < 0.08, rng.uniform(0.1, 0.9, (B, 10, 10)), 1.0)
    res = plan_reference(10, 10, s, g, blocks=b, health=health)
    same = plan_reference(10, 10, s, g, blocks=b, avoid=health < 1)
    np.testing.assert_array_equal(res.lower_bound, same.lower_bound)
    # a move succeeds with the health of the electrode the droplet stands on: a start on a degraded one is refused
    weak_start = (health[np.arange(B)[:, None], s[..., 0], s[..., 1]] < 1).any(axis=1)
    assert weak_start.any() and not res.success[weak_start].any() and same.success[weak_start].any()
    np.testing.assert_array_equal(res.success[~weak_start], same.success[~weak_start])
    ok = np.nonzero(res.success)[0]
    assert len(ok) > B // 4
    p = res.positions[ok].astype(int)
    assert not (health < 1)[ok[:, None, None], p[..., 0], p[..., 1]].any()   # no planned position on a degraded electrode
    # adversarial move draws: a droplet on an electrode of health h moves iff the draw is <= h
    assert judge(res, 10, 10, s, g, b, True, health=health, uniforms=0.999999) == len(ok)


# ---------------------------------------------------------------------------------------------------- C ABI
def test_route_plan_header_matches_the_binding_table():
    txt = open(os.path.join(ROOT, 'include', 'route_plan.h')).read()
    limit = int(re.search(r'#define ROUTE_PLAN_MAX_DIM (\d+)', txt).group(1))
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    txt = re.sub(r'^\s*#.*$', '', txt, flags=re.M)
    declared = {name: (0 if p.strip() in ('', 'void') else p.count(',') + 1)
                for name, p in re.findall(r'\b([a-z][a-z_0-9]*)\s*\(([^()]*)\)\s*;', txt)}
    assert declared['route_plan_dmfb'] == 16
    table = _lib.SIGNATURES['route_plan']
    assert sorted(table) == sorted(declared)
    raw = _lib.route_plan()
    for name, n in declared.items():
        sig = table[name]
        argtypes = sig[0] if isinstance(sig, tuple) else sig
        assert len(argtypes) == n and len(getattr(raw, name).argtypes) == n, name
    from marl_dmfb_amd import plan
    assert raw.route_plan_max_dim() == limit == plan.MAX_DIM
    # everything of a task lives in LDS: the largest chip with the most droplets fits the 160 KiB of a workgroup
    assert 0 < raw.route_plan_lds_bytes(limit, limit, plan.MAX_AGENTS) <= 160 * 1024 - 1024
    assert raw.route_plan_lds_bytes(50, 50, 10) == 199 * 50 * 8 + 4032
    assert raw.route_plan_lds_bytes(limit + 1, 10, 4) == -6 and raw.route_plan_lds_bytes(10, 10, 17) == -1


def test_route_plan_argument_guards_need_no_gpu():
    """Dummy non-null pointers in a child process that sees no GPU: a launch there would come back as a HIP error (-100), never as
    -1, -6 or 0."""
    child = r'''
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from marl_dmfb_amd import _lib
lib = _lib.route_plan()
host = C.create_string_buffer(4096)
p = C.addressof(host)
def call(B=4, W=10, L=10, n=4, nb=0, s=p, g=p, blocks=None, avoid=None, route=p, u=p, steps=p, success=p, attempt=p, lower=p):
    return lib.route_plan_dmfb(B, W, L, n, nb, s, g, blocks, avoid, route, u, steps, success, attempt, lower, None)
M = lib.route_plan_max_dim()
print(call(B=-1), call(W=0), call(L=-3), call(n=0), call(n=17), call(nb=-1), call(nb=2), call(s=None), call(g=None),
      call(route=None), call(u=None), call(steps=None), call(success=None), call(attempt=None), call(lower=None))
print(call(W=M + 1), call(L=M + 1), call(W=M + 1, L=M + 1, n=16))
print(call(B=0), call(B=0, W=M, L=M, n=16, nb=3, blocks=p, avoid=p))
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1')
    out = subprocess.run([sys.executable, '-c', child, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == ['-1'] * 15, out.stdout
    assert lines[1].split() == ['-6'] * 3, out.stdout
    assert lines[2].split() == ['0'] * 2, out.stdout


def test_checked_library_raises_the_documented_exceptions():
    lib = _lib.checked('route_plan')
    host = C.create_string_buffer(64)
    p = C.addressof(host)
    with pytest.raises(NotImplementedError):
        lib.route_plan_dmfb(1, 65, 10, 4, 0, p, p, None, None, p, p, p, p, p, p, None)
    with pytest.raises(ValueError):
        lib.route_plan_dmfb(1, 10, 10, 17, 0, p, p, None, None, p, p, p, p, p, p, None)


# ---------------------------------------------------------------------------------------------------- Router and CLI
def test_router_checks_the_fallback_before_any_launch():
    from marl_dmfb_amd.route import Router
    s = np.array([[[0, 0], [5, 5], [9, 9], [0, 9]]])
    g = np.array([[[9, 0], [2, 7], [4, 4], [8, 8]]])
    r = Router(agents=None, name='dmfb', width=10, length=10, n_agents=4, fov=9, device='cpu')
    with pytest.raises(ValueError, match='fallback'):
        r.route(s, g, fallback='astar')
    m = Router(None, name='meda', width=30, length=30, n_agents=4, fov=19, device='cpu')
    ms, mg = np.array([[[2, 2], [27, 27], [2, 27], [27, 2]]]), np.array([[[15, 15], [10, 20], [20, 10], [5, 5]]])
    with pytest.raises(ValueError, match='DMFB only'):
        m.route(ms, mg, fallback='plan')
    with pytest.raises(ValueError, match='DMFB only'):
        m.route(ms, mg, lower_bound=True)
    assert r.rounds == 0 and not r._slots and m.rounds == 0 and not m._slots
    empty = r.route(np.zeros((0, 4, 2), int), np.zeros((0, 4, 2), int), fallback='plan')
    assert len(empty) == 0 and empty.source.shape == (0,) and empty.source.dtype == np.int8 and empty.lower_bound.shape == (0,)
    assert r.route(np.zeros((0, 4, 2), int), np.zeros((0, 4, 2), int)).lower_bound is None


def test_route_result_keeps_its_six_argument_form():
    from marl_dmfb_amd.route import RouteResult
    res = RouteResult(np.zeros((3, 41, 4, 2), np.uint8), np.zeros((3, 40, 4), np.int8), np.array([5, 40, 7]),
                      np.array([True, False, True]), np.zeros(3, np.int64), np.zeros(3, np.int32))
    assert res.source.tolist() == [0, 0, 0] and res.source.dtype == np.int8 and res.lower_bound is None


def test_evaluate_cli_planner_flag(tmp_path, monkeypatch):
    """--planner only needs no model and saves source and lower_bound (the planner stubbed by plan_reference: no GPU here)."""
    from marl_dmfb_amd import evaluate, plan
    from marl_dmfb_amd.common.arguments import get_route_args
    assert get_route_args(['dmfb']).planner == 'off'
    assert get_route_args(['dmfb', '--planner', 'fallback']).planner == 'fallback'
    with pytest.raises(SystemExit):
        get_route_args(['dmfb', '--planner', 'astar'])
    s, g, b = oracle_tasks(B=16, **SETS['10x10_4_2b'])
    np.savez(tmp_path / 'tasks.npz', starts=s, goals=g, blocks=b)

    class FakePlanner:
        def __init__(self, width, length, n_agents, device=None):
            self.w, self.l = width, length

        def plan(self, starts, goals, blocks=None, avoid=None, health=None):
            return plan_reference(self.w, self.l, starts, goals, blocks=blocks, avoid=avoid, health=health)

    monkeypatch.setattr(plan, 'Planner', FakePlanner)
    monkeypatch.setattr(evaluate, '_make_env', lambda *a, **k: pytest.fail('--planner only builds no env'))
    out = tmp_path / 'routes.npz'
    evaluate.main(['dmfb', '--chip_size', '10', '--block_num', '2', '--tasks', str(tmp_path / 'tasks.npz'), '--routes', str(out),
                   '--planner', 'only'])
    want = plan_reference(10, 10, s, g, blocks=b)
    with np.load(out) as f:
        assert sorted(f.files) == sorted(['positions', 'actions', 'steps', 'success', 'constraints', 'try_index', 'starts',
                                          'goals', 'blocks', 'cfg', 'source', 'lower_bound'])
        np.testing.assert_array_equal(f['positions'], want.positions)
        np.testing.assert_array_equal(f['lower_bound'], want.lower_bound)
        np.testing.assert_array_equal(f['source'], want.success.astype(np.int8))
        assert (f['try_index'] == -1).all()
    with pytest.raises(ValueError, match='DMFB only'):
        evaluate.main(['meda', '--tasks', str(tmp_path / 'tasks.npz'), '--planner', 'only'])
