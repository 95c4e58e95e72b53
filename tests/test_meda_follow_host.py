"""Host side of closed-loop planner routing for MEDA: the failure-safe rule (marl_dmfb_amd.plan.plan_reference_meda(safe=True))
with the CPU oracle as judge and its safety property in numpy, the closed loop (follow_reference_meda) judged by the oracle on
degraded chips, the C ABI of include/meda_follow.h and Router's fallback='follow' for MEDA.  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from marl_dmfb_amd import _lib
from marl_dmfb_amd.plan import follow_reference_meda, park_order_meda, plan_reference_meda
from meda_follow_helpers import (CASES, case, failure_safe, judge, parking_never_takes_a_droplet_inside_its_disc, partial_plans,
                                 reference)
from meda_plan_helpers import DENSE, DENSER, MAX_UNROUTED, SETS, consistent, dense_tasks, hand_cases, no_conflict, oracle_tasks
from meda_plan_helpers import judge as judge_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_FIELDS = ('positions', 'actions', 'steps', 'success', 'constraints', 'attempt', 'lower_bound')


def _checked(res, plain, width, length, s, g, oracle=True):
    """What every safe plan must be: consistent, without a conflict, failure-safe, green before the oracle, and with the plain
    rule's lower bound (a droplet planned alone sees no other).  Returns the share left unrouted."""
    np.testing.assert_array_equal(res.lower_bound, plain.lower_bound)
    routed = np.nonzero(res.success)[0]
    for b in routed:
        consistent(res, width, length, b)
        no_conflict(res, b)
        assert failure_safe(res, b) >= 36, 'task %d' % b
    assert (res.steps[routed] >= res.lower_bound[routed]).all() and (res.constraints == 0).all()
    if oracle:
        assert judge_plan(res, width, length, s, g) == len(routed)
    return float((~res.success).mean())


# ---------------------------------------------------------------------------------------------------- 1. the safe rule
@pytest.mark.parametrize('name', sorted(SETS))
def test_the_safe_rule_on_the_oracle_sets(name):
    """The share the safe rule leaves unrouted, beside the plain rule's (profiles/plan/NOTES.md): 30x30 / 4 0.0039 (plain 0),
    30x60 / 8 0, 60x60 / 16 0, 45x45 / 9 0.0156 (plain 0).  All four sets meet the planner's cap."""
    c = SETS[name]
    W, L = c['width'], c['length']
    s, g = oracle_tasks(**c)
    plain, safe = plan_reference_meda(W, L, s, g), plan_reference_meda(W, L, s, g, safe=True)
    off = plan_reference_meda(W, L, s, g, safe=False)
    for k in PLAN_FIELDS:                    # the keyword's default is the rule as it was
        np.testing.assert_array_equal(getattr(off, k), getattr(plain, k), err_msg=k)
    unrouted = _checked(safe, plain, W, L, s, g)
    print('%s: safe rule %.4f of %d tasks unrouted (plain %.4f), mean steps %.2f (plain %.2f)'
          % (name, unrouted, len(s), (~plain.success).mean(), safe.steps[safe.success].mean(), plain.steps[plain.success].mean()))
    assert unrouted <= MAX_UNROUTED
    # the guards cost steps and routes, never gain any: what the safe rule routes it routes no faster than the plain rule
    both = safe.success & plain.success
    assert (safe.steps[both] >= plain.lower_bound[both]).all() and (safe.positions != plain.positions).any()


def test_the_safe_rule_on_the_denser_sets():
    """Starts 6 apart and goals 6 apart.  The cap does not hold here and is not asserted: the safe rule leaves 0.3047 of DENSE
    (plain 0.0078) and 0.5156 of DENSER (plain 0.0234) unrouted, because a start 6 from another start has d2 = 36 exactly and
    almost every first move of one of the two would be unsafe if the other's failed."""
    s, g = dense_tasks(**DENSE)
    W, L = DENSE['width'], DENSE['length']
    unrouted = _checked(plan_reference_meda(W, L, s, g, safe=True), plan_reference_meda(W, L, s, g), W, L, s, g)
    print('DENSE: safe rule %.4f unrouted' % unrouted)
    assert unrouted < 0.5
    s, g = dense_tasks(**DENSER)
    unrouted = _checked(plan_reference_meda(30, 30, s, g, safe=True), plan_reference_meda(30, 30, s, g), 30, 30, s, g, oracle=False)
    print('DENSER: safe rule %.4f unrouted' % unrouted)
    assert unrouted < 0.75


@pytest.mark.parametrize('name', sorted(hand_cases()))
def test_the_safe_rule_on_the_hand_cases(name):
    c = hand_cases()[name]
    W, L, s, g = c['width'], c['length'], c['starts'], c['goals']
    plain = plan_reference_meda(W, L, s, g, avoid=c['avoid'])
    safe = plan_reference_meda(W, L, s, g, avoid=c['avoid'], safe=True)
    _checked(safe, plain, W, L, s, g)
    assert not (safe.success & ~plain.success).any()          # the safe reach sets are subsets of the plain ones
    if s.shape[1] == 1:                                       # a droplet alone sees no N: the two rules are one
        for k in PLAN_FIELDS:
            np.testing.assert_array_equal(getattr(safe, k), getattr(plain, k), err_msg=k)


# ---------------------------------------------------------------------------------------------------- 2. the safety property
def test_the_plain_rule_is_not_failure_safe_and_the_safe_rule_is():
    """Two droplets passing each other, starting on rows 4 apart.  The plain rule looks at the two planned positions of a level
    only: it takes (17, 10), (15, 16) to (20, 10), (13, 14), d2 = 65 when both moves succeed; but if the first one's move fails it
    is still on (17, 10) when the other arrives on (13, 14): d2 = 32.  The safe rule keeps the second droplet on row 16 one step
    longer."""
    s, g = np.array([[[5, 10], [26, 14]]]), np.array([[[26, 10], [5, 14]]])
    plain, safe = plan_reference_meda(30, 30, s, g), plan_reference_meda(30, 30, s, g, safe=True)
    assert plain.success[0] and safe.success[0]
    no_conflict(plain)                       # no conflict as long as every move succeeds
    assert failure_safe(plain) == 32 and failure_safe(safe) == 37
    assert judge_plan(safe, 30, 30, s, g) == 1
    # on rows 6 apart every combination is d2 >= 36 by the rows alone: the two rules plan the same straight lines
    s, g = np.array([[[5, 10], [26, 16]]]), np.array([[[26, 10], [5, 16]]])
    plain, safe = plan_reference_meda(30, 30, s, g), plan_reference_meda(30, 30, s, g, safe=True)
    np.testing.assert_array_equal(plain.positions, safe.positions)
    assert failure_safe(safe) == 36 and safe.steps[0] == 7


def test_the_property_is_what_the_env_counts():
    """The same hand case through the oracle with the one draw that fails the first droplet's third move: the plain plan, played
    open loop, is punished by the env; the closed loop never is."""
    from oracle.meda_oracle import MedaOracle
    s, g = np.array([[[5, 10], [26, 14]]]), np.array([[[26, 10], [5, 14]]])
    plain = plan_reference_meda(30, 30, s, g)
    p = plain.positions[0].astype(int)
    t_bad, i_bad = next((t, i) for t in range(int(plain.steps[0])) for i in (0, 1)
                        if ((p[t, i] - p[t + 1, 1 - i]) ** 2).sum() < 36)
    health = np.full((1, 30, 30), 0.5)
    u = np.zeros((60, 1, 2))
    u[t_bad, 0, i_bad] = 0.75                # above the move probability 0.5: that one move fails
    ora = MedaOracle(30, 30, 2, fov=19, n_envs=1, seed=0, with_maps=True)
    ora.set_map('health', health)
    ora.set_task(s, g)
    fails = [ora.step(plain.actions[0, t].astype(np.int32)[None], u[t])[2][0] for t in range(int(plain.steps[0]))]
    assert min(fails) < 0 and ora.get_state()['failed'][0] == 1
    res = follow_reference_meda(30, 30, s, g, health=health, uniforms=u)
    judge(res, 30, 30, s, g, health, u)
    assert res.success[0] and res.replans[0] >= 1


# ---------------------------------------------------------------------------------------------------- 3. the closed loop
@pytest.mark.parametrize('name', sorted(CASES))
def test_the_oracle_plays_every_followed_episode(name):
    c, s, g, health, uniforms = case(name)
    res = reference(name)
    judge(res, c['width'], c['length'], s, g, health, uniforms)
    parking_never_takes_a_droplet_inside_its_disc(res, g)
    assert res.replans.dtype == np.int32 and res.lower_bound.dtype == np.int32 and res.steps.dtype == np.int64
    assert (res.replans[~res.gave_up | (res.steps > 0)] >= 1).all()
    T = c['width'] + c['length']
    assert (res.positions[np.arange(len(res)), np.minimum(res.steps, T)] == res.positions[:, -1]).all()


def test_every_branch_of_the_loop_is_taken_by_the_cases():
    """Counted on the reference, so that no later change of a seed or a case can empty a branch unnoticed."""
    seen = {}
    for name in sorted(CASES):
        c, s, g, health, uniforms = case(name)
        res = reference(name)
        seen[name] = (int(res.success.sum()), int((res.replans > 1).sum()), int(partial_plans(res, c['width'], c['length'], g).sum()),
                      int(res.gave_up.sum()), int((res.lower_bound < 0).sum()))
        print(name, 'success %d, replans > 1 %d, partial plans %d, gave up %d, a goal out of reach %d, of %d'
              % (seen[name] + (len(res),)))
    for name, (success, replanned, partial, gave_up, unreachable) in seen.items():
        assert success > 0 and replanned > 0, name
    assert all(seen[k][2] > 0 for k in ('30x30_4', '30x60_8', '60x30_8', '20x64_4', '64x64_16', '30x30_4_many'))
    for name in ('30x30_4_min_health', '30x60_8_min_health'):      # blocked centres: goals out of reach, parking, giving up
        success, replanned, partial, gave_up, unreachable = seen[name]
        assert partial > 0 and gave_up > 0 and unreachable > 0, name
    assert seen['15x15_1'][0] == 64                                 # a droplet alone always arrives


@pytest.mark.parametrize('name', ['30x30_4', '30x60_8', '45x45_9'])
def test_on_healthy_chips_the_follower_plays_the_safe_plan(name):
    c = SETS[name]
    W, L = c['width'], c['length']
    s, g = oracle_tasks(**dict(c, B=48))
    plan = plan_reference_meda(W, L, s, g, safe=True)
    ok = plan.success
    res = follow_reference_meda(W, L, s, g, health=np.ones((48, W, L)) if name == '30x30_4' else None)
    for k in ('positions', 'actions', 'steps', 'success', 'constraints'):
        np.testing.assert_array_equal(getattr(res, k)[ok], getattr(plan, k)[ok], err_msg=k)
    np.testing.assert_array_equal(res.lower_bound, plan.lower_bound)
    assert ok.any() and (res.replans[ok] == 1).all() and not res.gave_up[ok].any()
    assert ((res.replans[~ok] > 1) | res.gave_up[~ok]).all()
    judge(res, W, L, s, g, None, None)


def test_min_health_blocks_the_centres_whose_box_touches_a_worn_cell():
    from marl_dmfb_amd.plan import _meda_blocked
    c, s, g, health, uniforms = case('30x30_4_min_health')
    res = reference('30x30_4_min_health')
    p = res.positions.astype(int)
    B = len(res)
    entered = 0
    for b in range(B):
        blocked = _meda_blocked(30, 30, health[b] < 0.9)
        on = blocked[p[b, ..., 1], p[b, ..., 0]]                                # (T+1, n)
        moved = (p[b, 1:] != p[b, :-1]).any(axis=-1)
        # a droplet may start on a blocked centre and leave it; the one blocked centre a droplet may come to is its goal, by the
        # env's snap, which no plan can stop
        snapped = (p[b, 1:] == g[b][None]).all(axis=-1)
        assert not (on[1:] & moved & ~snapped).any(), b
        entered += int(on[0].sum())
    assert entered > 0
    # the same call with `avoid` in place of the threshold is the same episode, and the threshold does change the routes
    same = follow_reference_meda(30, 30, s[:8], g[:8], avoid=health[:8] < 0.9, health=health[:8], uniforms=uniforms[:, :8])
    free = follow_reference_meda(30, 30, s[:8], g[:8], health=health[:8], uniforms=uniforms[:, :8])
    for k in ('positions', 'actions', 'steps', 'replans', 'gave_up'):
        np.testing.assert_array_equal(getattr(same, k), getattr(res, k)[:8], err_msg=k)
    assert (free.positions != res.positions[:8]).any()


def test_parking_and_the_goal_disc():
    # ascending d2 outside the disc, ties by descending index; d2 < 16 is never listed
    assert park_order_meda([(2, 2), (10, 10), (20, 20), (5, 20)], [(2, 6), (10, 13), (20, 24), (5, 24)]) == [3, 2, 0]
    assert park_order_meda([(2, 2)], [(2, 2)]) == []
    # droplet 0 stands inside its disc, droplet 1's goal is walled off, droplet 2 crosses the chip: the chip is planned with
    # droplet 1 parked (the nearer of the two candidates; the farthest is never parked), droplet 0 is snapped by the first step,
    # and the follower gives up when droplet 2 has come nearer its goal than droplet 1 is to its own (d2 = 193): from then on
    # droplet 2 is the one parked first, and nothing routes droplet 1
    s, g = np.array([[[10, 10], [27, 27], [2, 27]]]), np.array([[[12, 12], [15, 20], [27, 2]]])
    assert park_order_meda([tuple(p) for p in s[0].tolist()], [tuple(p) for p in g[0].tolist()]) == [1, 2]
    avoid = np.zeros((1, 30, 30), bool)
    avoid[0, 14:27, 9] = avoid[0, 14:27, 21] = avoid[0, 14, 9:22] = avoid[0, 26, 9:22] = True
    res = follow_reference_meda(30, 30, s, g, avoid=avoid)
    steps = int(res.steps[0])
    assert res.lower_bound[0] == -1 and not res.success[0] and res.gave_up[0] and res.replans[0] == steps > 2
    assert res.positions[0, 1, 0].tolist() == [12, 12] and res.actions[0, 0, :2].tolist() == [8, 8]
    assert (res.positions[0, :, 1] == (27, 27)).all() and (res.actions[0, :steps, 1] == 8).all() and (res.constraints == 0).all()
    d2 = ((res.positions[0, :steps + 1, 2].astype(int) - g[0, 2]) ** 2).sum(axis=1)
    assert (d2[:-1] > 193).all() and d2[-1] < 193


def test_a_draw_equal_to_the_box_mean_moves():
    s, g = np.array([[[5, 5]]]), np.array([[[20, 5]]])
    health = np.full((1, 30, 30), 0.75)
    u = np.full((60, 1, 1), 0.75)
    res = follow_reference_meda(30, 30, s, g, health=health, uniforms=u)
    assert res.success[0] and res.steps[0] == 5 and res.replans[0] == 1
    assert res.actions[0, :6, 0].tolist() == [1, 1, 1, 1, 8, -1]
    res = follow_reference_meda(30, 30, s, g, health=health, uniforms=np.nextafter(u, 1.0))
    assert not res.success[0] and res.steps[0] == 60 and (res.positions[0] == (5, 5)).all() and res.replans[0] == 60
    u2 = u.copy()
    u2[1] = 0.8                                   # one failed move: one replan, one step more
    res = follow_reference_meda(30, 30, s, g, health=health, uniforms=u2)
    assert res.success[0] and res.steps[0] == 6 and res.replans[0] == 2


def test_inputs_are_validated():
    s, g = np.array([[[5, 5]]]), np.array([[[20, 5]]])
    with pytest.raises(ValueError, match='uniforms must have shape'):
        follow_reference_meda(30, 30, s, g, uniforms=np.zeros((59, 1, 1)))
    with pytest.raises(ValueError, match='avoid must have shape'):
        follow_reference_meda(30, 30, s, g, avoid=np.zeros((1, 30, 29)))
    with pytest.raises(ValueError, match='off the chip'):
        follow_reference_meda(30, 30, np.array([[[1, 5]]]), g)
    empty = follow_reference_meda(30, 30, np.zeros((0, 4, 2), int), np.zeros((0, 4, 2), int))
    assert len(empty) == 0 and empty.positions.shape == (0, 61, 4, 2) and empty.constraints.dtype == np.float64


# ---------------------------------------------------------------------------------------------------- 5. C ABI
def test_meda_follow_header_matches_the_binding_table():
    txt = open(os.path.join(ROOT, 'include', 'meda_follow.h')).read()
    limit = int(re.search(r'#define MEDA_FOLLOW_MAX_DIM (\d+)', txt).group(1))
    most = int(re.search(r'#define MEDA_FOLLOW_MAX_AGENTS (\d+)', txt).group(1))
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    txt = re.sub(r'^\s*#.*$', '', txt, flags=re.M)
    declared = {name: (0 if p.strip() in ('', 'void') else p.count(',') + 1)
                for name, p in re.findall(r'\b([a-z][a-z_0-9]*)\s*\(([^()]*)\)\s*;', txt)}
    assert declared == {'meda_follow_plan': 14, 'meda_follow_step': 21, 'meda_follow_max_dim': 0, 'meda_follow_lds_bytes': 3,
                        'meda_follow_last_hip_error': 0}
    table = _lib.SIGNATURES['meda_follow']
    assert sorted(table) == sorted(declared)
    raw = _lib.meda_follow()
    for name, n in declared.items():
        sig = table[name]
        argtypes = sig[0] if isinstance(sig, tuple) else sig
        assert len(argtypes) == n and len(getattr(raw, name).argtypes) == n, name
    from marl_dmfb_amd import plan
    assert raw.meda_follow_max_dim() == limit == plan.MEDA_MAX_DIM == _lib.meda_plan().meda_plan_max_dim()
    assert most == plan.MEDA_MAX_AGENTS
    formula = lambda w, l, n: (w + l - 1) * w * 8 + (((w + l + 1) * n * 2 + 15) // 16) * 16
    for w, l, n in ((30, 30, 4), (30, 60, 8), (60, 30, 8), (20, 64, 4), (15, 15, 1), (5, 5, 1), (64, 64, 16)):
        assert raw.meda_follow_lds_bytes(w, l, n) == formula(w, l, n) == _lib.meda_plan().meda_plan_lds_bytes(w, l, n), (w, l, n)
    assert 64 * 1024 < raw.meda_follow_lds_bytes(limit, limit, most) <= 160 * 1024 - 1024
    assert raw.meda_follow_lds_bytes(limit + 1, 30, 4) == -6 and raw.meda_follow_lds_bytes(30, 30, most + 1) == -6
    assert raw.meda_follow_lds_bytes(4, 30, 4) == -1 and raw.meda_follow_lds_bytes(30, 30, 0) == -1
    assert _lib._LAST_ERROR['meda_follow_'] == 'meda_follow_last_hip_error'
    assert _lib.ENV_ERRORS['meda_follow'][-1][0] is ValueError and _lib.ENV_ERRORS['meda_follow'][-6][0] is NotImplementedError
    # the two pinned headers keep their prototypes
    assert sorted(_lib.SIGNATURES['meda_plan']) == ['meda_plan_last_hip_error', 'meda_plan_lds_bytes', 'meda_plan_max_dim',
                                                    'meda_plan_route']


def test_meda_follow_argument_guards_need_no_gpu():
    """Dummy non-null pointers in a child process that sees no GPU: a launch there would come back as a HIP error (-100), never as
    -1, -6 or 0."""
    child = r'''
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from marl_dmfb_amd import _lib
lib = _lib.meda_follow()
host = C.create_string_buffer(4096)
p = C.addressof(host)
def plan(B=4, W=30, L=30, n=4, s=p, g=p, avoid=None, route=p, u=p, steps=p, success=p, attempt=p, lower=p):
    return lib.meda_follow_plan(B, W, L, n, s, g, avoid, route, u, steps, success, attempt, lower, None)
names = ('goals', 'avoid', 'positions', 'terminated', 'route', 'route_u', 'cursor', 'partial', 'replans', 'gave_up', 'active',
         'steps', 'lower', 'actions', 'u')
def step(B=4, W=30, L=30, n=4, t=0, **ptr):
    a = dict({k: p for k in names}, avoid=None)
    a.update(ptr)
    return lib.meda_follow_step(B, W, L, n, t, *[a[k] for k in names], None)
M = lib.meda_follow_max_dim()
print(plan(B=-1), plan(W=0), plan(L=-3), plan(W=4), plan(n=0), plan(s=None), plan(g=None), plan(route=None), plan(u=None),
      plan(steps=None), plan(success=None), plan(attempt=None), plan(lower=None))
print(plan(W=M + 1), plan(L=M + 1), plan(n=17), plan(W=M + 1, L=M + 1, n=16))
print(plan(B=0), plan(B=0, W=M, L=M, n=16, avoid=p))
print(step(B=-1), step(W=0), step(L=-3), step(W=4), step(n=0), step(t=-1), step(t=60), step(positions=p + 1), step(route=p + 1),
      *[step(**{k: None}) for k in names if k != 'avoid'])
print(step(W=M + 1), step(L=M + 1), step(n=17))
print(step(B=0), step(B=0, W=M, L=M, n=16, avoid=p, t=2 * M - 1))
'''
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', ROCR_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1')
    out = subprocess.run([sys.executable, '-c', child, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == ['-1'] * 13, out.stdout
    assert lines[1].split() == ['-6'] * 4, out.stdout
    assert lines[2].split() == ['0'] * 2, out.stdout
    assert lines[3].split() == ['-1'] * (9 + 14), out.stdout
    assert lines[4].split() == ['-6'] * 3, out.stdout
    assert lines[5].split() == ['0'] * 2, out.stdout


# ---------------------------------------------------------------------------------------------------- 6. Router
class _FakeFollower:
    """follow_reference_meda behind the interface of MedaPlanner.follow (no GPU here); the draws come from numpy."""

    def __init__(self, width, length, n_agents):
        self.width, self.length, self.n_agents, self.calls = width, length, n_agents, []

    def follow(self, starts, goals, avoid=None, health=None, min_health=0.0, seed=0, uniforms=None, use_graph=False):
        self.calls.append((len(starts), min_health, seed))
        T = self.width + self.length
        u = np.random.default_rng(seed).random((T, len(starts), self.n_agents))
        return follow_reference_meda(self.width, self.length, starts, goals, avoid=avoid, health=health, min_health=min_health,
                                     uniforms=u)


def test_router_takes_the_follower_of_a_given_planner_for_meda():
    from marl_dmfb_amd.route import RouteResult, Router, round_stream
    m = Router(None, name='meda', width=30, length=30, n_agents=4, fov=19, device='cpu')
    s, g = oracle_tasks(**dict(SETS['30x30_4'], B=48))
    with pytest.raises(ValueError, match='DMFB only'):
        m.route(s, g, fallback='follow')
    with pytest.raises(ValueError, match='follow'):
        m.route(s, g, fallback='follow', planner=object())

    class OnlyPlans:
        width, length, n_agents = 30, 30, 4

        def plan(self, *a, **k):
            raise AssertionError('not to be called')
    with pytest.raises(ValueError, match='follow'):
        m.route(s, g, fallback='follow', planner=OnlyPlans())
    with pytest.raises(ValueError, match='planner is for'):
        m.route(s, g, fallback='follow', planner=_FakeFollower(30, 60, 4))
    assert m.rounds == 0 and not m._slots
    empty = m.route(np.zeros((0, 4, 2), int), np.zeros((0, 4, 2), int), fallback='follow', planner=_FakeFollower(30, 30, 4))
    assert len(empty) == 0 and empty.constraints.dtype == np.float64

    # Router._follow with a result as a policy would leave it: two tasks of three failed
    T, B = 60, 48
    failed = np.arange(B) % 3 != 0
    health = np.random.default_rng(5).uniform(0.6, 1.0, (B, 30, 30))

    def policy():
        rng = np.random.default_rng(0)
        return RouteResult(rng.integers(2, 27, (B, T + 1, 4, 2)).astype(np.uint8), rng.integers(0, 9, (B, T, 4)).astype(np.int8),
                           np.where(failed, T, 12).astype(np.int64), ~failed, np.where(failed, -1.2, 0.0),
                           np.arange(B, dtype=np.int32) % 3)
    before, res, fake = policy(), policy(), _FakeFollower(30, 30, 4)
    out = m._follow(res, s, g, None, health, 0.25, 9, fake)
    gen_seed = round_stream(9, 0, 2)[1]
    assert out is res and fake.calls == [(32, 0.25, gen_seed)]
    fol = _FakeFollower(30, 30, 4).follow(s[failed], g[failed], health=health[failed], min_health=0.25, seed=gen_seed)
    took = np.zeros(B, bool)
    took[np.nonzero(failed)[0][fol.success]] = True
    assert took.any() and (took != failed).any()               # some followed episodes succeeded, not all
    np.testing.assert_array_equal(res.source, np.where(took, 2, 0).astype(np.int8))
    for k in ('positions', 'actions', 'steps', 'success', 'constraints'):
        np.testing.assert_array_equal(getattr(res, k)[took], getattr(fol, k)[fol.success], err_msg=k)
        np.testing.assert_array_equal(getattr(res, k)[~took], getattr(before, k)[~took], err_msg=k)
        assert getattr(res, k).dtype == getattr(before, k).dtype
    assert (res.try_index[took] == -1).all() and res.success[took].all()
    np.testing.assert_array_equal(res.try_index[~took], before.try_index[~took])
