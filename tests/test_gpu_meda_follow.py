"""Closed-loop planner routing for MEDA on the GPU (marl_dmfb_amd.plan.MedaFollower / MedaPlanner.follow / MedaPlanner.plan(safe=True),
include/meda_follow.h): the safe rule against plan_reference_meda(safe=True) and every field of the closed loop against
follow_reference_meda bit for bit, determinism, the HIP env as judge, Router's fallback and the argument checks."""
import numpy as np
import pytest
import torch

from meda_follow_helpers import CASES, FIELDS, case, equal, reference
from meda_plan_helpers import DENSE, DENSER, SETS, dense_tasks, hand_cases, oracle_tasks
from meda_plan_helpers import equal as equal_plan
from vdn_helpers import det_init

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_PLANNERS = {}


def _planner(W, L, n):
    from marl_dmfb_amd.plan import MedaPlanner
    key = (W, L, n)
    if key not in _PLANNERS:
        _PLANNERS[key] = MedaPlanner(W, L, n, device=DEV)
    return _PLANNERS[key]


def _follow(name, **kw):
    c, s, g, health, uniforms = case(name)
    return _planner(c['width'], c['length'], c['n_agents']).follow(s, g, health=health, uniforms=uniforms,
                                                                    min_health=c.get('min_health', 0.0), **kw)


# ---------------------------------------------------------------------------------------------------- 1. the safe rule
def _both(width, length, s, g, avoid=None):
    """The safe rule and, beside it, the plain one through the same MedaPlanner: each against its numpy statement."""
    from marl_dmfb_amd.plan import plan_reference_meda
    planner = _planner(width, length, s.shape[1])
    equal_plan(planner.plan(s, g, avoid=avoid), plan_reference_meda(width, length, s, g, avoid=avoid))
    got = planner.plan(s, g, avoid=avoid, safe=True)
    equal_plan(got, plan_reference_meda(width, length, s, g, avoid=avoid, safe=True))
    return got


@pytest.mark.parametrize('name', sorted(SETS))
def test_safe_planner_equals_the_reference_on_the_oracle_sets(name):
    c = SETS[name]
    s, g = oracle_tasks(**c)
    assert _both(c['width'], c['length'], s, g).success.mean() >= 0.9


@pytest.mark.parametrize('cfg', [DENSE, DENSER], ids=['30x60_8', '30x30_6'])
def test_safe_planner_equals_the_reference_on_the_denser_sets(cfg):
    s, g = dense_tasks(**cfg)
    res = _both(cfg['width'], cfg['length'], s, g)
    assert (res.attempt > 0).any() and (~res.success).any() and res.success.any()


@pytest.mark.parametrize('name', sorted(hand_cases()))
def test_safe_planner_equals_the_reference_on_the_hand_cases(name):
    c = hand_cases()[name]
    _both(c['width'], c['length'], c['starts'], c['goals'], avoid=c['avoid'])


# ---------------------------------------------------------------------------------------------------- 2. kernel == the loop
@pytest.mark.parametrize('name', sorted(CASES))
def test_follow_equals_the_reference(name):
    got, want = _follow(name), reference(name)
    equal(got, want)
    assert got.reward.dtype == np.float64 and got.reward.shape == want.steps.shape and got.constraints.dtype == np.float64


def test_on_healthy_chips_the_follower_plays_the_safe_plan():
    c = SETS['30x30_4']
    s, g = oracle_tasks(**c)
    planner = _planner(30, 30, 4)
    plan, res = planner.plan(s, g, safe=True), planner.follow(s, g)
    ok = plan.success
    assert ok.mean() > 0.9 and (~ok).any()
    for k in ('positions', 'actions', 'steps', 'success', 'constraints'):
        np.testing.assert_array_equal(getattr(res, k)[ok], getattr(plan, k)[ok], err_msg=k)
    np.testing.assert_array_equal(res.lower_bound, plan.lower_bound)
    assert (res.replans[ok] == 1).all() and not res.gave_up[ok].any()
    assert ((res.replans[~ok] > 1) | res.gave_up[~ok]).all()
    # all ones as a health map: the same episodes on a handle with maps
    equal(planner.follow(s, g, health=np.ones((len(s), 30, 30)), uniforms=np.full((60, len(s), 4), 0.999)), res)


# ---------------------------------------------------------------------------------------------------- 3. determinism
def test_eager_graph_repeat_and_side_stream_give_the_same_bytes():
    first = _follow('20x64_4')
    equal(_follow('20x64_4'), first)
    captured = _follow('20x64_4', use_graph=True)
    equal(captured, first)
    equal(_follow('20x64_4', use_graph=True), first)       # the replay
    np.testing.assert_array_equal(captured.reward.view(np.int64), first.reward.view(np.int64))
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        third = _follow('20x64_4')
    side.synchronize()
    equal(third, first)
    # drawn from a seed instead of given: the same seed, the same episodes
    c, s, g, health, _ = case('20x64_4')
    p = _planner(20, 64, 4)
    a, a2, other = (p.follow(s, g, health=health, seed=k) for k in (5, 5, 6))
    equal(a2, a)
    assert (other.positions != a.positions).any()


# ---------------------------------------------------------------------------------------------------- 4. the env as judge
def test_the_env_counts_no_failure_and_grants_the_successes():
    from marl_dmfb_amd.env.meda import VecMEDA
    from marl_dmfb_amd.plan import MedaFollower
    s, g, health, uniforms = (a.copy() for a in case('30x30_4')[1:])      # torch takes no read-only array
    B, T = len(s), 60
    env = VecMEDA(30, 30, 4, fov=19, n_envs=B, seed=0, with_maps=True, device=DEV)
    env.set_task(s, g)
    env.set_map('health', health)
    env.restart()
    res = MedaFollower(env).play(uniforms=uniforms, record=False)
    want = reference('30x30_4')
    host = type(want)(*[getattr(res, k).cpu().numpy() for k in FIELDS])
    equal(host, want)
    assert (host.constraints == 0).all()                       # summed by the env over every step of every chip
    st = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    assert (st['failed'] == 0).all()
    np.testing.assert_array_equal(st['step_count'], want.steps)
    np.testing.assert_array_equal(host.success, (st['status'] == 1).all(axis=1) & (want.steps < T) & ~host.gave_up)
    assert host.success.any() and host.gave_up.any()
    # the Philox stream of the handle in place of given draws: a legal episode all the same
    env.set_task(s, g)
    env.restart()
    res = MedaFollower(env).play(record=False)
    assert (res.constraints == 0).all() and (env.get_state()['failed'] == 0).all() and res.success.float().mean() > 0.5


# ---------------------------------------------------------------------------------------------------- 5. Router fallback
def test_router_follow_fallback_replaces_only_the_failed_tasks():
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.meda import VecMEDA
    from marl_dmfb_amd.route import Router, round_stream
    cfg = dict(width=30, length=30, n_agents=4, fov=19)
    probe = VecMEDA(n_envs=1, device=DEV, **cfg)
    args = make_args(name='meda', drop_num=4, width=30, length=30, fov=19, device=DEV, alg='vdn', **probe.get_env_info())
    agents = Agents(args)
    det_init(agents.policy.eval_rnn, salt=0.25)
    s, g = oracle_tasks(**dict(SETS['30x30_4'], B=64))
    health = np.random.default_rng(3).uniform(0.6, 1.0, (64, 30, 30))
    router = Router(agents, name='meda', device=DEV, **cfg)
    planner = _planner(30, 30, 4)
    policy = ('positions', 'actions', 'steps', 'success', 'constraints', 'try_index')
    before = router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4)
    assert (~before.success).any() and (before.source == 0).all()
    res = router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4, fallback='follow', planner=planner)
    after = router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4)
    for k in policy:
        np.testing.assert_array_equal(getattr(after, k), getattr(before, k), err_msg=k)
    failed = np.nonzero(~before.success)[0]
    fol = planner.follow(s[failed], g[failed], health=health[failed], seed=round_stream(4, 0, 2)[1])
    took = np.zeros(64, bool)
    took[failed[fol.success]] = True
    assert took.any() and res.source.dtype == np.int8
    np.testing.assert_array_equal(res.source, np.where(took, 2, 0))
    for k in policy:
        np.testing.assert_array_equal(getattr(res, k)[~took], getattr(before, k)[~took], err_msg=k)
        assert getattr(res, k).dtype == getattr(before, k).dtype
    for k in ('positions', 'actions', 'steps', 'success', 'constraints'):
        np.testing.assert_array_equal(getattr(res, k)[took], getattr(fol, k)[fol.success], err_msg=k)
    assert (res.try_index[took] == -1).all() and res.success[took].all() and res.lower_bound is None
    # the open-loop planner routes nothing on these chips: every box has a cell below 1.0
    assert not router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4, fallback='plan', planner=planner).source.any()


# ---------------------------------------------------------------------------------------------------- 6. argument checks
def test_meda_follow_step_argument_checks():
    from marl_dmfb_amd import _lib
    lib = _lib.meda_follow()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    names = ('goals', 'avoid', 'positions', 'terminated', 'route', 'route_u', 'cursor', 'partial', 'replans', 'gave_up', 'active',
             'steps', 'lower', 'actions', 'u')

    def call(B=1, W=30, L=30, n=4, t=0, **ptr):
        a = dict({k: p for k in names}, avoid=None)
        a.update(ptr)
        return lib.meda_follow_step(B, W, L, n, t, *[a[k] for k in names], None)

    bad = [call(B=-1), call(W=0), call(L=-3), call(W=4), call(n=0), call(t=-1), call(t=60), call(positions=p + 1), call(route=p + 1)]
    bad += [call(**{k: None}) for k in names if k != 'avoid']
    assert bad == [-1] * len(bad)
    M = lib.meda_follow_max_dim()
    assert [call(W=M + 1), call(L=M + 1), call(n=17)] == [-6, -6, -6]
    assert call(B=0) == 0 and call(B=0, W=M, L=M, n=16, avoid=p, t=2 * M - 1) == 0
    # a chip whose active byte is 0 is left alone: nothing of the (zeroed) buffers is read further or written
    assert call() == 0 and call(t=5) == 0
    torch.cuda.synchronize()
    assert int(buf.sum().item()) == 0
    checked = _lib.checked('meda_follow')
    with pytest.raises(NotImplementedError):
        checked.meda_follow_step(1, 65, 30, 4, 0, *[p] * 15, None)
    with pytest.raises(ValueError):
        checked.meda_follow_step(1, 30, 30, 4, 60, *[p] * 15, None)
