"""Closed-loop routing on the GPU (marl_dmfb_amd.plan.Follower / Planner.follow, include/route_plan.h: route_follow_dmfb): every
field against follow_reference bit for bit, the planner on healthy chips, determinism, the HIP env as judge, Router's fallback,
the evaDegre driver and the argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from follow_helpers import CASES, FIELDS, case, equal, reference
from plan_helpers import SETS, oracle_tasks
from vdn_helpers import det_init

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_PLANNERS = {}


def _planner(W, L, n):
    from marl_dmfb_amd.plan import Planner
    key = (W, L, n)
    if key not in _PLANNERS:
        _PLANNERS[key] = Planner(W, L, n, device=DEV)
    return _PLANNERS[key]


def _follow(name, **kw):
    c, s, g, b, health, uniforms = case(name)
    return _planner(c['width'], c['length'], c['n_agents']).follow(s, g, blocks=b, health=health, uniforms=uniforms,
                                                                    min_health=c.get('min_health', 0.0), **kw)


# ---------------------------------------------------------------------------------------------------- 1. kernel == the rule
@pytest.mark.parametrize('name', sorted(CASES))
def test_follow_equals_the_reference(name):
    got, want = _follow(name), reference(name)
    equal(got, want)
    assert got.reward.dtype == np.float64 and got.reward.shape == want.steps.shape


def test_on_healthy_chips_the_follower_plays_the_plan():
    c = SETS['10x10_4_2b']
    s, g, b = oracle_tasks(**c)
    planner = _planner(10, 10, 4)
    plan, res = planner.plan(s, g, blocks=b), planner.follow(s, g, blocks=b)
    ok = plan.success
    assert ok.mean() > 0.9 and (~ok).any()
    for k in ('positions', 'actions', 'steps', 'success', 'constraints'):
        np.testing.assert_array_equal(getattr(res, k)[ok], getattr(plan, k)[ok], err_msg=k)
    np.testing.assert_array_equal(res.lower_bound, plan.lower_bound)
    assert (res.replans[ok] == 1).all() and not res.gave_up[ok].any()
    assert ((res.replans[~ok] > 1) | res.gave_up[~ok]).all()
    # all ones as a health map: the same episodes on a handle with maps
    equal(planner.follow(s, g, blocks=b, health=np.ones((len(s), 10, 10)), uniforms=np.full((40, len(s), 4), 0.999)), res)


# ---------------------------------------------------------------------------------------------------- 2. determinism
def test_eager_graph_repeat_and_side_stream_give_the_same_bytes():
    first = _follow('12x30_5_2b')
    equal(_follow('12x30_5_2b'), first)
    captured = _follow('12x30_5_2b', use_graph=True)
    equal(captured, first)
    equal(_follow('12x30_5_2b', use_graph=True), first)       # the replay
    np.testing.assert_array_equal(captured.reward.view(np.int64), first.reward.view(np.int64))
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        third = _follow('12x30_5_2b')
    side.synchronize()
    equal(third, first)
    # drawn from a seed instead of given: the same seed, the same episodes
    c, s, g, b, health, _ = case('12x30_5_2b')
    p = _planner(12, 30, 5)
    a, a2, other = (p.follow(s, g, blocks=b, health=health, seed=k) for k in (5, 5, 6))
    equal(a2, a)
    assert (other.positions != a.positions).any()


# ---------------------------------------------------------------------------------------------------- 3. the env as judge
def test_the_env_counts_no_constraint_and_grants_the_successes():
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.plan import Follower
    s, g, b, health, uniforms = (a.copy() for a in case('10x10_4_2b')[1:])      # torch takes no read-only array
    B = len(s)
    env = VecDMFB(10, 10, 4, 2, fov=9, n_envs=B, seed=0, with_maps=True, device=DEV)
    env.set_task(s, g)
    env.set_blocks(b)
    env.set_map('health', health)
    env.restart()
    res = Follower(env).play(uniforms=uniforms, record=False)
    want = reference('10x10_4_2b')
    host = type(want)(*[getattr(res, k).cpu().numpy() for k in FIELDS])
    equal(host, want)
    assert (host.constraints == 0).all()                       # summed by the env over every step of every chip
    st = env.get_state()
    assert (st['constraints'].cpu().numpy() == 0).all()
    np.testing.assert_array_equal(st['step_count'].cpu().numpy(), want.steps)
    home = (st['dist'].cpu().numpy() == 0).all(axis=1)
    np.testing.assert_array_equal(host.success, home & (want.steps < 40))     # the env's flag is what the rule says
    assert host.success.any() and host.gave_up.any()
    # the Philox stream of the handle in place of given draws: a legal episode all the same
    env.restart()
    res = Follower(env).play(record=False)
    assert (res.constraints == 0).all() and res.success.float().mean() > 0.5


# ---------------------------------------------------------------------------------------------------- 4. Router fallback
def _agents(cfg):
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.dmfb import VecDMFB
    env = VecDMFB(n_envs=1, device=DEV, **cfg)
    args = make_args(name='dmfb', drop_num=env.n_agents, width=env.width, length=env.length, fov=env.fov, device=DEV, alg='vdn',
                     **env.get_env_info())
    agents = Agents(args)
    det_init(agents.policy.eval_rnn, salt=0.25)
    return agents


def test_router_follow_fallback_replaces_only_the_failed_tasks():
    from marl_dmfb_amd.route import Router, round_stream
    cfg = dict(width=10, length=10, n_agents=4, fov=9)
    s, g, _ = oracle_tasks(**dict(SETS['10x10_4'], B=64))
    health = np.random.default_rng(3).uniform(0.6, 1.0, (64, 10, 10))
    router = Router(_agents(cfg), name='dmfb', device=DEV, **cfg)
    policy = ('positions', 'actions', 'steps', 'success', 'constraints', 'try_index')
    before = router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4)
    assert (~before.success).any() and (before.source == 0).all()
    res = router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4, fallback='follow')
    after = router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4)
    for k in policy:
        np.testing.assert_array_equal(getattr(after, k), getattr(before, k), err_msg=k)
    failed = np.nonzero(~before.success)[0]
    fol = _planner(10, 10, 4).follow(s[failed], g[failed], health=health[failed], seed=round_stream(4, 0, 2)[1])
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
    # the open-loop planner routes nothing on these chips: every electrode is below 1.0
    assert not router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4, fallback='plan').source.any()


# ---------------------------------------------------------------------------------------------------- 5. the evaDegre driver
def test_evadegre_with_the_follower_writes_the_four_files(tmp_path, monkeypatch):
    from marl_dmfb_amd import evaDegre
    monkeypatch.chdir(tmp_path)
    evaDegre.main(['dmfb', '--chip_size', '10', '--drop_num', '4', '--fov', '9', '--n_envs', '2', '--evaluate_epoch', '2',
                   '--evaluate_task', '2', '--router', 'follow', '--min_health', '0.2'])
    d = tmp_path / 'DegreData_follow' / '10by10-4d0b'
    assert sorted(os.listdir(d)) == ['health.npy', 'rewards.npy', 'steps.npy', 'success.npy']
    out = {k: np.load(d / (k + '.npy')) for k in ('rewards', 'steps', 'success', 'health')}
    for k in ('rewards', 'steps', 'success'):
        assert out[k].shape == (2, 2) and out[k].dtype == np.float64
    assert out['health'].shape == (2, 2, 10, 10)
    assert (out['health'][:, 1] <= out['health'][:, 0]).all()              # four short episodes wear no electrode past 50 uses
    assert ((out['success'] >= 0) & (out['success'] <= 1)).all() and ((out['steps'] > 0) & (out['steps'] <= 40)).all()
    assert not (tmp_path / 'DegreData').exists()


def test_chips_age_under_the_follower():
    """record=True: the follower's steps count as usage, and reset(new=False) between its episodes degrades the electrodes."""
    from types import SimpleNamespace
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.evaDegre import Degre_follower
    env = VecDMFB(10, 10, 4, fov=9, b_degrade=True, per_degrade=1.0, n_envs=2, seed=1, device=DEV)
    env.set_map('usage', torch.full((2, 10, 10), 50.0, dtype=torch.float64))     # one more use passes the threshold of 50
    _, steps, success, health = Degre_follower(env, SimpleNamespace(min_health=0.0, evaluate_epoch=3, evaluate_task=2)).evaluate_process()
    assert (health[:, 0] == 1.0).all() and (np.diff(health, axis=1) <= 0).all() and (health > 0).all()
    assert (health[:, 1].min(axis=(1, 2)) < 1.0).all()                         # every chip wore some electrode in its first epoch
    assert ((success >= 0) & (success <= 1)).all() and ((steps > 0) & (steps <= 40)).all()


# ---------------------------------------------------------------------------------------------------- 6. argument checks
def test_route_follow_argument_checks():
    from marl_dmfb_amd import _lib
    lib = _lib.route_plan()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    names = ('goals', 'blocks', 'avoid', 'positions', 'route', 'route_u', 'cursor', 'partial', 'replans', 'gave_up', 'active',
             'steps', 'lower', 'actions', 'u')

    def call(B=1, W=10, L=10, n=4, nb=0, t=0, **ptr):
        a = dict({k: p for k in names}, blocks=None, avoid=None)
        a.update(ptr)
        return lib.route_follow_dmfb(B, W, L, n, nb, t, *[a[k] for k in names], None)

    bad = [call(B=-1), call(W=0), call(L=-3), call(n=0), call(n=17), call(nb=-1), call(nb=2), call(t=-1), call(t=40),
           call(positions=p + 1), call(route=p + 1)]
    bad += [call(**{k: None}) for k in names if k not in ('blocks', 'avoid')]
    assert bad == [-1] * len(bad)
    M = lib.route_plan_max_dim()
    assert [call(W=M + 1), call(L=M + 1)] == [-6, -6]
    assert call(B=0) == 0 and call(B=0, W=M, L=M, n=16, nb=3, blocks=p, avoid=p, t=4 * M - 1) == 0
    # a chip whose active byte is 0 is left alone: nothing of the (zeroed) buffers is read further or written
    assert call() == 0
    torch.cuda.synchronize()
    assert int(buf.sum().item()) == 0
    checked = _lib.checked('route_plan')
    with pytest.raises(NotImplementedError):
        checked.route_follow_dmfb(1, 65, 10, 4, 0, 0, *[p] * 15, None)
    with pytest.raises(ValueError):
        checked.route_follow_dmfb(1, 10, 10, 4, 0, 40, *[p] * 15, None)
