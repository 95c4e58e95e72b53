"""Reservations and retries of the DMFB planner on the GPU (marl_dmfb_amd.plan.Planner(reserve=, retries=), include/route_plan.h:
route_plan_dmfb_opt / route_follow_dmfb_opt): every output array against plan_reference / follow_reference bit for bit, the old
entry points against the new ones at 0 / 0, eager and captured closed loops, and Router's fallbacks with a given planner."""
import functools

import numpy as np
import pytest
import torch

from plan_helpers import SETS, equal, oracle_tasks, router_fallback_substitutes_only_the_failed_tasks
from plan_reserve_helpers import CORNERED_GOALS, CORNERED_STARTS, CORNERED_STEPS, RETRY_GOALS, RETRY_STARTS
import follow_helpers
from vdn_helpers import det_init

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# name -> (oracle_tasks arguments, B), or the literal tasks
PLAN_CASES = {
    '10x10_4_2b': (dict(width=10, length=10, n_agents=4, n_blocks=2, seed=2), 256),
    '20x20_10': (dict(width=20, length=20, n_agents=10, n_blocks=0, seed=3), 64),
    '12x30_5': (dict(width=12, length=30, n_agents=5, n_blocks=2, seed=6), 64),
    '30x12_5': (dict(width=30, length=12, n_agents=5, n_blocks=2, seed=7), 64),
    '10x10_1': (dict(width=10, length=10, n_agents=1, n_blocks=3, seed=8), 64),
    '64x64_16': (dict(width=64, length=64, n_agents=16, n_blocks=0, seed=11), 4),      # the LDS limit
    'cornered': None,
    'retry': None,
}
# (reserve, retries); 'n' = the droplet count of the case
RULES = [(0, 0), (1, 0), (2, 0), (1, 'n'), (255, 0), (0, 'n')]
FOLLOW_CASES = {
    '10x10_4_2b': dict(width=10, length=10, n_agents=4, n_blocks=2, seed=21, B=128),
    '20x20_10': dict(width=20, length=20, n_agents=10, n_blocks=0, seed=22, B=32),
}


@functools.lru_cache(maxsize=None)
def plan_tasks(name):
    """(width, length, starts, goals, blocks or None)"""
    if name == 'cornered':
        return 10, 10, CORNERED_STARTS, CORNERED_GOALS, None
    if name == 'retry':
        return 20, 20, RETRY_STARTS, RETRY_GOALS, None
    cfg, B = PLAN_CASES[name]
    return (cfg['width'], cfg['length']) + oracle_tasks(B=B, **cfg)


@functools.lru_cache(maxsize=None)
def plan_want(name, reserve, retries):
    from marl_dmfb_amd.plan import plan_reference
    W, L, s, g, b = plan_tasks(name)
    return plan_reference(W, L, s, g, blocks=b, reserve=reserve, retries=retries)


@functools.lru_cache(maxsize=None)
def follow_case(name):
    c = FOLLOW_CASES[name]
    W, L, n, B = c['width'], c['length'], c['n_agents'], c['B']
    s, g, b = oracle_tasks(W, L, n, c['n_blocks'], c['seed'], B=B)
    rng = np.random.default_rng(c['seed'])
    return W, L, s, g, b, rng.uniform(0.6, 1.0, (B, W, L)), rng.random((2 * (W + L), B, n))


@functools.lru_cache(maxsize=None)
def follow_want(name, reserve, retries):
    from marl_dmfb_amd.plan import follow_reference
    W, L, s, g, b, health, uniforms = follow_case(name)
    return follow_reference(W, L, s, g, blocks=b, health=health, uniforms=uniforms, reserve=reserve, retries=retries)


def _rule(rule, n):
    return tuple(n if v == 'n' else v for v in rule)


# ---------------------------------------------------------------------------------------------------- 1. kernel == the rule
@pytest.mark.parametrize('rule', RULES, ids=lambda r: 'R%s_Q%s' % r)
@pytest.mark.parametrize('name', sorted(PLAN_CASES))
def test_planner_equals_the_reference(name, rule):
    from marl_dmfb_amd.plan import Planner
    W, L, s, g, b = plan_tasks(name)
    n = s.shape[1]
    reserve, retries = _rule(rule, n)
    want = plan_want(name, reserve, retries)
    got = Planner(W, L, n, device=DEV, reserve=reserve, retries=retries).plan(s, g, blocks=b)
    equal(got, want)
    if name == 'cornered':
        assert got.success.all() if reserve else not got.success.any()
        if reserve == 1:
            assert got.attempt.tolist() == [0, 0, 0] and got.steps.tolist() == CORNERED_STEPS
    if name == 'retry' and reserve == 0:
        assert got.attempt.tolist() == ([n + 1] if retries else [-1])


def test_the_cases_reach_the_new_paths():
    """What the comparisons run through, read off the reference: reservations that route more, retries that are kept (in a plan
    and in the replans of a closed loop), and a reservation over every level that plans differently from one over the first."""
    n = 10
    assert plan_want('20x20_10', 1, 0).success.sum() > plan_want('20x20_10', 0, 0).success.sum()
    assert (plan_want('20x20_10', 0, n).attempt >= n).sum() >= 2
    assert (plan_want('10x10_4_2b', 0, 4).attempt >= 4).any()
    assert (plan_want('10x10_4_2b', 255, 0).steps != plan_want('10x10_4_2b', 1, 0).steps).any()
    assert any((getattr(follow_want('10x10_4_2b', 0, 4), k) != getattr(follow_want('10x10_4_2b', 0, 0), k)).any()
               for k in ('actions', 'gave_up'))


# ---------------------------------------------------------------------------------------------------- 2. old entry points
def test_the_old_entry_points_are_the_new_ones_at_zero():
    from marl_dmfb_amd import _lib
    lib = _lib.checked('route_plan')
    W, L, s, g, b = plan_tasks('10x10_4_2b')
    B, n, T, nb = s.shape[0], s.shape[1], 2 * (W + L), b.shape[1]
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    ds, dg, db = d(s.astype(np.int32)), d(g.astype(np.int32)), d(b.astype(np.int32))

    def plan_out():     # filled with a pattern no result has, so that every byte must be written alike
        out = [torch.full((B, T + 1, n, 2), 0xAB, dtype=torch.uint8, device=DEV), torch.full((B, T, n), 0x5A, dtype=torch.int8, device=DEV)]
        return out + [torch.full((B,), 77, dtype=dt, device=DEV) for dt in (torch.int32, torch.uint8, torch.int32, torch.int32)]
    old, new = plan_out(), plan_out()
    lib.route_plan_dmfb(B, W, L, n, nb, ds.data_ptr(), dg.data_ptr(), db.data_ptr(), None, *[t.data_ptr() for t in old], None)
    lib.route_plan_dmfb_opt(B, W, L, n, nb, ds.data_ptr(), dg.data_ptr(), db.data_ptr(), None, *[t.data_ptr() for t in new], 0, 0, None)
    torch.cuda.synchronize()
    for a, c in zip(old, new):
        assert torch.equal(a, c)
    want = plan_want('10x10_4_2b', 0, 0)
    np.testing.assert_array_equal(old[0].cpu().numpy(), want.positions)
    np.testing.assert_array_equal(old[4].cpu().numpy(), want.attempt)

    # lock-step 0 of the closed loop from the same start of an episode
    def follow_state():
        pos = torch.zeros((B, T + 1, n, 2), dtype=torch.uint8, device=DEV)
        pos[:, 0] = ds.to(torch.uint8)
        z = lambda shape, dt, v=0: torch.full(shape, v, dtype=dt, device=DEV)
        return dict(positions=pos, route=z((B, T + 1, n, 2), torch.uint8), route_u=z((B, T, n), torch.int8),
                    cursor=z((B,), torch.int32, -1), partial=z((B,), torch.uint8), replans=z((B,), torch.int32),
                    gave_up=z((B,), torch.uint8), active=z((B,), torch.uint8, 1), steps=z((B,), torch.int32),
                    lower=z((B,), torch.int32), actions=z((B, n), torch.int32), u=z((B, T, n), torch.int8, -1))
    names = ('positions', 'route', 'route_u', 'cursor', 'partial', 'replans', 'gave_up', 'active', 'steps', 'lower', 'actions', 'u')
    fo, fn = follow_state(), follow_state()
    lib.route_follow_dmfb(B, W, L, n, nb, 0, dg.data_ptr(), db.data_ptr(), None, *[fo[k].data_ptr() for k in names], None)
    lib.route_follow_dmfb_opt(B, W, L, n, nb, 0, dg.data_ptr(), db.data_ptr(), None, *[fn[k].data_ptr() for k in names], 0, 0, None)
    torch.cuda.synchronize()
    for k in names:
        assert torch.equal(fo[k], fn[k]), k
    routed = want.success
    np.testing.assert_array_equal(fo['replans'].cpu().numpy()[routed], 1)
    np.testing.assert_array_equal(fo['route'].cpu().numpy()[routed], want.positions[routed])
    np.testing.assert_array_equal(fo['lower'].cpu().numpy(), want.lower_bound)


# ---------------------------------------------------------------------------------------------------- 3. the closed loop
@pytest.mark.parametrize('name,rule', [(name, rule) for name in sorted(FOLLOW_CASES) for rule in [(1, 0), (1, 'n')]]
                         + [('10x10_4_2b', (0, 'n'))],      # replans that only retries route
                         ids=lambda v: v if isinstance(v, str) else 'R%s_Q%s' % v)
def test_follow_equals_the_reference_eager_and_captured(name, rule):
    from marl_dmfb_amd.plan import Planner
    W, L, s, g, b, health, uniforms = follow_case(name)
    n = s.shape[1]
    reserve, retries = _rule(rule, n)
    want = follow_want(name, reserve, retries)
    planner = Planner(W, L, n, device=DEV, reserve=reserve, retries=retries)
    follow_helpers.equal(planner.follow(s, g, blocks=b, health=health, uniforms=uniforms), want)
    follow_helpers.equal(planner.follow(s, g, blocks=b, health=health, uniforms=uniforms, use_graph=True), want)
    follow_helpers.equal(planner.follow(s, g, blocks=b, health=health, uniforms=uniforms, use_graph=True), want)      # the replay
    assert (want.constraints == 0).all() and want.success.any() and (want.replans > 1).any()


def test_a_follower_takes_the_rule_from_its_arguments():
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.plan import Follower
    W, L, s, g, b, health, uniforms = follow_case('10x10_4_2b')
    B = len(s)
    env = VecDMFB(W, L, 4, 2, fov=5, n_envs=B, seed=0, with_maps=True, device=DEV)
    env.set_task(s.copy(), g.copy())
    env.set_blocks(b.copy())
    env.set_map('health', health.copy())
    env.restart()
    with pytest.raises(ValueError, match='0 .. 255'):
        Follower(env, reserve=256)
    res = Follower(env, reserve=1, retries=4).play(uniforms=uniforms.copy(), record=False)
    want = follow_want('10x10_4_2b', 1, 4)
    follow_helpers.equal(type(want)(*[getattr(res, k).cpu().numpy() for k in follow_helpers.FIELDS]), want)


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


def test_router_fallbacks_use_the_given_planner():
    from marl_dmfb_amd.plan import Planner
    from marl_dmfb_amd.route import Router, round_stream
    cfg = dict(width=10, length=10, n_agents=4, fov=9)
    s, g, _ = oracle_tasks(**dict(SETS['10x10_4'], B=61))
    s, g = np.concatenate([s, CORNERED_STARTS]), np.concatenate([g, CORNERED_GOALS])
    router = Router(_agents(cfg), name='dmfb', device=DEV, **cfg)
    planner = Planner(10, 10, 4, device=DEV, reserve=1)
    res = router_fallback_substitutes_only_the_failed_tasks(router, planner, s, g, planner=planner)
    assert not Planner(10, 10, 4, device=DEV).plan(s[-3:], g[-3:]).success.any()
    assert res.success[-3:].all()          # the cornered tasks: the policy's or, where it failed them, the reserving planner's
    assert res.steps[-3:][res.source[-3:] == 1].tolist() == [v for v, k in zip(CORNERED_STEPS, res.source[-3:]) if k == 1]

    # fallback='follow': the follower the given planner builds, with its rule
    health = np.random.default_rng(3).uniform(0.6, 1.0, (64, 10, 10))
    policy = ('positions', 'actions', 'steps', 'success', 'constraints', 'try_index')
    before = router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4)
    assert (~before.success).any() and (before.source == 0).all()
    got = router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4, fallback='follow', planner=planner)
    failed = np.nonzero(~before.success)[0]
    fol = planner.follow(s[failed], g[failed], health=health[failed], seed=round_stream(4, 0, 2)[1])
    assert all(f.reserve == 1 and f.retries == 0 for f in planner._followers.values())
    took = np.zeros(64, bool)
    took[failed[fol.success]] = True
    assert took.any()
    np.testing.assert_array_equal(got.source, np.where(took, 2, 0))
    for k in policy:
        np.testing.assert_array_equal(getattr(got, k)[~took], getattr(before, k)[~took], err_msg=k)
    for k in ('positions', 'actions', 'steps', 'success', 'constraints'):
        np.testing.assert_array_equal(getattr(got, k)[took], getattr(fol, k)[fol.success], err_msg=k)
    assert (got.constraints[took] == 0).all() and got.lower_bound is None
