"""Closed-loop planner routing for MEDA on chips up to 128 x 128 on the GPU (marl_dmfb_amd.plan.MedaWideFollower /
MedaWideFollowPlanner.follow, include/meda_follow_wide.h): every field of the closed loop against follow_reference_meda bit for
bit, with the levels of a plan in LDS and in the workspace, against the narrow follower below 65, against the safe plan on
healthy chips, determinism, a masked batch larger than the grid, the HIP env as judge, Router's fallback and the argument checks."""
import numpy as np
import pytest
import torch

import meda_follow_helpers as narrow
from meda_follow_wide_helpers import CASES, FEW_LEVELS, FIELDS, case, equal, reference
from meda_plan_helpers import oracle_tasks
from meda_plan_wide_helpers import WIDE_SETS, set_case
from vdn_helpers import det_init

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_PLANNERS = {}


def _planner(W, L, n, lds_levels=None):
    from marl_dmfb_amd.plan import MedaWideFollowPlanner
    key = (W, L, n, lds_levels)
    if key not in _PLANNERS:
        _PLANNERS[key] = MedaWideFollowPlanner(W, L, n, device=DEV, lds_levels=lds_levels)
    return _PLANNERS[key]


def _follow(name, lds_levels=None, cases=case, **kw):
    c, s, g, health, uniforms = cases(name)
    return _planner(c['width'], c['length'], c['n_agents'], lds_levels).follow(s, g, health=health, uniforms=uniforms,
                                                                                min_health=c.get('min_health', 0.0), **kw)


# ---------------------------------------------------------------------------------------------------- 1. kernel == the loop
@pytest.mark.parametrize('name', sorted(CASES))
def test_wide_follow_equals_the_reference(name):
    got, want = _follow(name), reference(name)
    equal(got, want)
    assert got.reward.dtype == np.float64 and got.reward.shape == want.steps.shape and got.constraints.dtype == np.float64


@pytest.mark.parametrize('lds_levels', [12, 1])
@pytest.mark.parametrize('name', FEW_LEVELS)
def test_the_levels_of_a_plan_in_the_workspace(name, lds_levels):
    """Arrivals beyond the levels kept in LDS: the walk back of every such plan crosses from the workspace into LDS."""
    want = reference(name)
    assert want.steps.max() - 1 > lds_levels
    equal(_follow(name, lds_levels), want)


# ---------------------------------------------------------------------------------------------------- 2. the narrow follower
@pytest.mark.parametrize('name', ['20x64_4', '64x64_16', '15x15_1', '30x30_4_min_health'])
def test_wide_follower_equals_the_narrow_one_below_65(name):
    from marl_dmfb_amd.plan import MedaPlanner
    c, s, g, health, uniforms = narrow.case(name)
    want = MedaPlanner(c['width'], c['length'], c['n_agents'], device=DEV).follow(s, g, health=health, uniforms=uniforms,
                                                                                  min_health=c.get('min_health', 0.0))
    got = _follow(name, cases=narrow.case)
    equal(got, want)
    np.testing.assert_array_equal(got.reward.view(np.int64), want.reward.view(np.int64))
    assert want.success.any() and (want.replans > 1).any()


# ---------------------------------------------------------------------------------------------------- 3. healthy chips
@pytest.mark.parametrize('name', ['20x100_4', '100x20_4'])
def test_on_healthy_chips_the_wide_follower_plays_the_safe_plan(name):
    c = set_case(name)
    W, L, s, g = c['width'], c['length'], c['starts'], c['goals']
    planner = _planner(W, L, s.shape[1])
    plan, res = planner.plan(s, g, safe=True), planner.follow(s, g)
    ok = plan.success
    assert ok.mean() > 0.9
    for k in ('positions', 'actions', 'steps', 'success', 'constraints'):
        np.testing.assert_array_equal(getattr(res, k)[ok], getattr(plan, k)[ok], err_msg=k)
    np.testing.assert_array_equal(res.lower_bound, plan.lower_bound)
    assert (res.replans[ok] == 1).all() and not res.gave_up[ok].any()
    assert ((res.replans[~ok] > 1) | res.gave_up[~ok]).all()
    assert res.positions[..., 0 if L > W else 1].max() >= 64
    # all ones as a health map: the same episodes on a handle with maps
    equal(planner.follow(s, g, health=np.ones((len(s), W, L)), uniforms=np.full((W + L, len(s), s.shape[1]), 0.999)), res)


# ---------------------------------------------------------------------------------------------------- 4. determinism
def test_eager_graph_repeat_and_side_stream_give_the_same_bytes():
    first = _follow('20x72_3')
    equal(first, reference('20x72_3'))
    equal(_follow('20x72_3'), first)
    captured = _follow('20x72_3', use_graph=True)
    equal(captured, first)
    equal(_follow('20x72_3', use_graph=True), first)       # the replay
    np.testing.assert_array_equal(captured.reward.view(np.int64), first.reward.view(np.int64))
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        third = _follow('20x72_3')
    side.synchronize()
    equal(third, first)
    # drawn from a seed instead of given: the same seed, the same episodes
    c, s, g, health, _ = case('20x72_3')
    p = _planner(20, 72, 3)
    a, a2, other = (p.follow(s, g, health=health, seed=k) for k in (5, 5, 6))
    equal(a2, a)
    assert (other.positions != a.positions).any()


# ---------------------------------------------------------------------------------------------------- 5. the chip walk
def test_a_masked_batch_larger_than_the_grid():
    """1032 chips on 512 workgroups, every third chip inactive: a walk that stopped at its first inactive chip would leave the
    chips after it unplayed."""
    from marl_dmfb_amd.env.meda import VecMEDA
    from marl_dmfb_amd.plan import MedaWideFollower
    c, s, g, health, uniforms = (a if isinstance(a, dict) else a.copy() for a in case('20x72_3_many'))
    B, n, T = c['B'], c['n_agents'], c['width'] + c['length']
    env = VecMEDA(c['width'], c['length'], n, fov=19, n_envs=B, seed=0, with_maps=True, device=DEV, version=2)
    env.set_task(s, g)
    env.set_map('health', health)
    env.restart()
    mask = (np.arange(B) % 3 != 1)
    follower = MedaWideFollower(env)
    res = follower.play(uniforms=uniforms, record=False, active=mask.astype(np.uint8))
    host = {k: getattr(res, k).cpu().numpy() for k in FIELDS}
    want = reference('20x72_3_many')
    off = ~mask
    assert off.sum() > 300 and (host['steps'][off] == 0).all() and (host['actions'][off] == -1).all()
    assert (host['replans'][off] == 0).all() and not host['success'][off].any() and not host['gave_up'][off].any()
    for k in FIELDS:
        np.testing.assert_array_equal(host[k][mask], getattr(want, k)[mask], err_msg=k)
    assert (want.steps[mask] > 0).all()
    # the same follower with every chip active: the whole batch
    res = follower.play(uniforms=uniforms, record=False)
    equal(type(want)(*[getattr(res, k).cpu().numpy() for k in FIELDS]), want)


# ---------------------------------------------------------------------------------------------------- 6. the env as judge
def test_the_env_counts_no_failure_and_grants_the_successes():
    from marl_dmfb_amd.env.meda import VecMEDA
    from marl_dmfb_amd.plan import MedaWideFollower
    s, g, health, uniforms = (a.copy() for a in case('80x80_10')[1:])      # torch takes no read-only array
    B, T = len(s), 160
    env = VecMEDA(80, 80, 10, fov=19, n_envs=B, seed=0, with_maps=True, device=DEV)
    env.set_task(s, g)
    env.set_map('health', health)
    env.restart()
    res = MedaWideFollower(env).play(uniforms=uniforms, record=False)
    want = reference('80x80_10')
    host = type(want)(*[getattr(res, k).cpu().numpy() for k in FIELDS])
    equal(host, want)
    assert (host.constraints == 0).all()                       # summed by the env over every step of every chip
    st = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    assert (st['failed'] == 0).all()
    np.testing.assert_array_equal(st['step_count'], want.steps)
    np.testing.assert_array_equal(host.success, (st['status'] == 1).all(axis=1) & (want.steps < T) & ~host.gave_up)
    assert host.success.any() and host.gave_up.any()


# ---------------------------------------------------------------------------------------------------- 7. Router fallback
def test_router_follow_fallback_replaces_only_the_failed_tasks():
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.meda import VecMEDA
    from marl_dmfb_amd.plan import MedaWideFollowPlanner
    from marl_dmfb_amd.route import Router, round_stream
    cfg = dict(width=80, length=80, n_agents=10, fov=19)
    probe = VecMEDA(n_envs=1, device=DEV, **cfg)
    args = make_args(name='meda', drop_num=10, width=80, length=80, fov=19, device=DEV, alg='vdn', **probe.get_env_info())
    agents = Agents(args)
    det_init(agents.policy.eval_rnn, salt=0.25)
    s, g = oracle_tasks(**dict(WIDE_SETS['80x80_10'], B=8))
    health = np.random.default_rng(3).uniform(0.6, 1.0, (8, 80, 80))
    router = Router(agents, name='meda', device=DEV, **cfg)
    planner = _planner(80, 80, 10)
    policy = ('positions', 'actions', 'steps', 'success', 'constraints', 'try_index')
    before = router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4)
    assert (~before.success).any() and (before.source == 0).all()
    with pytest.raises(ValueError, match='planner is for'):
        router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4, fallback='follow',
                     planner=MedaWideFollowPlanner(80, 100, 10, device=DEV))
    res = router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4, fallback='follow', planner=planner)
    after = router.route(s, g, health=health, tries=2, epsilon=0.3, seed=4)
    for k in policy:
        np.testing.assert_array_equal(getattr(after, k), getattr(before, k), err_msg=k)
    failed = np.nonzero(~before.success)[0]
    fol = planner.follow(s[failed], g[failed], health=health[failed], seed=round_stream(4, 0, 2)[1])
    took = np.zeros(8, bool)
    took[failed[fol.success]] = True
    assert took.any() and res.source.dtype == np.int8
    np.testing.assert_array_equal(res.source, np.where(took, 2, 0))
    for k in policy:
        np.testing.assert_array_equal(getattr(res, k)[~took], getattr(before, k)[~took], err_msg=k)
        assert getattr(res, k).dtype == getattr(before, k).dtype
    for k in ('positions', 'actions', 'steps', 'success', 'constraints'):
        np.testing.assert_array_equal(getattr(res, k)[took], getattr(fol, k)[fol.success], err_msg=k)
    assert (res.try_index[took] == -1).all() and res.success[took].all() and res.lower_bound is None


# ---------------------------------------------------------------------------------------------------- 8. argument checks
def test_meda_follow_wide_step_argument_checks():
    from marl_dmfb_amd import _lib
    lib = _lib.meda_follow_wide()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    assert p % 16 == 0
    names = ('goals', 'avoid', 'positions', 'terminated', 'route', 'route_u', 'cursor', 'partial', 'replans', 'gave_up', 'active',
             'steps', 'lower', 'actions', 'u')

    def call(B=1, W=30, L=30, n=4, t=0, work=None, wb=0, levels=0, **ptr):
        a = dict({k: p for k in names}, avoid=None)
        a.update(ptr)
        return lib.meda_follow_wide_step(B, W, L, n, t, *[a[k] for k in names], work, wb, levels, None)

    M = lib.meda_follow_wide_max_dim()
    bad = [call(B=-1), call(W=0), call(L=-3), call(W=4), call(L=4), call(n=0), call(t=-1), call(t=60), call(W=M, L=M, t=2 * M),
           call(positions=p + 1), call(route=p + 1)]
    bad += [call(**{k: None}) for k in names if k != 'avoid']
    assert bad == [-1] * len(bad)
    assert [call(W=M + 1), call(L=M + 1), call(n=17), call(W=M + 1, goals=None)] == [-6, -6, -6, -6]
    # the workspace: 65 x 20 with 8 levels in LDS needs (85 - 2 - 8) * 65 * 16 bytes for its one workgroup
    need = lib.meda_follow_wide_work_bytes(1, 65, 20, 1, 8)
    assert need == 75 * 65 * 16 and lib.meda_follow_wide_work_bytes(1, 65, 20, 1, 0) == 0
    wide = dict(W=65, L=20, n=1, levels=8)
    assert [call(**wide), call(work=p, wb=need - 1, **wide), call(wb=need, **wide), call(work=p + 8, wb=need + 8, **wide),
            call(W=M, L=M, n=16), call(W=M, L=M, n=16, work=p, wb=4096)] == [-1] * 6
    assert call(B=0) == 0 and call(B=0, W=M, L=M, n=16, avoid=p, t=2 * M - 1) == 0 and call(B=0, **wide) == 0
    # a chip whose active byte is 0 is left alone: nothing of the (zeroed) buffers is read further or written, with or without a
    # workspace, at the first lock-step or a later one
    assert call() == 0 and call(t=5) == 0 and call(W=65, L=20, n=1) == 0 and call(work=p, wb=need, **wide) == 0
    assert call(work=p, wb=need, t=84, **wide) == 0
    torch.cuda.synchronize()
    assert int(buf.sum().item()) == 0
    checked = _lib.checked('meda_follow_wide')
    with pytest.raises(NotImplementedError):
        checked.meda_follow_wide_step(1, 129, 30, 4, 0, *[p] * 15, None, 0, 0, None)
    with pytest.raises(ValueError):
        checked.meda_follow_wide_step(1, 30, 30, 4, 60, *[p] * 15, None, 0, 0, None)
    with pytest.raises(ValueError):
        checked.meda_follow_wide_step(1, 65, 20, 1, 0, *[p] * 15, None, 0, 8, None)
