"""The MEDA space-time planner on the GPU (marl_dmfb_amd.plan.MedaPlanner, include/meda_plan.h): every output array against
plan_reference_meda bit for bit, the HIP env as judge of the planned routes, the size limit, Router's `planner=` and determinism."""
import numpy as np
import pytest
import torch

from meda_plan_helpers import DENSE, DENSER, SETS, dense_tasks, equal, hand_cases, oracle_tasks, serpentine
from plan_helpers import router_fallback_substitutes_only_the_failed_tasks
from vdn_helpers import det_init

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _both(width, length, s, g, avoid=None, health=None):
    from marl_dmfb_amd.plan import MedaPlanner, plan_reference_meda
    got = MedaPlanner(width, length, s.shape[1], device=DEV).plan(s, g, avoid=avoid, health=health)
    want = plan_reference_meda(width, length, s, g, avoid=avoid, health=health)
    equal(got, want)
    return got


# ---------------------------------------------------------------------------------------------------- 1. kernel == the rule
@pytest.mark.parametrize('name', sorted(SETS))
def test_planner_equals_the_reference_on_the_oracle_sets(name):
    c = SETS[name]
    s, g = oracle_tasks(**c)
    res = _both(c['width'], c['length'], s, g)
    assert res.success.mean() >= 0.9


@pytest.mark.parametrize('cfg', [DENSE, DENSER], ids=['30x60_8', '30x30_6'])
def test_planner_equals_the_reference_on_the_denser_sets(cfg):
    s, g = dense_tasks(**cfg)
    res = _both(cfg['width'], cfg['length'], s, g)
    assert (res.attempt > 0).any() and (~res.success).any() and res.success.mean() > 0.5


@pytest.mark.parametrize('name', sorted(hand_cases()))
def test_planner_equals_the_reference_on_the_hand_cases(name):
    c = hand_cases()[name]
    _both(c['width'], c['length'], c['starts'], c['goals'], avoid=c['avoid'])


def test_planner_equals_the_reference_at_the_step_limit():
    """The winding corridor of the host test: goals along its end, entered around level T-2."""
    W = L = 40
    avoid, rows = serpentine(W, L)
    goals = [(gx, gy) for gy in (rows[-1], W - 3) for gx in (2, 3, 4, 5, 6, 8, 11, 20)]
    s = np.array([[(2, 2)]] * len(goals))
    g = np.array([[q] for q in goals])
    res = _both(W, L, s, g, avoid=np.repeat(avoid[None], len(goals), 0))
    assert res.success.any() and (res.steps.max() >= W + L - 3)


@pytest.mark.parametrize('cfg', [
    dict(width=64, length=64, n_agents=16, seed=21, B=16),     # the size limit itself
    dict(width=30, length=60, n_agents=8, seed=22, B=64),      # non-square, both ways
    dict(width=60, length=30, n_agents=8, seed=23, B=64),
    dict(width=64, length=20, n_agents=4, seed=24, B=64),
    dict(width=30, length=30, n_agents=1, seed=25, B=64),
    dict(width=30, length=30, n_agents=4, seed=26, B=1),       # batch sizes 1 and 4096
    dict(width=30, length=30, n_agents=4, seed=27, B=4096),
])
def test_planner_equals_the_reference_on_other_shapes(cfg):
    s, g = oracle_tasks(**cfg)
    res = _both(cfg['width'], cfg['length'], s, g)
    assert res.success.mean() >= 0.9
    if cfg['n_agents'] == 1:
        np.testing.assert_array_equal(res.steps, res.lower_bound)


def test_avoid_mask_and_health():
    c = SETS['30x60_8']
    s, g = oracle_tasks(**c)
    B = len(s)
    rng = np.random.default_rng(0)
    avoid = rng.random((B, 30, 60)) < 0.004
    health = np.where(rng.random((B, 30, 60)) < 0.003, 0.5, 1.0)
    for kw in (dict(avoid=avoid), dict(health=health), dict(avoid=avoid.astype(np.uint8) * 7, health=health)):
        res = _both(30, 60, s, g, **kw)
        assert res.success.any() and ('health' not in kw or (~res.success).any())    # starts on degraded boxes are refused
    dense = rng.random((B, 30, 60)) < 0.02
    res = _both(30, 60, s, g, avoid=dense)
    assert (res.lower_bound < 0).any()


# ---------------------------------------------------------------------------------------------------- 2. the HIP env as judge
@pytest.mark.parametrize('name', ['30x30_4', '30x60_8'])
def test_hip_env_follows_the_plan(name):
    from marl_dmfb_amd.env.meda import VecMEDA
    from marl_dmfb_amd.plan import MedaPlanner
    c = SETS[name]
    W, L, n = c['width'], c['length'], c['n_agents']
    s, g = oracle_tasks(**c)
    res = MedaPlanner(W, L, n, device=DEV).plan(s, g)
    B = len(res)
    routed = res.success
    assert routed.mean() >= 0.9
    env = VecMEDA(W, L, n, fov=19, n_envs=B, seed=0, device=DEV)
    env.set_task(s, g)
    env.restart()
    np.testing.assert_array_equal(env.get_state()['pos'].cpu().numpy(), res.positions[:, 0])
    failed = np.zeros(B, bool)
    for t in range(int(res.steps.max())):
        live = routed & (t < res.steps)
        a = np.where(live[:, None], res.actions[:, t], 8).astype(np.int32)
        _, _, _, info = env.step(torch.as_tensor(a, device=DEV), active=torch.as_tensor(live.astype(np.uint8), device=DEV))
        pos = env.get_state()['pos'].cpu().numpy()
        np.testing.assert_array_equal(pos[live], res.positions[live, t + 1], err_msg='t=%d' % t)
        failed |= live & (info['constraints'].cpu().numpy() != 0)
        succ = info['success'].cpu().numpy() > 0
        ends = live & (res.steps == t + 1)
        assert succ[ends].all() and not succ[live & ~ends].any(), 't=%d' % t
    assert not failed.any()
    assert (env.get_state()['failed'].cpu().numpy()[routed] == 0).all()


# ---------------------------------------------------------------------------------------------------- 3. size limit
def test_one_past_the_size_limit_is_refused():
    from marl_dmfb_amd import _lib
    from marl_dmfb_amd.plan import MEDA_MAX_DIM, MedaPlanner
    assert _lib.meda_plan().meda_plan_max_dim() == MEDA_MAX_DIM
    s = np.array([[[2, 2], [20, 20]]])
    g = np.array([[[12, 12], [27, 5]]])
    for w, l in ((MEDA_MAX_DIM + 1, 30), (30, MEDA_MAX_DIM + 1)):
        with pytest.raises(NotImplementedError):
            MedaPlanner(w, l, 2, device=DEV).plan(s, g)
    assert MedaPlanner(MEDA_MAX_DIM, MEDA_MAX_DIM, 2, device=DEV).plan(s, g).success.all()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 4. Router
def test_router_takes_a_meda_planner_as_fallback():
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.meda import VecMEDA
    from marl_dmfb_amd.plan import MedaPlanner
    from marl_dmfb_amd.route import Router
    cfg = dict(width=30, length=30, n_agents=4, fov=19)
    probe = VecMEDA(n_envs=1, device=DEV, **cfg)
    args = make_args(name='meda', drop_num=4, width=30, length=30, fov=19, device=DEV, alg='vdn', **probe.get_env_info())
    agents = Agents(args)
    det_init(agents.policy.eval_rnn, salt=0.25)
    s, g = oracle_tasks(**SETS['30x30_4'])
    router = Router(agents, name='meda', device=DEV, **cfg)
    planner = MedaPlanner(30, 30, 4, device=DEV)
    with pytest.raises(ValueError, match='planner is for'):
        router.route(s, g, fallback='plan', planner=MedaPlanner(30, 60, 4, device=DEV))
    router_fallback_substitutes_only_the_failed_tasks(router, planner, s, g, planner=planner)


# ---------------------------------------------------------------------------------------------------- 5. determinism
def test_two_calls_and_a_side_stream_give_the_same_bytes():
    from marl_dmfb_amd.plan import MedaPlanner
    c = SETS['30x60_8']
    s, g = oracle_tasks(**c)
    planner = MedaPlanner(30, 60, 8, device=DEV)
    first = planner.plan(s, g)
    equal(planner.plan(s, g), first)
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        third = planner.plan(s, g)
    side.synchronize()
    equal(third, first)
