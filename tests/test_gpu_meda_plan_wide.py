"""The wide MEDA planner on the GPU (marl_dmfb_amd.plan.MedaWidePlanner, include/meda_plan_wide.h; chips up to 128 x 128): every
output array against plan_reference_meda bit for bit, plain and safe rule, around the word seam and the row seam, on both sides
of the levels the LDS holds, with more tasks than workgroups; against MedaPlanner below 65; as Router's `planner=`; the limits."""
import numpy as np
import pytest
import torch

from meda_plan_helpers import SETS, equal, judge, oracle_tasks
from meda_plan_wide_helpers import (FORCED_LEVELS, REHOSTED, SEAM_LENGTHS, SEAM_WIDTHS, SERPENTINES, WIDE_SETS, lds_levels, many_tasks_case,
                                    reference, rehosted, seam_case, serpentine_case, set_case, walled_goal_80, workspace_case)
from vdn_helpers import det_init

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RULES = pytest.mark.parametrize('safe', [False, True], ids=['plain', 'safe'])


def _plan(c, safe, lds_levels=None):
    from marl_dmfb_amd.plan import MedaWidePlanner
    planner = MedaWidePlanner(c['width'], c['length'], c['starts'].shape[1], device=DEV, lds_levels=lds_levels)
    return planner.plan(c['starts'], c['goals'], avoid=c['avoid'], safe=safe)


def _both(key, c, safe, lds_levels=None):
    got = _plan(c, safe, lds_levels)
    equal(got, reference(key, c, safe))
    return got


# ---------------------------------------------------------------------------------------------------- 1. kernel == the rule
@RULES
@pytest.mark.parametrize('name', sorted(WIDE_SETS))
def test_wide_planner_equals_the_reference_on_the_oracle_sets(name, safe):
    res = _both(name, set_case(name), safe)
    assert res.success.all()


@RULES
@pytest.mark.parametrize('size,transposed', [(k, False) for k in SEAM_LENGTHS] + [(k, True) for k in SEAM_WIDTHS])
def test_word_seam_row_seam_and_clamp_folds(size, transposed, safe):
    c = seam_case(size, transposed)
    res = _both(('seam', size, transposed), c, safe)
    assert res.success.all() and tuple(res.steps.tolist()) == c['steps']


@RULES
def test_walled_off_goal_beyond_column_and_row_63(safe):
    res = _both('walled_80', walled_goal_80(), safe)
    assert not res.success[0] and res.lower_bound[0] == -1 and res.attempt[0] == -1


@RULES
@pytest.mark.parametrize('axis', [0, 1], ids=['x+64', 'y+64'])
@pytest.mark.parametrize('name', REHOSTED)
def test_hand_cases_in_the_second_word_and_the_second_half_of_the_rows(name, axis, safe):
    _both(('rehosted', name, axis), rehosted(name, axis), safe)


@RULES
@pytest.mark.parametrize('shape', SERPENTINES, ids=lambda s: '%dx%d' % s)
def test_every_side_of_the_lds_workspace_seam(shape, safe):
    """Arrivals at the levels 10 .. 13, 40 .. 42, T-3, T-2 and one past the rule, with as many levels in LDS as fit, with 12 and
    with 41: the same bytes whatever stays in LDS."""
    W, L = shape
    c = serpentine_case(W, L)
    assert lds_levels(W, L, 1) == W + L - 2                                # by default nothing of these chips needs the workspace
    first = _both(('serpentine', W, L), c, safe)
    assert first.steps[:-1].tolist() == [k + 1 for k in c['levels'][:-1]] and not first.success[-1] and first.lower_bound[-1] == -1
    for H in FORCED_LEVELS:
        equal(_plan(c, safe, lds_levels=H), first)


@RULES
def test_the_workspace_without_forcing(safe):
    c = workspace_case()
    res = _both('workspace', c, safe)
    assert tuple(res.steps.tolist()) == c['steps'] and min(c['steps']) - 1 < lds_levels(128, 128, 2) < max(c['steps']) - 1


def test_more_tasks_than_workgroups():
    """max_groups + 3 tasks with 8 levels in LDS: the task loop of a workgroup and the reuse of its workspace slice."""
    from marl_dmfb_amd import _lib
    B = _lib.meda_plan_wide().meda_plan_wide_max_groups() + 3
    c = many_tasks_case(B)
    res = _both('many', c, False, lds_levels=8)
    assert len(res) == B and res.success.all()


# ---------------------------------------------------------------------------------------------------- 2. the narrow planner
@RULES
@pytest.mark.parametrize('name', ['30x30_4', '60x60_16'])
def test_wide_planner_equals_the_narrow_one_below_65(name, safe):
    from marl_dmfb_amd.plan import MedaPlanner, MedaWidePlanner
    c = SETS[name]
    s, g = oracle_tasks(**c)
    narrow = MedaPlanner(c['width'], c['length'], c['n_agents'], device=DEV).plan(s, g, safe=safe)
    equal(MedaWidePlanner(c['width'], c['length'], c['n_agents'], device=DEV).plan(s, g, safe=safe), narrow)
    assert narrow.success.mean() >= 0.9


# ---------------------------------------------------------------------------------------------------- 3. Router
def test_router_takes_the_wide_planner_as_fallback():
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.meda import VecMEDA
    from marl_dmfb_amd.plan import MedaWidePlanner, PlanResult
    from marl_dmfb_amd.route import Router
    c = set_case('80x80_10')
    s, g = c['starts'], c['goals']
    cfg = dict(width=80, length=80, n_agents=10, fov=19)
    probe = VecMEDA(n_envs=1, device=DEV, **cfg)
    args = make_args(name='meda', drop_num=10, width=80, length=80, fov=19, device=DEV, alg='vdn', **probe.get_env_info())
    agents = Agents(args)
    det_init(agents.policy.eval_rnn, salt=0.25)
    router = Router(agents, name='meda', device=DEV, **cfg)
    with pytest.raises(ValueError, match='planner is for'):
        router.route(s, g, fallback='plan', planner=MedaWidePlanner(80, 100, 10, device=DEV))
    res = router.route(s, g, fallback='plan', lower_bound=True, planner=MedaWidePlanner(80, 80, 10, device=DEV))
    ref = reference('80x80_10', c, False)
    np.testing.assert_array_equal(res.lower_bound, ref.lower_bound)
    planned = res.source == 1
    assert planned.any() and res.success[planned].all()              # a random-init policy fails most tasks; the planner none
    for k in ('positions', 'actions', 'steps'):
        np.testing.assert_array_equal(getattr(res, k)[planned], getattr(ref, k)[planned], err_msg=k)
    routes = PlanResult(res.positions, res.actions, res.steps, planned, res.constraints, None, res.lower_bound)
    assert judge(routes, 80, 80, s, g) == int(planned.sum())         # the CPU oracle replays them without a failure


# ---------------------------------------------------------------------------------------------------- 4. limits
def test_limits_of_both_planners():
    from marl_dmfb_amd.plan import MEDA_MAX_DIM, MEDA_WIDE_MAX_DIM, MedaPlanner, MedaWidePlanner
    s = np.array([[[2, 2], [20, 20]]])
    g = np.array([[[12, 12], [27, 5]]])
    for w, l in ((MEDA_WIDE_MAX_DIM + 1, 30), (30, MEDA_WIDE_MAX_DIM + 1)):
        with pytest.raises(NotImplementedError):
            MedaWidePlanner(w, l, 2, device=DEV).plan(s, g)
    many = np.array([[[2 + 7 * i, 2] for i in range(17)]])
    with pytest.raises(NotImplementedError):
        MedaWidePlanner(30, 128, 17, device=DEV).plan(many, many + [0, 20])
    with pytest.raises(NotImplementedError):
        MedaPlanner(MEDA_MAX_DIM + 1, 30, 2, device=DEV).plan(s, g)             # the narrow planner keeps its limit
    assert not hasattr(MedaWidePlanner, 'follow')
    at_limit = MedaWidePlanner(MEDA_WIDE_MAX_DIM, MEDA_WIDE_MAX_DIM, 2, device=DEV).plan(s, g)
    assert at_limit.success.all()
    torch.cuda.synchronize()
