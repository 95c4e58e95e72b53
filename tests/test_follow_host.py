"""The closed-loop rule in numpy (marl_dmfb_amd.plan.follow_reference), no GPU: on healthy chips it is plan_reference, the CPU
oracle judges its episodes on degraded chips, and the parameters do what they say."""
import numpy as np
import pytest

from follow_helpers import case, judge, reference
from plan_helpers import SETS, oracle_tasks

from marl_dmfb_amd.plan import follow_reference, park_order, plan_reference


# ---------------------------------------------------------------------------------------------------- healthy chips
@pytest.mark.parametrize('name', sorted(SETS))
def test_on_healthy_chips_the_follower_is_the_planner(name):
    """Where plan_reference routes a task the follower plays exactly that plan: one plan, never a replan.  Where it fails, the
    follower parks droplets (the plan is partial, so it replans at every step) and either routes the task after all or gives up;
    it gives up at step 0, with the planner's failure result, exactly when no parking routes the starts either."""
    c = SETS[name]
    s, g, b = oracle_tasks(**c)
    W, L = c['width'], c['length']
    plan = plan_reference(W, L, s, g, blocks=b)
    ok = plan.success
    # the failed tasks replan at every step of a long episode: a handful of them shows the relation
    rest = np.nonzero(~ok)[0][:6]
    idx = np.sort(np.concatenate([np.nonzero(ok)[0], rest]))
    sub = lambda a: None if a is None else a[idx]
    res = follow_reference(W, L, sub(s), sub(g), blocks=sub(b), health=np.ones((len(idx), W, L)) if name == '10x10_4' else None)
    ok = ok[idx]
    for k in ('positions', 'actions', 'steps', 'success', 'lower_bound'):
        np.testing.assert_array_equal(getattr(res, k)[ok], getattr(plan, k)[idx][ok], err_msg=k)
    np.testing.assert_array_equal(res.lower_bound, plan.lower_bound[idx])
    assert (res.replans[ok] == 1).all() and not res.gave_up[ok].any() and (res.constraints == 0).all()
    assert len(rest) and ((res.replans[~ok] > 1) | res.gave_up[~ok]).all()
    np.testing.assert_array_equal(res.gave_up[~ok], ~res.success[~ok] & (res.steps[~ok] < 2 * (W + L)))
    at0 = res.gave_up & (res.steps == 0)
    for k in ('positions', 'actions', 'steps', 'success'):      # gave up at once: the planner's failure result
        np.testing.assert_array_equal(getattr(res, k)[at0], getattr(plan, k)[idx][at0], err_msg=k)
    assert (res.replans[at0] == 0).all()
    judge(res, W, L, sub(s), sub(g), sub(b), None, None)


# ---------------------------------------------------------------------------------------------------- the oracle as judge
@pytest.mark.parametrize('name', ['10x10_4_2b', '20x20_10'])
def test_the_oracle_plays_every_followed_episode(name):
    c, s, g, b, health, uniforms = case(name)
    res = reference(name)
    judge(res, c['width'], c['length'], s, g, b, health, uniforms)
    assert res.success.mean() > 0.5
    # every branch of the rule is taken: replans after a failed move, partial plans (a replan at every step), giving up
    assert (res.replans > 1).any() and res.gave_up.any() and _partial(name).any()


def _partial(name):
    """Tasks that replanned although every move of the step before succeeded: only a partial plan does that."""
    c, s, g, b, health, uniforms = case(name)
    res = reference(name)
    B, T = len(res), res.actions.shape[1]
    out = np.zeros(B, bool)
    for i in range(B):
        # with a complete plan, replans <= 1 + the steps at which some droplet failed to move
        p = res.positions[i].astype(int)
        failed = 0
        for t in range(int(res.steps[i])):
            want = p[t] + np.array([(0, 0), (1, 0), (-1, 0), (0, -1), (0, 1)])[res.actions[i, t]]
            failed += bool((want != p[t + 1]).any())
        out[i] = res.replans[i] > 1 + failed
    return out


def test_a_goal_walled_in_gives_up_at_step_0():
    s = np.array([[[0, 0], [9, 9]]])
    g = np.array([[[5, 5], [9, 7]]])
    avoid = np.zeros((1, 10, 10), bool)
    avoid[0, 4:7, 4:7] = True
    avoid[0, 5, 5] = False
    res = follow_reference(10, 10, s, g, avoid=avoid)
    assert res.gave_up[0] and not res.success[0] and res.steps[0] == 0 and res.lower_bound[0] == -1 and res.replans[0] == 0
    assert (res.positions[0] == s[0]).all() and (res.actions == -1).all()
    # the walled droplet is the farther one, so it is never the one parked; were it the nearer, the other would still be routed
    assert park_order([(0, 0), (9, 9)], [(5, 5), (9, 7)]) == [1, 0]
    avoid2 = np.zeros((1, 10, 10), bool)
    avoid2[0, 0, 1] = avoid2[0, 1, 0] = avoid2[0, 1, 1] = True          # droplet 0 cannot leave its corner
    s2 = np.array([[[0, 0], [9, 9]]])
    g2 = np.array([[[0, 2], [0, 9]]])
    res2 = follow_reference(10, 10, s2, g2, avoid=avoid2)
    assert park_order([(0, 0), (9, 9)], [(0, 2), (0, 9)]) == [0, 1]
    # droplet 1 travels with droplet 0 parked until it is as near its goal as droplet 0 is (2 cells; the tie parks the higher
    # index first): from then on droplet 0 is never the one parked, nothing routes it, and the task gives up
    assert res2.lower_bound[0] == -1 and res2.gave_up[0] and not res2.success[0] and res2.steps[0] == 7 and res2.replans[0] == 7
    assert (res2.positions[0, -1, 1] == (2, 9)).all() and (res2.positions[0, :, 0] == (0, 0)).all()


# ---------------------------------------------------------------------------------------------------- other parameters
def test_a_draw_equal_to_the_health_moves():
    s, g = np.array([[[2, 2]]]), np.array([[[5, 2]]])
    health = np.full((1, 10, 10), 0.75)
    u = np.full((40, 1, 1), 0.75)
    res = follow_reference(10, 10, s, g, health=health, uniforms=u)
    assert res.success[0] and res.steps[0] == 3 and res.replans[0] == 1
    res = follow_reference(10, 10, s, g, health=health, uniforms=np.nextafter(u, 1.0))
    assert not res.success[0] and res.steps[0] == 40 and (res.positions[0] == (2, 2)).all()
    assert (res.actions[0, :, 0] == 1).all() and res.replans[0] == 40      # off the plan after every step: replanned every time
    u2 = u.copy()
    u2[0] = 0.8                                   # one failed move: one replan, one step more
    res = follow_reference(10, 10, s, g, health=health, uniforms=u2)
    assert res.success[0] and res.steps[0] == 4 and res.replans[0] == 2


def test_min_health_forbids_exactly_the_cells_below_it():
    c, s, g, b, health, uniforms = case('10x10_4_min_health')
    res = reference('10x10_4_min_health')
    judge(res, 10, 10, s, g, b, health, uniforms)
    assert res.success.any()
    p = res.positions.astype(int)
    B = len(res)
    low = (health < 0.3)[np.arange(B)[:, None, None], p[..., 0], p[..., 1]]          # (B, T+1, n)
    started = low[:, :1]
    moved = np.concatenate([np.zeros_like(low[:, :1]), (p[:, 1:] != p[:, :-1]).any(axis=-1)], axis=1)
    assert started.any()                      # droplets do start on such cells, and leave them
    assert not (low & moved).any()            # none is ever entered
    # the threshold itself is allowed: the same call with `avoid` in place of the health threshold is the same episode
    same = follow_reference(10, 10, s[:8], g[:8], avoid=health[:8] < 0.3, health=health[:8], uniforms=uniforms[:, :8])
    for k in ('positions', 'actions', 'steps', 'replans'):
        np.testing.assert_array_equal(getattr(same, k), getattr(res, k)[:8])
    # and min_health does change the routes
    free = follow_reference(10, 10, s[:8], g[:8], health=health[:8], uniforms=uniforms[:, :8])
    assert (free.positions != res.positions[:8]).any()


def test_stall_off_is_accepted_and_changes_nothing():
    c, s, g, b, health, uniforms = case('10x10_4_2b')
    res = reference('10x10_4_2b')
    off = follow_reference(10, 10, s[:32], g[:32], blocks=b[:32], health=health[:32], uniforms=uniforms[:, :32], stall=False)
    for k in ('positions', 'actions', 'steps', 'success', 'replans', 'gave_up'):
        np.testing.assert_array_equal(getattr(off, k), getattr(res, k)[:32], err_msg=k)
    judge(off, 10, 10, s[:32], g[:32], b[:32], health[:32], uniforms[:, :32], stall=False)


def test_inputs_are_validated():
    s, g = np.array([[[2, 2]]]), np.array([[[5, 2]]])
    with pytest.raises(ValueError, match='uniforms must have shape'):
        follow_reference(10, 10, s, g, uniforms=np.zeros((39, 1, 1)))
    with pytest.raises(ValueError, match='avoid must have shape'):
        follow_reference(10, 10, s, g, avoid=np.zeros((1, 10, 9)))
    empty = follow_reference(10, 10, np.zeros((0, 4, 2), int), np.zeros((0, 4, 2), int))
    assert len(empty) == 0 and empty.positions.shape == (0, 41, 4, 2) and empty.replans.dtype == np.int32


def test_router_refuses_the_follower_for_meda_before_any_launch():
    from marl_dmfb_amd.route import Router
    m = Router(None, name='meda', width=30, length=30, n_agents=4, fov=19, device='cpu')
    ms, mg = np.array([[[2, 2], [27, 27], [2, 27], [27, 2]]]), np.array([[[15, 15], [10, 20], [20, 10], [5, 5]]])
    with pytest.raises(ValueError, match='DMFB only'):
        m.route(ms, mg, fallback='follow')
    assert m.rounds == 0 and not m._slots
