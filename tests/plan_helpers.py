"""Shared by tests/test_plan_host.py and tests/test_gpu_plan.py: task sets drawn by the CPU oracle's own generator, and the
oracle as judge of a planned route.  Shared with the MEDA planner's tests too: `equal` and the Router-fallback check."""
import numpy as np

# The three sets of the planner's tests, 256 tasks each.  The third was meant to be 20x20 / 10 droplets; plan_reference leaves
# 15.2 % of that set unrouted (profiles/plan/NOTES.md), above the 10 % the judge may leave out, so the sparser 30x30 / 10 stands in.
SETS = {
    '10x10_4': dict(width=10, length=10, n_agents=4, n_blocks=0, seed=1),
    '10x10_4_2b': dict(width=10, length=10, n_agents=4, n_blocks=2, seed=2),
    '30x30_10': dict(width=30, length=30, n_agents=10, n_blocks=0, seed=3),
}
MAX_UNROUTED = 0.10
FIELDS = ('positions', 'actions', 'steps', 'success', 'constraints', 'attempt', 'lower_bound')


def equal(got, want, fields=FIELDS):
    for k in fields:
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        np.testing.assert_array_equal(a, b, err_msg=k)


def oracle_tasks(width, length, n_agents, n_blocks=0, seed=0, B=256):
    """(starts, goals, blocks or None) of B tasks as DmfbOracle draws them."""
    from oracle.dmfb_oracle import DmfbOracle
    ora = DmfbOracle(width, length, n_agents, n_blocks, fov=5, n_envs=B, seed=seed)
    ora.reset(new=True)
    s, g = ora.get_task()
    return s, g, (ora.get_blocks().copy() if n_blocks else None)


def judge(res, width, length, s, g, b, stall, health=None, uniforms=None):
    """Plays the routed tasks of `res` through DmfbOracle: the planned positions after every step, no constraint ever, success
    exactly at step `steps` and not before.  Returns the number of tasks played."""
    from oracle.dmfb_oracle import DmfbOracle
    idx = np.nonzero(res.success)[0]
    E, n = len(idx), s.shape[1]
    if E == 0:
        return 0
    ora = DmfbOracle(width, length, n, 0 if b is None else b.shape[1], fov=5, stall=stall, n_envs=E, seed=0,
                     with_maps=health is not None)
    if health is not None:
        ora.set_map('health', health[idx])
    if b is not None:
        ora.set_blocks(b[idx])
    ora.set_task(s[idx], g[idx])
    ora.restart()
    pos, act, steps = res.positions[idx], res.actions[idx], res.steps[idx]
    np.testing.assert_array_equal(ora.get_state()['pos'], pos[:, 0])
    done = steps == 0
    for t in range(int(steps.max())):
        live = t < steps
        a = np.where(live[:, None], act[:, t], 0).astype(np.int32)
        assert (a >= 0).all(), 'action -1 before the end at t=%d' % t
        u = None if health is None else np.full((E, n), uniforms)
        _, _, cons, succ = ora.step(a, u)
        np.testing.assert_array_equal(ora.get_state()['pos'][live], pos[live, t + 1], err_msg='t=%d' % t)
        assert (cons[live] == 0).all(), 'a constraint at t=%d' % t
        ends = live & (steps == t + 1)
        assert (succ[ends] == 1).all(), 'no success at step `steps` (t=%d)' % t
        assert (succ[live & ~ends] == 0).all(), 'success before step `steps` (t=%d)' % t
        done |= ends
    assert done.all()
    assert (ora.get_state()['constraints'] == 0).all()
    return E


def router_fallback_substitutes_only_the_failed_tasks(router, planner, s, g, /, **kw):
    """Router.route before, with and after `fallback='plan'`, and with the bound alone: the planner's routes replace exactly the
    tasks the policy failed and the planner routed, everything else stays the policy's.  `kw` goes to every call that may plan
    (`planner=` for MEDA).  Returns the fallback result."""
    policy = ('positions', 'actions', 'steps', 'success', 'constraints', 'try_index')
    before = router.route(s, g, tries=2, epsilon=0.3, seed=4)
    assert before.lower_bound is None and (before.source == 0).all()
    assert (~before.success).any()                            # a random-init policy fails most tasks
    res = router.route(s, g, tries=2, epsilon=0.3, seed=4, fallback='plan', **kw)
    after = router.route(s, g, tries=2, epsilon=0.3, seed=4, **kw)
    equal(after, before, policy)                              # the handle cache is not disturbed; a planner alone asks nothing
    assert after.lower_bound is None
    plan = planner.plan(s, g)
    pol, pla = res.source == 0, res.source == 1
    assert pla.any() and res.source.dtype == np.int8
    np.testing.assert_array_equal(pla, ~before.success & plan.success)
    for k in policy:
        np.testing.assert_array_equal(getattr(res, k)[pol], getattr(before, k)[pol], err_msg=k)
    for k in ('positions', 'actions', 'steps', 'success', 'constraints'):
        np.testing.assert_array_equal(getattr(res, k)[pla], getattr(plan, k)[pla], err_msg=k)
        assert getattr(res, k).dtype == getattr(before, k).dtype
    assert (res.try_index[pla] == -1).all()
    assert not (~res.success & plan.success).any()
    np.testing.assert_array_equal(res.lower_bound, plan.lower_bound)
    only_bound = router.route(s, g, tries=2, epsilon=0.3, seed=4, lower_bound=True, **kw)
    equal(only_bound, before, policy)
    np.testing.assert_array_equal(only_bound.lower_bound, plan.lower_bound)
    return res
