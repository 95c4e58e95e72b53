"""Shared by tests/test_follow_host.py and tests/test_gpu_follow.py: the cases of the closed-loop router (tasks as the CPU oracle
draws them, a seeded health map and seeded move draws), their follow_reference results computed once per process, and the oracle
as judge of a followed episode.  `build_case` and `build_reference` serve tests/meda_follow_helpers.py too."""
import functools

import numpy as np

from plan_helpers import oracle_tasks

FIELDS = ('positions', 'actions', 'steps', 'success', 'constraints', 'replans', 'gave_up', 'lower_bound')

# name -> chip, tasks, health range, min_health.  `unique`: the batch is that many distinct tasks repeated (the reference is
# computed on the distinct ones; what the large batch is there for is more workgroups than are resident at once).
CASES = {
    '10x10_4_2b': dict(width=10, length=10, n_agents=4, n_blocks=2, seed=21, B=256, low=0.6),
    '20x20_10': dict(width=20, length=20, n_agents=10, n_blocks=0, seed=22, B=64, low=0.6),
    '12x30_5_2b': dict(width=12, length=30, n_agents=5, n_blocks=2, seed=23, B=64, low=0.6),
    '30x12_5_2b': dict(width=30, length=12, n_agents=5, n_blocks=2, seed=24, B=64, low=0.6),
    '10x10_1_3b': dict(width=10, length=10, n_agents=1, n_blocks=3, seed=25, B=128, low=0.6),
    '64x64_16': dict(width=64, length=64, n_agents=16, n_blocks=0, seed=34, B=2, low=0.6),
    '10x10_4_many': dict(width=10, length=10, n_agents=4, n_blocks=0, seed=27, B=4097, unique=241, low=0.6),
    # ten goals and 37 % of the cells below the threshold: a goal is out of reach on every chip, parking routes what it can
    '20x20_10_min_health': dict(width=20, length=20, n_agents=10, n_blocks=0, seed=22, B=64, low=0.2, min_health=0.5),
    '10x10_4_min_health': dict(width=10, length=10, n_agents=4, n_blocks=0, seed=28, B=64, low=0.2, min_health=0.3),
}


def equal(got, want, fields=FIELDS):
    for k in fields:
        a, b = np.asarray(getattr(got, k)), np.asarray(getattr(want, k))
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        np.testing.assert_array_equal(a, b, err_msg=k)


def build_case(c, tasks, T):
    """(starts, goals, blocks or None, health, uniforms) of the case `c` of either env; `tasks(m)` draws m tasks as (starts, goals,
    blocks or None), T is the env's episode limit.  The arrays are shared: do not write to them."""
    W, L, n, B = c['width'], c['length'], c['n_agents'], c['B']
    m = c.get('unique', B)
    s, g, b = tasks(m)
    rng = np.random.default_rng(c['seed'])
    health = rng.uniform(c['low'], 1.0, (m, W, L))
    if 'worn' in c:
        health = np.where(rng.random((m, W, L)) < c['worn'], health, rng.uniform(c['min_health'], 1.0, (m, W, L)))
    uniforms = rng.random((T, m, n))
    if m != B:
        assert B % m == 0
        rep = lambda a, axis=0: None if a is None else np.ascontiguousarray(np.repeat(a, B // m, axis=axis))
        s, g, b, health, uniforms = rep(s), rep(g), rep(b), rep(health), rep(uniforms, 1)
    for a in (s, g, b, health, uniforms):
        if a is not None:
            a.setflags(write=False)
    return s, g, b, health, uniforms


def build_reference(c, s, g, b, health, uniforms, follow):
    """`follow` (follow_reference, or follow_reference_meda behind its signature) on the distinct tasks of a case, repeated as
    the case repeats them."""
    from marl_dmfb_amd.plan import FollowResult
    B, m = c['B'], c.get('unique', c['B'])
    r = B // m
    sub = lambda a, axis=0: None if a is None else np.take(a, np.arange(0, B, r), axis=axis)
    res = follow(c['width'], c['length'], sub(s), sub(g), blocks=sub(b), health=sub(health), min_health=c.get('min_health', 0.0),
                 uniforms=sub(uniforms, 1))
    if r > 1:
        res = FollowResult(*[np.repeat(getattr(res, k), r, axis=0) for k in FIELDS])
    for k in FIELDS:
        getattr(res, k).setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, starts, goals, blocks or None, health, uniforms) of a case; the arrays are shared: do not write to them."""
    c = CASES[name]
    W, L = c['width'], c['length']
    return (c,) + build_case(c, lambda m: oracle_tasks(W, L, c['n_agents'], c['n_blocks'], c['seed'], B=m), 2 * (W + L))


@functools.lru_cache(maxsize=None)
def reference(name):
    """follow_reference of a case, computed once per process."""
    from marl_dmfb_amd.plan import follow_reference
    return build_reference(*case(name), follow_reference)


def judge(res, width, length, s, g, b, health, uniforms, stall=True):
    """Plays the recorded actions of every task through DmfbOracle with the same draws: the recorded positions after every step,
    no constraint at any step on any chip, the success flag at step `steps` and at no other."""
    from oracle.dmfb_oracle import DmfbOracle
    B, n = s.shape[:2]
    ora = DmfbOracle(width, length, n, 0 if b is None else b.shape[1], fov=5, stall=stall, n_envs=B, seed=0,
                     with_maps=health is not None)
    if health is not None:
        ora.set_map('health', health)
    if b is not None:
        ora.set_blocks(b)
    ora.set_task(s, g)
    ora.restart()
    np.testing.assert_array_equal(ora.get_state()['pos'], res.positions[:, 0])
    ended = np.zeros(B, bool)
    for t in range(int(res.steps.max())):
        live = t < res.steps
        assert (res.actions[live, t] >= 0).all(), 'action -1 before the end at t=%d' % t
        # a chip whose episode is over keeps stepping in the oracle (it has no active mask); nothing of it is compared
        a = np.where(live[:, None], res.actions[:, t], 0).astype(np.int32)
        _, _, cons, succ = ora.step(a, None if uniforms is None else uniforms[t])
        np.testing.assert_array_equal(ora.get_state()['pos'][live], res.positions[live, t + 1], err_msg='t=%d' % t)
        assert (cons[live] == 0).all(), 'a constraint at t=%d' % t
        ends = live & (res.steps == t + 1)
        np.testing.assert_array_equal(succ[ends] > 0, res.success[ends], err_msg='success at the last step, t=%d' % t)
        assert (succ[live & ~ends] == 0).all(), 'success before step `steps` (t=%d)' % t
        ended |= ends
    assert (ended | (res.steps == 0)).all()
    assert (res.constraints == 0).all()
    home = (res.positions[:, -1].astype(np.int64) == g).all(axis=(1, 2))
    np.testing.assert_array_equal(res.success, home & (res.steps < 2 * (width + length)) & ~res.gave_up)
