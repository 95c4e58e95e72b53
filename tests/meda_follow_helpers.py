"""Shared by tests/test_meda_follow_host.py and tests/test_gpu_meda_follow.py: the cases of the MEDA closed-loop router (tasks as
the CPU oracle draws them, a seeded health map and seeded move draws), their follow_reference_meda results computed once per
process, the oracle as judge of a followed episode and the failure-safety property of a plan in numpy."""
import functools

import numpy as np

from follow_helpers import FIELDS, build_case, build_reference, equal  # noqa: F401  (all as for DMFB)
from meda_plan_helpers import DELTA, oracle_tasks

# name -> chip, tasks, health range, min_health.  `unique`: the batch is that many distinct tasks repeated (the reference is
# computed on the distinct ones; what the large batch is there for is more workgroups than are resident at once).
# 20x64 / 4 puts bit 61 and the east clamp at the far edge of the row word, 15x15 / 1 is the smallest chip the env takes,
# 64x64 / 16 is the LDS limit, the two min_health cases force parking.
CASES = {
    '30x30_4': dict(width=30, length=30, n_agents=4, seed=41, B=128, low=0.6),
    '30x60_8': dict(width=30, length=60, n_agents=8, seed=42, B=32, low=0.6),
    '60x30_8': dict(width=60, length=30, n_agents=8, seed=43, B=32, low=0.6),
    '20x64_4': dict(width=20, length=64, n_agents=4, seed=44, B=32, low=0.6),
    '15x15_1': dict(width=15, length=15, n_agents=1, seed=45, B=64, low=0.6),
    '64x64_16': dict(width=64, length=64, n_agents=16, seed=46, B=2, low=0.6),
    '30x30_4_many': dict(width=30, length=30, n_agents=4, seed=47, B=4097, unique=241, low=0.6),
    # A centre is blocked if ANY of the 25 cells under it is below min_health.  With every cell drawn from 0.2 .. 1, 7 in 8 are
    # below 0.9, no centre of any chip is free and the reference gives up on every task at step 0 (measured: 64 of 64 and 32 of
    # 32).  So here only a share `worn` of the cells is drawn from 0.2 .. 1 and the others from 0.9 .. 1: about a third of the
    # centres are blocked, which is where goals get out of reach and parking has work to do.
    '30x30_4_min_health': dict(width=30, length=30, n_agents=4, seed=48, B=64, low=0.2, min_health=0.9, worn=0.02),
    '30x60_8_min_health': dict(width=30, length=60, n_agents=8, seed=49, B=32, low=0.2, min_health=0.9, worn=0.02),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, starts, goals, health, uniforms) of a case; the arrays are shared: do not write to them."""
    c = CASES[name]
    W, L = c['width'], c['length']
    s, g, _, health, uniforms = build_case(c, lambda m: (*oracle_tasks(W, L, c['n_agents'], c['seed'], B=m), None), W + L)
    return c, s, g, health, uniforms


@functools.lru_cache(maxsize=None)
def reference(name):
    """follow_reference_meda of a case, computed once per process."""
    from marl_dmfb_amd.plan import follow_reference_meda
    c, s, g, health, uniforms = case(name)
    return build_reference(c, s, g, None, health, uniforms, lambda W, L, s, g, blocks, **kw: follow_reference_meda(W, L, s, g, **kw))


def partial_plans(res, width, length, g):
    """bool (B,): tasks that replanned although every move of the step before succeeded: only a partial plan does that."""
    hi = np.array([length - 3, width - 3])
    out = np.zeros(len(res), bool)
    for b in range(len(res)):
        p, goal = res.positions[b].astype(int), g[b].astype(int)
        failed = 0
        for t in range(int(res.steps[b])):
            in_g = ((p[t] - goal) ** 2).sum(axis=1) < 16
            want = np.where(in_g[:, None], p[t + 1], np.clip(p[t] + DELTA[res.actions[b, t]], 2, hi))
            failed += bool((want != p[t + 1]).any())
        out[b] = res.replans[b] > 1 + failed      # with a complete plan, replans <= 1 + the steps at which some move failed
    return out


def judge(res, width, length, s, g, health, uniforms):
    """Plays the recorded actions of every task through MedaOracle with the same draws: the recorded centres after every step,
    fail == 0 at every step of every chip, failed == 0, the success flag at step `steps` on exactly the chips flagged and at no
    other step, constraints == 0 everywhere."""
    from oracle.meda_oracle import MedaOracle
    B, n = s.shape[:2]
    T = width + length
    ora = MedaOracle(width, length, n, fov=19, n_envs=B, seed=0, with_maps=health is not None)
    if health is not None:
        ora.set_map('health', health)
    ora.set_task(s, g)
    np.testing.assert_array_equal(ora.get_state()['pos'], res.positions[:, 0])
    ended = np.zeros(B, bool)
    for t in range(int(res.steps.max())):
        live = t < res.steps
        assert (res.actions[live, t] >= 0).all(), 'action -1 before the end at t=%d' % t
        # a chip whose episode is over keeps stepping in the oracle (it has no active mask); nothing of it is compared
        a = np.where(live[:, None], res.actions[:, t], 8).astype(np.int32)
        _, _, fail, succ = ora.step(a, None if uniforms is None else uniforms[t])
        st = ora.get_state()
        np.testing.assert_array_equal(st['pos'][live], res.positions[live, t + 1], err_msg='t=%d' % t)
        assert (fail[live] == 0).all(), 'a failure at t=%d' % t
        assert (st['failed'][live] == 0).all()
        ends = live & (res.steps == t + 1)
        np.testing.assert_array_equal(succ[ends] > 0, res.success[ends], err_msg='success at the last step, t=%d' % t)
        assert (succ[live & ~ends] == 0).all(), 'success before step `steps` (t=%d)' % t
        # an episode ends with every droplet done, at the step limit, or where the follower gave up
        done = (st['status'][ends] == 1).all(axis=1)
        np.testing.assert_array_equal(done | (res.steps[ends] == T) | res.gave_up[ends], np.ones(ends.sum(), bool))
        np.testing.assert_array_equal(res.success[ends], done & (res.steps[ends] < T) & ~res.gave_up[ends])
        ended |= ends
    assert (ended | (res.steps == 0)).all()
    assert not res.success[res.steps == 0].any()
    assert (res.constraints == 0).all() and res.constraints.dtype == np.float64


def parking_never_takes_a_droplet_inside_its_disc(res, g):
    """At every recorded state of every chip, park_order_meda lists exactly the droplets with d2(centre, goal) >= 16, by ascending
    d2 and then descending index; and a droplet that stands inside its disc, not yet done, is on its goal one step later (the env
    snapped it, whatever the plan of that step was).  Returns how many such droplets were seen."""
    from marl_dmfb_amd.plan import park_order_meda
    seen = 0
    for b in range(len(res)):
        p, goal = res.positions[b].astype(int), g[b].astype(int)
        for t in range(int(res.steps[b])):
            d2 = ((p[t] - goal) ** 2).sum(axis=1)
            order = park_order_meda([tuple(q) for q in p[t].tolist()], [tuple(q) for q in goal.tolist()])
            assert sorted(order) == [i for i in range(len(d2)) if d2[i] >= 16]
            assert [(d2[i], -i) for i in order] == sorted((d2[i], -i) for i in order)
            inside = (d2 < 16) & (d2 > 0)
            assert (p[t + 1][inside] == goal[inside]).all() and (res.actions[b, t][inside] == 8).all()
            seen += int(inside.sum())
    return seen


def failure_safe(res, b=0):
    """The safety property of the plan of task b: for every step t -> t + 1 and every pair (i, j), the combinations of (moved,
    stayed) all leave d2 >= 36, except for the pair of positions at level 0 (where the chip starts is not the plan's doing).
    The one combination that cannot happen is left out: a droplet inside its goal disc at level t is snapped onto its goal by the
    env without a draw, so it never stays on the cell it leaves (the rule guards that cell for no one).  Returns the smallest d2
    seen (2 ** 30 if the plan has a single droplet)."""
    steps = int(res.steps[b])
    pos = res.positions[b].astype(int)
    n = pos.shape[1]
    goal = pos[-1]
    certain = ((pos - goal) ** 2).sum(axis=-1) < 16         # (T+1, n): the step from this level cannot fail
    low = 1 << 30
    for t in range(steps):
        for i in range(n):
            for j in range(i + 1, n):
                for mi in (0, 1):
                    for mj in (0, 1):
                        if (t == 0 and not mi and not mj) or (not mi and certain[t, i]) or (not mj and certain[t, j]):
                            continue
                        low = min(low, int(((pos[t + mi, i] - pos[t + mj, j]) ** 2).sum()))
    return low
