"""Shared by tests/test_meda_plan_host.py and tests/test_gpu_meda_plan.py: task sets drawn by the MEDA CPU oracle's own
generator, denser generated sets, hand-made cases and the oracle as judge of a planned MEDA route."""
import numpy as np

from plan_helpers import FIELDS, MAX_UNROUTED, equal  # noqa: F401  (the same cap and comparison as for DMFB)

# The four oracle sets of the planner's tests.
SETS = {
    '30x30_4': dict(width=30, length=30, n_agents=4, seed=1, B=256),
    '30x60_8': dict(width=30, length=60, n_agents=8, seed=2, B=128),
    '60x60_16': dict(width=60, length=60, n_agents=16, seed=3, B=64),
    '45x45_9': dict(width=45, length=45, n_agents=9, seed=4, B=64),
}
# Denser than the env draws (it keeps starts, and goals, 9 apart): starts pairwise d2 >= 36 and goals pairwise d2 >= 36.
# DENSE is judged by the oracle; the env (and so the oracle) refuses more than (width / 15) * (length / 15) droplets, so
# 30x30 / 6 (DENSER) is a kernel-vs-reference case only, checked for consistency and conflicts in numpy.
DENSE = dict(width=30, length=60, n_agents=8, seed=5, B=128)
DENSER = dict(width=30, length=30, n_agents=6, seed=6, B=128)
DELTA = np.array([(0, -3), (3, 0), (0, 3), (-3, 0), (2, -2), (2, 2), (-2, 2), (-2, -2), (0, 0)])


def oracle_tasks(width, length, n_agents, seed=0, B=256):
    """(starts, goals) of B tasks as MedaOracle draws them: centres (x, y)."""
    from oracle.meda_oracle import MedaOracle
    ora = MedaOracle(width, length, n_agents, fov=19, n_envs=B, seed=seed)
    ora.reset()
    return ora.get_task()


def dense_tasks(width, length, n_agents, seed=0, B=128):
    """Starts pairwise d2 >= 36 and goals pairwise d2 >= 36, by rejection from a seeded generator."""
    rng = np.random.default_rng(seed)

    def draw():
        pts = []
        while len(pts) < n_agents:
            p = (int(rng.integers(2, length - 2)), int(rng.integers(2, width - 2)))
            if all((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 >= 36 for q in pts):
                pts.append(p)
        return pts
    s = np.array([draw() for _ in range(B)], np.int32)
    g = np.array([draw() for _ in range(B)], np.int32)
    return s, g


def box_cells(avoid, centres):
    """bool (...): does the 5x5 box of each centre (x, y) of `centres` (..., 2) touch a set cell of `avoid` (width, length)?"""
    c = np.asarray(centres).astype(int)
    out = np.zeros(c.shape[:-1], bool)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            out |= avoid[c[..., 1] + dy, c[..., 0] + dx]
    return out


def judge(res, width, length, s, g, health=None, uniforms=None):
    """Plays the routed tasks of `res` through MedaOracle: the start centres and the centres after every step are the planned
    ones, fail == 0 at every step, success exactly at step `steps` and not before, every status set at the end.  Returns the
    number of tasks played."""
    from oracle.meda_oracle import MedaOracle
    idx = np.nonzero(res.success)[0]
    E, n = len(idx), s.shape[1]
    if E == 0:
        return 0
    ora = MedaOracle(width, length, n, fov=19, n_envs=E, seed=0, with_maps=health is not None)
    if health is not None:
        ora.set_map('health', health[idx])
    ora.set_task(s[idx], g[idx])
    pos, act, steps = res.positions[idx], res.actions[idx], res.steps[idx]
    np.testing.assert_array_equal(ora.get_state()['pos'], pos[:, 0])
    assert (steps >= 1).all() and (steps <= width + length - 1).all()
    ended = np.zeros(E, bool)
    for t in range(int(steps.max())):
        live = t < steps
        a = np.where(live[:, None], act[:, t], 8).astype(np.int32)
        assert (a >= 0).all(), 'action -1 before the end at t=%d' % t
        u = None if health is None else np.full((E, n), uniforms)
        _, _, fail, succ = ora.step(a, u)
        st = ora.get_state()
        np.testing.assert_array_equal(st['pos'][live], pos[live, t + 1], err_msg='t=%d' % t)
        assert (fail[live] == 0).all(), 'a failure at t=%d' % t
        ends = live & (steps == t + 1)
        assert (succ[ends] == 1).all(), 'no success at step `steps` (t=%d)' % t
        assert (succ[live & ~ends] == 0).all(), 'success before step `steps` (t=%d)' % t
        assert (st['status'][ends] == 1).all(), 'a droplet not done at step `steps` (t=%d)' % t
        assert (st['failed'][live] == 0).all()
        ended |= ends
    assert ended.all()
    return E


def consistent(res, width, length, b=0):
    """positions follow from the actions through move(); 8 once a droplet is inside G; -1 from `steps` on; the last position
    repeated."""
    steps = int(res.steps[b])
    pos, act = res.positions[b].astype(int), res.actions[b]
    assert (act[:steps] >= 0).all() and (act[:steps] <= 8).all() and (act[steps:] == -1).all()
    hi = np.array([length - 3, width - 3])
    goal = pos[-1]
    for t in range(steps):
        in_g = ((pos[t] - goal) ** 2).sum(axis=1) < 16
        want = np.where(in_g[:, None], goal, np.clip(pos[t] + DELTA[act[t]], 2, hi))
        np.testing.assert_array_equal(pos[t + 1], want, err_msg='t=%d' % t)
        assert (act[t][in_g] == 8).all()
    assert (pos[steps:] == pos[steps]).all()


def no_conflict(res, b=0):
    """No pair of centres with d2 < 36 after any step."""
    pos = res.positions[b].astype(int)
    n = pos.shape[1]
    for i in range(n):
        for j in range(i + 1, n):
            assert (((pos[1:, i] - pos[1:, j]) ** 2).sum(axis=1) >= 36).all()


# ---------------------------------------------------------------------------------------------------- hand-made cases
def serpentine(width, length):
    """An avoid mask whose free centres form one corridor winding through the chip: rows 2, 8, 14, ... joined alternately at
    the right and the left end."""
    avoid = np.zeros((width, length), bool)
    rows = list(range(2, width - 2, 6))
    for k, y in enumerate(rows[:-1]):
        avoid[y + 3, :] = True
        if k % 2 == 0:
            avoid[y + 3, length - 5:] = False     # the gap at the right end: centre x = length-3
        else:
            avoid[y + 3, :5] = False              # the gap at the left end: centre x = 2
    return avoid, rows


def first_entry(width, length, start, goal, blocked):
    """Breadth-first search in plain Python, independent of the planner: the first t at which some reachable centre lies in
    G(goal), moving only through centres outside G and never onto a blocked one; None if there is none."""
    frontier, t = {tuple(start)}, 0
    seen_levels = 0
    in_g = lambda c: (c[0] - goal[0]) ** 2 + (c[1] - goal[1]) ** 2 < 16
    visited = set()
    while frontier and seen_levels < 4 * (width + length):
        if any(in_g(c) for c in frontier):
            return t
        nxt = set()
        for c in frontier:
            for dx, dy in DELTA.tolist():
                p = (min(max(c[0] + dx, 2), length - 3), min(max(c[1] + dy, 2), width - 3))
                if not blocked[p[1], p[0]] and p not in visited:
                    nxt.add(p)
        visited |= nxt
        frontier, t, seen_levels = nxt, t + 1, seen_levels + 1
    return None


def hand_cases():
    """name -> dict(width, length, starts (B, n, 2), goals, avoid or None): small cases that exercise the corners of the rule."""
    cases = {}
    # two droplets swapping the ends of a corridor (free centre rows 13 .. 16) with a bay in the middle
    av = np.zeros((1, 30, 30), bool)
    av[0, 10, :] = True
    av[0, 19, :] = True
    cases['corridor_swap'] = dict(width=30, length=30, starts=np.array([[[2, 14], [27, 15]]]), goals=np.array([[[27, 14], [2, 15]]]),
                                  avoid=av)
    av2 = av.copy()
    av2[0, 19, 10:21] = False
    av2[0, 27, :] = True
    cases['corridor_swap_bay'] = dict(width=30, length=30, starts=np.array([[[2, 14], [27, 15]]]),
                                      goals=np.array([[[27, 14], [2, 15]]]), avoid=av2)
    cases['start_in_goal'] = dict(width=30, length=30, starts=np.array([[[10, 10], [20, 20]]]),
                                  goals=np.array([[[12, 12], [20, 23]]]), avoid=None)
    cases['goals_closer_than_6'] = dict(width=30, length=30, starts=np.array([[[2, 2], [27, 27]]]),
                                        goals=np.array([[[15, 15], [18, 19]]]), avoid=None)
    wall = np.zeros((1, 30, 30), bool)
    wall[0, 8, 8:23] = wall[0, 22, 8:23] = True
    wall[0, 8:23, 8] = wall[0, 8:23, 22] = True
    cases['goal_walled_off'] = dict(width=30, length=30, starts=np.array([[[2, 2], [27, 27]]]), goals=np.array([[[15, 15], [27, 2]]]),
                                    avoid=wall)
    # clamped moves: goals in every corner and on every edge, starts 1, 2, 4 or 5 cells short of a multiple of the stride
    s, g = [], []
    for gx, gy in ((2, 2), (27, 2), (2, 27), (27, 27), (2, 15), (27, 15), (15, 2), (15, 27), (2, 3), (26, 27)):
        for sx, sy in ((13, 14), (9, 20), (22, 7), (16, 16), (6, 6), (23, 24)):
            s.append([[sx, sy]])
            g.append([[gx, gy]])
    cases['edges_and_corners'] = dict(width=30, length=30, starts=np.array(s), goals=np.array(g), avoid=None)
    # the same against the far edge of a 64-wide word and a non-square chip
    cases['edges_64'] = dict(width=20, length=64, starts=np.array([[[30, 9]], [[33, 10]], [[5, 5]], [[58, 14]]]),
                             goals=np.array([[[61, 2]], [[2, 17]], [[61, 17]], [[61, 17]]]), avoid=None)
    # a ring three centres wide along the border (everything inside is avoided): the moves there are clamped ones
    ring = np.zeros((1, 30, 30), bool)
    ring[0, 7:23, 7:23] = True
    pts = [(2, 2), (27, 27), (3, 26), (26, 3), (4, 14), (25, 15), (14, 4), (15, 25), (27, 2), (2, 27)]
    s = [[[a, b]] for (a, b) in pts for _ in range(3)]
    g = [[list(pts[(k + j) % len(pts)])] for k in range(len(pts)) for j in (3, 5, 7)]
    cases['ring'] = dict(width=30, length=30, starts=np.array(s), goals=np.array(g), avoid=np.repeat(ring, len(s), 0))
    ring64 = np.zeros((1, 20, 64), bool)
    ring64[0, 7:13, 7:57] = True
    pts = [(2, 2), (61, 17), (3, 16), (60, 3), (61, 2), (2, 17), (31, 3), (32, 16)]
    s = [[[a, b]] for (a, b) in pts for _ in range(3)]
    g = [[list(pts[(k + j) % len(pts)])] for k in range(len(pts)) for j in (1, 3, 5)]
    cases['ring_64'] = dict(width=20, length=64, starts=np.array(s), goals=np.array(g), avoid=np.repeat(ring64, len(s), 0))
    # two droplets in the ring, heading past each other
    cases['ring_pair'] = dict(width=30, length=30, starts=np.array([[[2, 2], [27, 27]], [[3, 26], [26, 3]]]),
                              goals=np.array([[[27, 27], [2, 2]], [[26, 3], [3, 26]]]), avoid=np.repeat(ring, 2, 0))
    return cases
