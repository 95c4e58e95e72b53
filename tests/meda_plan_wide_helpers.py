"""Shared by tests/test_meda_plan_wide_host.py and tests/test_gpu_meda_plan_wide.py: the task sets and hand cases of the wide MEDA
planner (chips up to 128 x 128) and their plan_reference_meda results, each computed once per process."""
import functools

import numpy as np

from meda_plan_helpers import first_entry, hand_cases, oracle_tasks, serpentine

LDS_BUDGET = 160 * 1024 - 1024      # marl_dmfb_amd/csrc/plan_core.h: kLdsBudget

# Oracle-drawn sets above 64 rows or columns; the reference routes every task of them.
WIDE_SETS = {
    '80x80_10': dict(width=80, length=80, n_agents=10, seed=11, B=24),
    '128x128_16': dict(width=128, length=128, n_agents=16, seed=12, B=6),
    '65x65_9': dict(width=65, length=65, n_agents=9, seed=13, B=16),
    '20x100_4': dict(width=20, length=100, n_agents=4, seed=14, B=16),
    '100x20_4': dict(width=100, length=20, n_agents=4, seed=15, B=16),
}


def case(width, length, starts, goals, avoid=None):
    return dict(width=width, length=length, starts=np.asarray(starts), goals=np.asarray(goals), avoid=avoid)


@functools.lru_cache(maxsize=None)
def set_case(name):
    c = WIDE_SETS[name]
    s, g = oracle_tasks(**c)
    return case(c['width'], c['length'], s, g)


def lds_levels(w, l, n):
    """H of include/meda_plan_wide.h, written out: what the budget holds beside the paths and the avoid rows."""
    paths = ((w + l + 1) * n * 2 + 15) // 16 * 16
    return min(w + l - 2, (LDS_BUDGET - paths - 16 * w) // (16 * w))


# ---------------------------------------------------------------------------------------------------- word seam and clamp folds
# size -> the steps plan_reference_meda gives for the three tasks of seam_case (plain and safe rule alike).  The third task crosses the
# whole chip: 121 or 122 columns at three a step from x = L-4 is arrival 41, steps 42, along either axis.
SEAM_LENGTHS = {65: (3, 3, 21), 66: (3, 3, 21), 67: (3, 3, 22), 68: (3, 4, 22), 127: (3, 23, 42), 128: (3, 23, 42)}
SEAM_WIDTHS = {65: (3, 3, 21), 66: (3, 3, 21), 67: (3, 3, 22), 128: (3, 23, 42)}


def seam_case(size, transposed):
    """Three one-droplet tasks around the word seam (columns 63 / 64) and the far clamp of a chip 20 wide and `size` long; or,
    transposed, around the row seam of a chip `size` wide and 20 long."""
    L = size
    tasks = (((L - 9, 9), (L - 3, 2)), ((60, 9), (L - 3, 17)), ((L - 4, 9), (2, 17)))
    if transposed:
        tasks = tuple(((s[1], s[0]), (g[1], g[0])) for s, g in tasks)
    c = case(size if transposed else 20, 20 if transposed else size, [[s] for s, _ in tasks], [[g] for _, g in tasks])
    c['steps'] = (SEAM_WIDTHS if transposed else SEAM_LENGTHS)[size]
    return c


# ---------------------------------------------------------------------------------------------------- avoid maps beyond 63
def walled_goal_80():
    """The walled-off goal of hand_cases() on 80x80 with the walls at rows / columns 58 and 72 around the goal (65, 65)."""
    wall = np.zeros((1, 80, 80), bool)
    wall[0, 58, 58:73] = wall[0, 72, 58:73] = True
    wall[0, 58:73, 58] = wall[0, 58:73, 72] = True
    return case(80, 80, [[[2, 2], [77, 77]]], [[[65, 65], [77, 2]]], wall)


def rehosted(name, axis):
    """hand_cases()[name] moved by +64 along x (axis 0: onto a chip 128 long) or along y (axis 1: onto a chip 128 wide): every
    cell outside the moved chip is avoided, so the whole case plays in the second word, or in the second half of the rows (the
    clamps of the near edge become avoided cells; those of the far edge stay clamps where the moved chip ends at 128)."""
    c = hand_cases()[name]
    W, L, B = c['width'], c['length'], len(c['starts'])
    off = np.array([64, 0] if axis == 0 else [0, 64])
    W2, L2 = (W, 128) if axis == 0 else (128, L)
    assert (L if axis == 0 else W) <= 64
    avoid = np.ones((B, W2, L2), bool)
    home = np.zeros((B, W, L), bool) if c['avoid'] is None else np.asarray(c['avoid']) != 0
    if axis == 0:
        avoid[:, :, 64:64 + L] = home
    else:
        avoid[:, 64:64 + W, :] = home
    return case(W2, L2, c['starts'] + off, c['goals'] + off, avoid)


REHOSTED = sorted(hand_cases())


# ---------------------------------------------------------------------------------------------------- every arrival level
SERPENTINES = ((32, 70), (70, 32), (26, 100))
FORCED_LEVELS = (12, 41)


def _entry_levels(W, L, blocked, start):
    """level -> the lowest free goal (y, x) whose disc d2 < 16 is first entered at that level from `start` (None: never)."""
    dist = np.full((W, L), -1)
    frontier, t = [start], 0
    dist[start[1], start[0]] = 0
    deltas = ((0, -3), (3, 0), (0, 3), (-3, 0), (2, -2), (2, 2), (-2, 2), (-2, -2))
    while frontier:
        nxt = []
        for x, y in frontier:
            for dx, dy in deltas:
                px, py = min(max(x + dx, 2), L - 3), min(max(y + dy, 2), W - 3)
                if not blocked[py, px] and dist[py, px] < 0:
                    dist[py, px] = t + 1
                    nxt.append((px, py))
        frontier, t = nxt, t + 1
    disc = [(dx, dy) for dy in range(-3, 4) for dx in range(-3, 4) if dx * dx + dy * dy < 16]
    entry = {}
    for gy in range(2, W - 2):
        for gx in range(2, L - 2):
            if blocked[gy, gx]:
                continue
            near = [dist[gy + dy, gx + dx] for dx, dy in disc if 0 <= gy + dy < W and 0 <= gx + dx < L]
            near = [d for d in near if d >= 0]
            entry.setdefault(min(near) if near else None, (gx, gy))
    return entry


@functools.lru_cache(maxsize=None)
def serpentine_case(W, L):
    """One droplet from (2, 2) through the winding corridor to goals entered at the levels 10 .. 13, 40 .. 42, T-3, T-2 and T-1.
    An arrival at level a stores the levels 0 .. a-1, so with H = 12 or 41 levels in LDS the arrivals at H and H + 1 are the last
    that stay in LDS and the first that reach the workspace; T-1 is one more than the rule allows.
    c['levels']: those levels; c['all_levels']: every entry level that exists on the chip."""
    from marl_dmfb_amd.plan import _meda_blocked
    T = W + L
    avoid, _ = serpentine(W, L)
    blocked = _meda_blocked(W, L, avoid)
    entry = _entry_levels(W, L, blocked, (2, 2))
    levels = (10, 11, 12, 13, 40, 41, 42, T - 3, T - 2, T - 1)
    goals = [entry[k] for k in levels]
    for k, g in zip(levels, goals):      # the independent search of meda_plan_helpers agrees
        assert first_entry(W, L, (2, 2), g, blocked) == k, (W, L, k, g)
    c = case(W, L, [[(2, 2)]] * len(goals), [[g] for g in goals], np.repeat(avoid[None], len(goals), 0))
    c['levels'], c['all_levels'] = levels, sorted(k for k in entry if k is not None)
    return c


def workspace_case():
    """128x128, the winding corridor, two droplets: droplet 0 arrives on both sides of the H (about 74) levels the LDS holds."""
    avoid, rows = serpentine(128, 128)
    goals0 = ((125, rows[2]), (60, rows[1]), (125, rows[4]))
    c = case(128, 128, [[(2, 2), (125, rows[-1])]] * 3, [[g, (2, rows[-1])] for g in goals0], np.repeat(avoid[None], 3, 0))
    c['steps'] = (127, 65, 213)
    return c


def many_tasks_case(B):
    """B one-droplet tasks on 65x20, starts and goals as distinct as the 61 * 16 centres allow."""
    cells = [(x, y) for y in range(2, 63) for x in range(2, 18)]
    k = np.arange(B)
    s = np.array([cells[i % len(cells)] for i in k])
    g = np.array([cells[(i * 37 + 500) % len(cells)] for i in k])
    return case(65, 20, s[:, None], g[:, None])


# ---------------------------------------------------------------------------------------------------- the reference, once
_REF = {}


def reference(key, c, safe):
    """plan_reference_meda of the case `c`, kept under (key, safe) for the tests of one process; never changed by them."""
    from marl_dmfb_amd.plan import plan_reference_meda
    if (key, safe) not in _REF:
        res = plan_reference_meda(c['width'], c['length'], c['starts'], c['goals'], avoid=c['avoid'], safe=safe)
        for k in ('positions', 'actions', 'steps', 'success', 'constraints', 'attempt', 'lower_bound'):
            getattr(res, k).setflags(write=False)
        _REF[(key, safe)] = res
    return _REF[(key, safe)]
