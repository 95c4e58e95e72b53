"""A deterministic prioritized space-time planner for DMFB: the classical baseline to hold a learned policy against, and the
fallback of marl_dmfb_amd.route.Router for the tasks the policy fails.

    res = Planner(width=20, length=20, n_agents=10).plan(starts, goals, blocks=None, avoid=None, health=None)
    ref = plan_reference(20, 20, starts, goals)          # the same rule in plain numpy, no GPU

The rule ("Space-time planner").  Cells (x, y), 0 <= x < width, 0 <= y < length; actions 0 STALL, 1 RIGHT (+1, 0),
2 LEFT (-1, 0), 3 DOWN (0, -1), 4 UP (0, +1), as the env; T = 2 * (width + length), the episode limit.  near(p) is the 3x3 box
around p, where the env counts a static or a dynamic conflict.  A cell is blocked if it lies in a block or in `avoid`.

Priority: droplets by descending Manhattan distance start -> goal, ties by ascending index; attempt k = 0 .. n-1 plans them in
that order rotated left by k, and the first attempt in which every droplet gets a path wins.

One droplet against the paths pos_q[t] (t = 0 .. T; a planned droplet stays on its goal) of those planned before it:
    F2[t] = union of near(pos_q[t]),  F1[t] = F2[t] | F2[t-1],  hold[a] = the goal is outside F2[t] for every a <= t <= T;
    reach[0] = {start};  c' is in reach[t+1] (t = 0 .. T-2) iff c' is not blocked, not in F1[t+1], some c in {c', c' - delta(1..4)}
    on the chip is in reach[t], not in F2[t+1] and not the goal, and hold[t+1] if c' is the goal (the first touch of the goal is
    final); arrival a* = the first t <= T-1 with the goal in reach[t]; the path is walked back from (a*, goal) taking at every level
    the lowest action number whose predecessor satisfied the conditions.
lower_bound = the largest arrival of the droplets planned alone (blocked cells only), -1 if some goal is out of reach.

Two opt-in parameters, `reserve` (R >= 0) and `retries` (Q >= 0), both 0 by default, and 0 / 0 is the rule above bit for bit.
Reservation: in an attempt with planning order o_0 .. o_{n-1} the droplet at place p is searched with F2' wherever the rule reads
F2 (the src filter, F1, hold, the walk back):
    F2'[t] = F2[t] | union over q > p of near(start of o_q)   for 1 <= t <= min(R, T);   F2'[t] = F2[t] for every other t
so a droplet not yet planned cannot be cornered on its start by the first steps of one planned before it.  Later droplets see true
paths only; the first droplet of an attempt is searched against the reservations too; lower_bound stays that of the droplets
alone.  Reservations only shrink reach sets, so every such plan is a plan under the rule above.
Retries: when all n rotations fail, let f be the first droplet that got no path in rotation 0 and O_0 the base order with f moved
to the front.  For r = 0 .. Q-1 the task is planned in order O_r; if every droplet gets a path it is kept and attempt = n + r,
otherwise the first droplet without a path moves to the front, giving O_{r+1}; the retries end early when O_{r+1} == O_r.
    res = Planner(10, 10, 4, reserve=1, retries=4).plan(starts, goals)
    ref = plan_reference(10, 10, starts, goals, reserve=1, retries=4)
The closed loop (`follow_reference`, `Follower`, `Planner.follow`) uses the same rule in every replan: "start" is where the droplet
stands at the replan, and a parked droplet has goal = position.  MEDA has neither parameter.

`plan_reference` is that statement in numpy; `Planner` runs include/route_plan.h (one workgroup per task, everything in LDS) and
must give the same arrays bit for bit.

MEDA has the same planner with the geometry of its env (include/meda_vec.h): `plan_reference_meda` and `MedaPlanner`
(include/meda_plan.h, chips up to 64 x 64); `MedaWidePlanner` (include/meda_plan_wide.h) plans the same rule on chips up to
128 x 128, and `MedaWideFollowPlanner` / `MedaWideFollower` (include/meda_follow_wide.h) close the loop there.

    res = MedaPlanner(width=30, length=30, n_agents=4).plan(starts, goals, avoid=None, health=None)
    ref = plan_reference_meda(30, 30, starts, goals)

The MEDA rule ("Space-time planner", MEDA).  A state is a droplet centre (x, y), 2 <= x <= length-3, 2 <= y <= width-3;
actions 0 N (0, -3), 1 E (+3, 0), 2 S (0, +3), 3 W (-3, 0), 4 NE (+2, -2), 5 SE (+2, +2), 6 SW (-2, +2), 7 NW (-2, -2), 8 STALL,
each axis then clamped into its range on its own: move(c, u).  T = width + length.  G(g) = the centres with d2(c, g) < 16: a
droplet inside G at the start of a step is snapped onto g by that step, whatever its action, and is done.  near(p) = the centres
with d2(c, p) < 36, where the env counts a failure (done droplets included); it counts after a step, so nothing is forbidden at
t = 0.  blocked = the centres whose 5x5 box touches a cell of `avoid` ((B, width, length), indexed [y][x]; with `health` every cell
below 1.0 joins it: the move probability is the box mean, 1.0 only on an all-healthy box).  A task with a start centre blocked
through `health` comes back failed, its lower bound kept.

Priority: droplets by descending d2(start, goal), ties by ascending index; attempt k plans them in that order rotated left by k.

One droplet against the planned paths pos_q[t], t = 0 .. T (a planned droplet sits on its goal from its snap step on):
    F[0] = empty;  F[t] = union of near(pos_q[t]) (t >= 1);  hold[a] = g outside F[t] for every a <= t <= T
    reach[0] = {start}
    arrival a* = the first t <= T-2 with  reach[t] & G & ~F[t]  non-empty and hold[t+1]
    src[t]     = reach[t] & ~G
    reach[t+1] = (union over u = 0..8 of move(src[t], u)) & ~blocked & ~F[t+1]
The arrival cell is the lowest (y, x) of reach[a*] & G & ~F[a*].  The path is walked back from it: at (t+1, c') the lowest action
number u for which some c in src[t] has move(c, u) = c', and among that action's sources the lowest (y, x).  Positions: the path,
then g from a*+1 on; actions: the walked ones, then 8.  steps = max (a* + 1) <= T-1 (the env grants success only while
step_count < max_step).  lower_bound = the same with no other droplet, -1 if some goal is out of reach.

The failure-safe MEDA rule (`safe=True`; include/meda_follow.h) guards both directions of a failed move, as
the DMFB rule does: with N[t] = union of near(pos_q[t]), t = 0 .. T (level 0 included), hold_s[a] = g outside N[t] for a <= t <= T,
    arrival a* = the first t <= T-2 with  reach[t] & G  non-empty and hold_s[t]
    src[t]     = reach[t] & ~G & ~N[t+1]                                                    (I fail, q moves)
    reach[t+1] = (union over u of move(src[t], u)) & ~blocked & ~N[t+1] & ~N[t]             (q fails, I move)
and everything else as above.  From a state whose pairs are all d2 >= 36, one env step of such plans cannot produce a pair with
d2 < 36, whichever subset of the drawn moves fails.  `follow_reference_meda` / `MedaFollower` / `MedaPlanner.follow` close the loop
around it for chips with degraded electrodes, as `follow_reference` / `Follower` / `Planner.follow` do for DMFB;
`MedaWideFollower` / `MedaWideFollowPlanner.follow` are the same loop on chips up to 128 x 128."""
import functools

import numpy as np

from . import _lib
from .route import validate_tasks

DELTA = ((0, 0), (1, 0), (-1, 0), (0, -1), (0, 1))
MAX_DIM = 64      # include/route_plan.h: ROUTE_PLAN_MAX_DIM
MAX_AGENTS = 16   # include/route_plan.h: ROUTE_PLAN_MAX_AGENTS
MEDA_DELTA = ((0, -3), (3, 0), (0, 3), (-3, 0), (2, -2), (2, 2), (-2, 2), (-2, -2), (0, 0))
MEDA_STALL = 8
MEDA_MAX_DIM = 64      # include/meda_plan.h: MEDA_PLAN_MAX_DIM
MEDA_MAX_AGENTS = 16   # include/meda_plan.h: MEDA_PLAN_MAX_AGENTS
MEDA_WIDE_MAX_DIM = 128   # include/meda_plan_wide.h: MEDA_PLAN_WIDE_MAX_DIM


class PlanResult:
    """positions uint8 (B, T+1, n, 2), actions int8 (B, T, n) (-1 from `steps` on), steps int64 (B,), success bool (B,),
    constraints (B,) (always 0: a planned route has no conflict; int64 for DMFB, float64 for MEDA, as the envs count them),
    attempt int32 (B,): the rotation that was kept (n + r for retry r), -1 for a failed task; lower_bound int32 (B,): steps no router can beat, -1 if
    a goal cannot be reached at all."""

    def __init__(self, positions, actions, steps, success, constraints, attempt, lower_bound):
        self.positions, self.actions, self.steps = positions, actions, steps
        self.success, self.constraints, self.attempt, self.lower_bound = success, constraints, attempt, lower_bound

    def __len__(self):
        return len(self.steps)


def _blank(B, T, n, constraints, follow=False):
    """The result of B tasks before anything is routed (what B == 0 returns): a PlanResult, with `follow` a FollowResult."""
    head = (np.zeros((B, T + 1, n, 2), np.uint8), np.full((B, T, n), -1, np.int8), np.zeros(B, np.int64), np.zeros(B, bool),
            np.zeros(B, constraints))
    if follow:
        return FollowResult(*head, np.zeros(B, np.int32), np.zeros(B, bool), np.zeros(B, np.int32))
    return PlanResult(*head, np.full(B, -1, np.int32), np.zeros(B, np.int32))


def _check_avoid(avoid, B, width, length):
    if avoid is None:
        return None
    avoid = np.asarray(avoid)
    if avoid.shape != (B, width, length):
        raise ValueError('avoid must have shape (B=%d, %d, %d), got %s' % (B, width, length, avoid.shape))
    return np.ascontiguousarray(avoid != 0)


def _checked(geo, width, length, n_agents, starts, goals, blocks, avoid, health):
    """What every entry point checks first: validate_tasks for the geometry's env, and `avoid` as bool (B, width, length) or None."""
    starts, goals, blocks, health = validate_tasks(geo.name, width, length, n_agents, starts, goals, blocks, health)
    return starts, goals, blocks, _check_avoid(avoid, starts.shape[0], width, length), health


def _refuse(res, starts, weak):
    """The tasks of `weak` as failures (their lower bound stays)."""
    if weak is not None and weak.any():
        res.positions[weak] = starts[weak][:, None].astype(np.uint8)
        res.actions[weak], res.steps[weak], res.success[weak], res.attempt[weak] = -1, 0, False, -1
    return res


# ---------------------------------------------------------------------------------------------------- DMFB: the rule in numpy
def _route_one(W, L, T, start, goal, blocked, F2, aux=None):
    """(positions t = 0 .. a*, actions t = 0 .. a*-1) of one droplet against F2 (bool (T+1, W, L)), or None."""
    gx, gy = goal
    hold = np.logical_and.accumulate(~F2[::-1, gx, gy])[::-1]      # hold[a], a = 0 .. T
    if start == goal:
        return ([start], []) if hold[0] else None
    reach = [np.zeros((W, L), bool)]
    reach[0][start] = True
    arrival = None
    for t in range(T - 1):
        src = reach[t] & ~F2[t + 1]
        src[gx, gy] = False
        nxt = src.copy()
        nxt[1:, :] |= src[:-1, :]
        nxt[:-1, :] |= src[1:, :]
        nxt[:, :-1] |= src[:, 1:]
        nxt[:, 1:] |= src[:, :-1]
        nxt &= ~blocked
        nxt &= ~(F2[t + 1] | F2[t])
        if not hold[t + 1]:
            nxt[gx, gy] = False
        reach.append(nxt)
        if nxt[gx, gy]:
            arrival = t + 1
            break
        if not nxt.any():
            break
    if arrival is None:
        return None
    path, acts, c = [goal], [], goal
    for t in range(arrival - 1, -1, -1):
        for u, (dx, dy) in enumerate(DELTA):
            p = (c[0] - dx, c[1] - dy)
            if 0 <= p[0] < W and 0 <= p[1] < L and reach[t][p] and not F2[t + 1][p] and p != goal:
                break
        else:
            raise AssertionError('no predecessor at level %d' % t)
        path.append(p)
        acts.append(u)
        c = p
    return path[::-1], acts[::-1]


def _stamp(F2, path, goal, T, aux=None):
    """near() of a planned droplet into F2 for t = 0 .. T (it stays on its goal)."""
    for t in range(T + 1):
        x, y = path[min(t, len(path) - 1)]
        F2[t, max(0, x - 1):x + 2, max(0, y - 1):y + 2] = True


class _Dmfb:
    """The DMFB geometry: what the shared procedure below asks of an env."""
    name, pad, after, constraints = 'dmfb', 0, 0, np.int64      # the action after arrival; steps = actions walked + after
    park_min = 1      # the smallest distance to its goal at which the closed loop may park a droplet
    route_one, stamp = staticmethod(_route_one), staticmethod(_stamp)

    @staticmethod
    def limit(width, length):
        return 2 * (width + length)

    @staticmethod
    def dist(s, g):
        return abs(s[0] - g[0]) + abs(s[1] - g[1])

    @staticmethod
    def aux(W, L):
        return None

    @staticmethod
    def inputs(width, length, n_agents, starts, goals, blocks, avoid, health):
        """Validated (starts, goals, blocks, avoid, weak): cells with health < 1 join `avoid`, so that no planned move can fail.
        A move succeeds with the health of the electrode the droplet stands ON (getMoveProb), so a start on a degraded electrode
        is the one place an avoided cell is ever left from: `weak` marks those tasks, and _refuse turns their plans into failures."""
        starts, goals, blocks, avoid, health = _checked(_Dmfb, width, length, n_agents, starts, goals, blocks, avoid, health)
        weak = None
        if health is not None:
            avoid = (health < 1.0) if avoid is None else (avoid | (health < 1.0))
            weak = (health[np.arange(len(starts))[:, None], starts[..., 0], starts[..., 1]] < 1.0).any(axis=1)
        return starts, goals, blocks, avoid, weak

    @staticmethod
    def blocked(width, length, blocks, avoid):
        blocked = np.zeros((width, length), bool) if avoid is None else avoid.copy()
        if blocks is not None:
            for x0, x1, y0, y1 in blocks.tolist():
                blocked[x0:x1 + 1, y0:y1 + 1] = True
        return blocked

    # the closed loop: the state of a chip at the restart, one env step on it (returns the step's constraints), the episode's end
    @staticmethod
    def chip(starts):
        return starts.astype(np.int64), None

    @staticmethod
    def step(W, L, pos, goals, state, acts, u, health, blocks, stall):
        return _env_step(W, L, pos, goals, acts, u, health, blocks, stall)

    @staticmethod
    def over(pos, goals, state):
        return all(tuple(p) == q for p, q in zip(pos.tolist(), goals))


# ---------------------------------------------------------------------------------------------------- MEDA: the rule in numpy
def meda_move(c, u, width, length):
    """move(c, u): the centre (x, y) after action u, each axis clamped into its range on its own."""
    dx, dy = MEDA_DELTA[u]
    return min(max(c[0] + dx, 2), length - 3), min(max(c[1] + dy, 2), width - 3)


def _meda_blocked(width, length, avoid):
    """bool (width, length), [y][x]: centres off the valid range or whose 5x5 box touches a cell of `avoid`."""
    blocked = np.ones((width, length), bool)
    inner = np.zeros((width - 4, length - 4), bool)
    if avoid is not None:
        for dy in range(5):
            for dx in range(5):
                inner |= avoid[dy:dy + width - 4, dx:dx + length - 4]
    blocked[2:width - 2, 2:length - 2] = inner
    return blocked


def _meda_route_one(W, L, T, start, goal, blocked, F, aux, safe=False):
    """(positions t = 0 .. a*, actions t = 0 .. a*-1) of one droplet against F (bool (T+1, W, L); the plain rule leaves F[0] empty,
    `safe` reads it as N[0]), or None."""
    (ty, tx), (Y, X) = aux
    gx, gy = goal
    G = (X - gx) ** 2 + (Y - gy) ** 2 < 16
    hold = np.ones(T + 2, bool)
    hold[1:T + 1] = np.logical_and.accumulate(~F[:0:-1, gy, gx])[::-1]     # hold[a], a = 1 .. T
    if safe:
        hold[0] = hold[1] and not F[0, gy, gx]
    reach = np.zeros((W, L), bool)
    reach[start[1], start[0]] = True
    srcs, arrival = [], None
    for t in range(T - 1):
        if safe:
            arr, ok = reach & G, hold[t]
        else:
            arr, ok = (reach & G if t == 0 else reach & G & ~F[t]), hold[t + 1]
        if arr.any() and ok:
            arrival = t
            break
        if t == T - 2:
            break
        src = reach & ~G
        if safe:
            src &= ~F[t + 1]
        srcs.append(src)
        ys, xs = np.nonzero(src)
        if len(ys) == 0:
            break
        nxt = np.zeros((W, L), bool)
        for u in range(9):
            nxt[ty[u][ys], tx[u][xs]] = True
        reach = nxt & ~blocked & ~F[t + 1]
        if safe:
            reach &= ~F[t]
    if arrival is None:
        return None
    ys, xs = np.nonzero(arr)               # row-major: the first is the lowest (y, x)
    c = (int(xs[0]), int(ys[0]))
    path, acts = [c], []
    for t in range(arrival - 1, -1, -1):
        found = None
        for u in range(9):
            dx, dy = MEDA_DELTA[u]
            sx = [x for x in range(max(2, c[0] - 3), min(L - 3, c[0] + 3) + 1) if min(max(x + dx, 2), L - 3) == c[0]]
            sy = [y for y in range(max(2, c[1] - 3), min(W - 3, c[1] + 3) + 1) if min(max(y + dy, 2), W - 3) == c[1]]
            for y in sy:
                for x in sx:
                    if srcs[t][y, x]:
                        found = (x, y)
                        break
                if found:
                    break
            if found:
                break
        if found is None:
            raise AssertionError('no predecessor at level %d' % t)
        path.append(found)
        acts.append(u)
        c = found
    return path[::-1], acts[::-1]


def _meda_stamp(F, path, goal, T, aux, safe=False):
    """near() of a planned droplet into F for t = 1 .. T (`safe`: 0 .. T): its path, then its goal from the snap step on."""
    Y, X = aux[1]
    for t in range(0 if safe else 1, len(path)):
        F[t] |= (X - path[t][0]) ** 2 + (Y - path[t][1]) ** 2 < 36
    F[len(path):] |= (X - goal[0]) ** 2 + (Y - goal[1]) ** 2 < 36


class _Meda:
    """The MEDA geometry."""
    name, pad, after, constraints = 'meda', MEDA_STALL, 1, np.float64      # the snap step follows the walked actions
    park_min = 16     # a droplet inside its goal disc is never parked: the env snaps it whatever the plan says
    route_one, stamp = staticmethod(_meda_route_one), staticmethod(_meda_stamp)

    @staticmethod
    def limit(width, length):
        return width + length

    @staticmethod
    def dist(s, g):
        return (s[0] - g[0]) ** 2 + (s[1] - g[1]) ** 2

    @staticmethod
    def aux(W, L):
        """The clamped move tables (rows, columns) of every action and the (Y, X) grid."""
        ty = [np.clip(np.arange(W) + d[1], 2, W - 3) for d in MEDA_DELTA]
        tx = [np.clip(np.arange(L) + d[0], 2, L - 3) for d in MEDA_DELTA]
        return (ty, tx), np.mgrid[0:W, 0:L]

    @staticmethod
    def inputs(width, length, n_agents, starts, goals, blocks, avoid, health):
        """Validated (starts, goals, None, avoid, weak): cells with health < 1 join `avoid`; `weak` marks the tasks with a start
        centre whose box lies on such a cell (the one place a planned move could fail), which _refuse turns into failures."""
        starts, goals, _, avoid, health = _checked(_Meda, width, length, n_agents, starts, goals, None, avoid, health)
        B = starts.shape[0]
        weak = None
        if health is not None:
            low = health < 1.0
            avoid = low if avoid is None else (avoid | low)
            weak = np.zeros(B, bool)
            for b in range(B):
                bl = _meda_blocked(width, length, low[b])
                weak[b] = bl[starts[b, :, 1], starts[b, :, 0]].any()
        return starts, goals, None, avoid, weak

    @staticmethod
    def blocked(width, length, blocks, avoid):
        return _meda_blocked(width, length, avoid)

    # the closed loop: the centres and done flags of a chip, the env step (returns `fail`), every droplet done
    @staticmethod
    def chip(starts):
        return [tuple(p) for p in starts.tolist()], [False] * len(starts)

    @staticmethod
    def step(W, L, pos, goals, done, acts, u, health, blocks, stall):
        return _meda_env_step(W, L, pos, goals, done, acts.tolist(), u, health)

    @staticmethod
    def over(pos, goals, done):
        return all(done)


class _MedaSafe(_Meda):
    """The MEDA geometry with the failure-safe rule."""
    route_one = staticmethod(functools.partial(_meda_route_one, safe=True))
    stamp = staticmethod(functools.partial(_meda_stamp, safe=True))


# ---------------------------------------------------------------------------------------------------- the procedure, once
def _reserved(W, L, starts, later):
    """bool (W, L): the union of near(start) over the droplets `later`."""
    m = np.zeros((W, L), bool)
    for q in later:
        x, y = starts[q]
        m[max(0, x - 1):x + 2, max(0, y - 1):y + 2] = True
    return m


def _plan_one(geo, W, L, starts, goals, blocked, reserve=0, retries=0):
    """(the attempt kept or -1, {droplet: (positions, actions)} or None, lower bound) of one task."""
    n, T, aux = len(starts), geo.limit(W, L), geo.aux(W, L)
    none = np.zeros((T + 1, W, L), bool)
    alone = [geo.route_one(W, L, T, starts[i], goals[i], blocked, none, aux) for i in range(n)]
    if any(r is None for r in alone):
        return -1, None, -1         # a droplet that cannot arrive alone arrives in no attempt
    lower = max(len(r[1]) for r in alone) + geo.after
    dist = [geo.dist(starts[i], goals[i]) for i in range(n)]
    base = sorted(range(n), key=lambda i: (-dist[i], i))
    hi = min(reserve, T)           # the levels 1 .. hi carry the reservations

    def attempt(order):
        """(paths, None) if every droplet of `order` got a path, else (None, the place of the first one that got none)."""
        F = np.zeros((T + 1, W, L), bool)
        paths = {}
        for p, i in enumerate(order):
            if hi and p < n - 1:
                true = F[1:hi + 1].copy()
                F[1:hi + 1] |= _reserved(W, L, starts, order[p + 1:])
                r = geo.route_one(W, L, T, starts[i], goals[i], blocked, F, aux)
                F[1:hi + 1] = true          # the droplets planned later see true paths only
            else:
                r = alone[i] if not paths else geo.route_one(W, L, T, starts[i], goals[i], blocked, F, aux)
            if r is None:
                return None, p
            paths[i] = r
            geo.stamp(F, r[0], goals[i], T, aux)
        return paths, None

    first = None
    for k in range(n):
        paths, p = attempt(base[k:] + base[:k])
        if paths is not None:
            return k, paths, lower
        first = p if k == 0 else first
    order, p = list(base), first
    for r in range(retries):
        if r > 0 and p == 0:
            break                  # the droplet without a path is at the front already: O_{r+1} == O_r
        order = [order[p]] + order[:p] + order[p + 1:]
        paths, p = attempt(order)
        if paths is not None:
            return n + r, paths, lower
    return -1, None, lower


def _plan_reference(geo, width, length, starts, goals, blocks, avoid, health, reserve=0, retries=0):
    starts = np.asarray(starts)
    if starts.ndim != 3:
        raise ValueError('starts must have shape (B, n, 2), got %s' % (starts.shape,))
    n = starts.shape[1]
    starts, goals, blocks, avoid, weak = geo.inputs(width, length, n, starts, goals, blocks, avoid, health)
    B, T = starts.shape[0], geo.limit(width, length)
    out = _blank(B, T, n, geo.constraints)
    for b in range(B):
        blocked = geo.blocked(width, length, None if blocks is None else blocks[b], None if avoid is None else avoid[b])
        s = [tuple(p) for p in starts[b].tolist()]
        g = [tuple(p) for p in goals[b].tolist()]
        k, paths, out.lower_bound[b] = _plan_one(geo, width, length, s, g, blocked, reserve, retries)
        out.positions[b] = starts[b][None]
        if k < 0:
            continue
        steps = max(len(acts) for _, acts in paths.values()) + geo.after
        out.success[b], out.attempt[b], out.steps[b] = True, k, steps
        for i, (p, acts) in paths.items():
            out.positions[b, :, i] = np.array(p + [g[i]] * (T + 1 - len(p)))       # on its goal once the path ends
            out.actions[b, :steps, i] = acts + [geo.pad] * (steps - len(acts))
    return _refuse(out, starts, weak)


def _check_rule(reserve, retries):
    """(reserve, retries) as ints; each 0 .. 255, as include/route_plan.h takes them."""
    reserve, retries = int(reserve), int(retries)
    if not (0 <= reserve <= 255 and 0 <= retries <= 255):
        raise ValueError('reserve and retries must lie in 0 .. 255, got %d and %d' % (reserve, retries))
    return reserve, retries


def plan_reference(width, length, starts, goals, blocks=None, avoid=None, health=None, reserve=0, retries=0):
    """The rule in plain numpy, one task after another on the CPU: what Planner.plan must equal bit for bit.  `reserve`, `retries`:
    R and Q of the rule (0 / 0: no reservations, the n rotations only)."""
    reserve, retries = _check_rule(reserve, retries)
    return _plan_reference(_Dmfb, width, length, starts, goals, blocks, avoid, health, reserve, retries)


def plan_reference_meda(width, length, starts, goals, avoid=None, health=None, safe=False):
    """The MEDA rule in plain numpy, one task after another on the CPU: what MedaPlanner.plan must equal bit for bit.  `safe`: the
    failure-safe rule."""
    return _plan_reference(_MedaSafe if safe else _Meda, width, length, starts, goals, None, avoid, health)


# ---------------------------------------------------------------------------------------------------- the closed loop
class FollowResult:
    """positions uint8 (B, T+1, n, 2): after the restart and after every lock-step, the last position repeated; actions int8
    (B, T, n): what was played, -1 from `steps` on; steps int64 (B,) lock-steps played; success bool (B,); constraints int64
    (B,) summed over the episode; replans int32 (B,): plans made, the first included; gave_up bool (B,): a replan found no
    route, the chip was frozen there; lower_bound int32 (B,): of the first plan, -1 if a goal cannot be reached at all.
    `Follower.play` returns the same fields as device tensors, and `reward` float64 (B,), the summed team reward."""

    def __init__(self, positions, actions, steps, success, constraints, replans, gave_up, lower_bound, reward=None):
        self.positions, self.actions, self.steps, self.success = positions, actions, steps, success
        self.constraints, self.replans, self.gave_up, self.lower_bound = constraints, replans, gave_up, lower_bound
        self.reward = reward

    def __len__(self):
        return len(self.steps)


def _follow_inputs(geo, width, length, starts, goals, blocks, avoid, health, min_health):
    """Validated (starts, goals, blocks, blocked cells or None, health): a cell is avoided if it lies in `avoid` or its health is
    below `min_health` (nothing enters it, for MEDA with any cell of a 5x5 box; a droplet that stands on one may leave)."""
    starts = np.asarray(starts)
    if starts.ndim != 3:
        raise ValueError('starts must have shape (B, n, 2), got %s' % (starts.shape,))
    starts, goals, blocks, avoid, health = _checked(geo, width, length, starts.shape[1], starts, goals, blocks, avoid, health)
    if health is not None and min_health > 0.0:
        low = health < min_health
        avoid = low if avoid is None else (avoid | low)
    return starts, goals, blocks, avoid, health


def _park_order(geo, pos, goals):
    d = [geo.dist(p, g) for p, g in zip(pos, goals)]
    return sorted((i for i in range(len(pos)) if d[i] >= geo.park_min), key=lambda i: (d[i], -i))


def park_order(pos, goals):
    """The droplets off their goals by ascending Manhattan distance, ties by descending index: the order in which a replan parks."""
    return _park_order(_Dmfb, pos, goals)


def park_order_meda(pos, goals):
    """The droplets outside their goal discs (d2 >= 16) by ascending d2, ties by descending index."""
    return _park_order(_MedaSafe, pos, goals)


def _replan(W, L, pos, goals, blocked, geo=_Dmfb, reserve=0, retries=0):
    """(k, actions (steps, n) and positions (steps + 1, n, 2) of the plan, lower bound of k = 0), k = -1 if every parking fails."""
    order, first = _park_order(geo, pos, goals), None
    for k in range(max(1, len(order))):      # a chip with every droplet at home is planned once, with nobody to park
        g = list(goals)
        for i in order[:k]:
            g[i] = pos[i]
        kept, paths, lower = _plan_one(geo, W, L, pos, g, blocked, reserve, retries)
        first = lower if k == 0 else first
        if kept >= 0:
            steps, n = max(len(a) for _, a in paths.values()) + geo.after, len(pos)
            acts = np.full((steps, n), geo.pad, np.int8)
            route = np.zeros((steps + 1, n, 2), np.int64)
            for i, (p, a) in paths.items():
                acts[:len(a), i] = a
                route[:, i] = np.array(p + [g[i]] * (steps + 1 - len(p)))
            return k, acts, route, first
    return -1, None, None, first


def _env_step(W, L, pos, goals, acts, u, health, blocks, stall):
    """The env's move rule (moveOneDroplet, droplet after droplet) on the positions of one chip, in place; returns the step's
    constraints (static and dynamic conflicts, each counted for both droplets)."""
    n, past = len(pos), pos.copy()
    for i in range(n):
        x, y = pos[i]
        if stall and (x, y) == tuple(goals[i]):
            continue
        if u[i] <= (1.0 if health is None else health[x, y]):
            dx, dy = DELTA[acts[i]]
            nx, ny = min(max(x + dx, 0), W - 1), min(max(y + dy, 0), L - 1)
            if blocks is not None and any(x0 <= nx <= x1 and y0 <= ny <= y1 for x0, x1, y0, y1 in blocks):
                nx, ny = x, y
            if any((nx, ny) == tuple(pos[j]) for j in range(n) if j != i):
                nx, ny = x, y
            pos[i] = (nx, ny)
    close = lambda a, b: abs(a[0] - b[0]) <= 1 and abs(a[1] - b[1]) <= 1      # norm < 2
    static = sum(2 for i in range(n) for j in range(i + 1, n) if close(pos[i], pos[j]))
    dynamic = sum(2 for i in range(n) for j in range(n) if i != j and close(past[i], pos[j]))
    return static + dynamic


def _meda_env_step(W, L, pos, goals, done, acts, u, health):
    """The env's step (oracle/meda_oracle.c: step_env) on the centres and done flags of one chip, in place; returns `fail`."""
    n = len(pos)
    for i in range(n):
        if done[i]:
            continue
        x, y = int(pos[i][0]), int(pos[i][1])
        if _Meda.dist((x, y), goals[i]) < 16:        # inside the goal disc at the start of the step: snapped, no draw
            pos[i], done[i] = goals[i], True
            continue
        prob = 1.0
        if health is not None:                       # the 25 cells summed row-major, then divided: the env's operation order
            prob = 0.0
            for cy in range(y - 2, y + 3):
                for cx in range(x - 2, x + 3):
                    prob = prob + float(health[cy, cx])
            prob = prob / 25.0
        if u[i] <= prob:
            pos[i] = meda_move((x, y), acts[i], W, L)
    punish = np.zeros(n)
    for i in range(n):
        for j in range(i + 1, n):
            if _Meda.dist(pos[i], pos[j]) < 36:
                punish[i] -= 0.6
                punish[j] -= 0.6
    return float(np.sum(punish))       # numpy's pairwise order for n >= 8, as the env


def _follow_reference(geo, width, length, starts, goals, blocks, avoid, health, min_health, uniforms, stall, reserve, retries):
    """The closed loop of both envs, once: what follow_reference and follow_reference_meda state.  `geo` gives the limit, the
    constraints dtype, the chip's state and env step, the end of an episode and the action a droplet plays where its plan has
    none.  A step's constraints are never of mixed sign (DMFB counts conflicts, MEDA sums penalties), so an episode's sum is 0
    exactly when every step's is."""
    starts, goals, blocks, avoid, health = _follow_inputs(geo, width, length, starts, goals, blocks, avoid, health, float(min_health))
    B, n = starts.shape[:2]
    W, L, T = width, length, geo.limit(width, length)
    if uniforms is None:
        uniforms = np.zeros((T, B, n))
    uniforms = np.asarray(uniforms, np.float64)
    if uniforms.shape != (T, B, n):
        raise ValueError('uniforms must have shape (T=%d, B=%d, n=%d), got %s' % (T, B, n, uniforms.shape))
    out = _blank(B, T, n, geo.constraints, follow=True)
    for b in range(B):
        blocked = geo.blocked(W, L, None if blocks is None else blocks[b], None if avoid is None else avoid[b])
        bl = None if blocks is None else blocks[b].tolist()
        g = [tuple(p) for p in goals[b].tolist()]
        pos, state = geo.chip(starts[b])
        out.positions[b, 0] = pos
        acts = route = None
        cursor, partial, t, failed = 0, False, 0, False
        while t < T:
            if acts is None or partial or not np.array_equal(pos, route[min(cursor, len(route) - 1)]):
                k, acts, route, lower = _replan(W, L, [tuple(p) for p in np.asarray(pos).tolist()], g, blocked, geo, reserve, retries)
                if t == 0:
                    out.lower_bound[b] = lower
                if k < 0:
                    out.gave_up[b] = True
                    break
                cursor, partial = 0, k > 0
                out.replans[b] += 1
            a = acts[cursor] if cursor < len(acts) else np.full(n, geo.pad, np.int8)      # -1 read as STALL
            cursor += 1
            out.actions[b, t] = a
            c = geo.step(W, L, pos, g, state, a, uniforms[t, b], None if health is None else health[b], bl, stall)
            out.constraints[b] += c
            failed = failed or c != 0
            t += 1
            out.positions[b, t] = pos
            if geo.over(pos, g, state):
                out.success[b] = t < T and not failed
                break
        out.steps[b] = t
        out.positions[b, t:] = pos
    return out


def follow_reference(width, length, starts, goals, blocks=None, avoid=None, health=None, min_health=0.0, uniforms=None,
                     stall=True, reserve=0, retries=0):
    """The closed loop in plain numpy ("Closed-loop routing"): plan, step the chip with the env's move rule, keep the
    plan while the chip is where the plan says, otherwise replan from where it is, parking the droplets nearest their goals
    until the rest can be routed.  `uniforms` float64 (T, B, n): the move draw of droplet i of task b at lock-step t (None: every
    move succeeds).  `stall=False` (a droplet on its goal draws and moves like any other) is accepted and changes nothing: a
    plan stalls every droplet that is on its goal, and the draws are given per droplet, not taken from a stream.
    `reserve`, `retries`: R and Q of the rule, in every replan (a droplet's start is where it stands at the replan).
    What Planner.follow must equal bit for bit."""
    reserve, retries = _check_rule(reserve, retries)
    return _follow_reference(_Dmfb, width, length, starts, goals, blocks, avoid, health, min_health, uniforms, stall, reserve, retries)


def follow_reference_meda(width, length, starts, goals, avoid=None, health=None, min_health=0.0, uniforms=None):
    """The closed loop for MEDA in plain numpy: the loop of follow_reference with the MEDA env step, the
    failure-safe rule for every plan, and parking only of droplets outside their goal discs.  A centre is blocked if its 5x5 box
    touches a cell of `avoid` or a cell with health < min_health.  `uniforms` float64 (T, B, n), T = width + length: the move
    draw of droplet i of task b at lock-step t (None: every move succeeds).  `constraints` is the env's summed `fail` (float64,
    <= 0).  What MedaPlanner.follow must equal bit for bit."""
    return _follow_reference(_MedaSafe, width, length, starts, goals, None, avoid, health, min_health, uniforms, True, 0, 0)


# ---------------------------------------------------------------------------------------------------- the GPU planners
class _DevicePlanner:
    """One workgroup per task, any batch size in one launch on the current stream.  A subclass names its geometry, its entry
    point as a (library, function) pair and, in _launch, that function's argument list (`out`: the six result pointers in the
    headers' order)."""

    def __init__(self, width, length, n_agents, device=None):
        import torch
        self.width, self.length, self.n_agents = int(width), int(length), int(n_agents)
        self.episode_limit = self.geo.limit(self.width, self.length)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())

    def _plan(self, entry, starts, goals, blocks, avoid, health):
        import torch
        W, L, n, T = self.width, self.length, self.n_agents, self.episode_limit
        starts, goals, blocks, avoid, weak = self.geo.inputs(W, L, n, starts, goals, blocks, avoid, health)
        B = starts.shape[0]
        if B == 0:
            return _blank(0, T, n, self.geo.constraints)
        route = getattr(_lib.checked(entry[0]), entry[1])
        dev = self.device
        with torch.cuda.device(dev):
            nb = 0 if blocks is None else blocks.shape[1]
            d_in = [torch.as_tensor(a, device=dev) for a in (starts, goals)]
            d_in += [torch.as_tensor(blocks, device=dev) if nb else None,
                     torch.as_tensor(avoid.astype(np.uint8), device=dev) if avoid is not None else None]
            out = [torch.empty((B, T + 1, n, 2), dtype=torch.uint8, device=dev), torch.empty((B, T, n), dtype=torch.int8, device=dev)]
            out += [torch.empty(B, dtype=dt, device=dev) for dt in (torch.int32, torch.uint8, torch.int32, torch.int32)]
            ptr = lambda t: None if t is None else t.data_ptr()
            self._launch(route, B, nb, *[ptr(t) for t in d_in], [ptr(t) for t in out], torch.cuda.current_stream(dev).cuda_stream)
            pos, u, steps, success, attempt, lower = [t.cpu().numpy() for t in out]
        return _refuse(PlanResult(pos, u, steps.astype(np.int64), success > 0, np.zeros(B, self.geo.constraints), attempt, lower),
                       starts, weak)


    def _follow(self, starts, goals, blocks, avoid, health, min_health, seed, uniforms, use_graph, stall=True):
        """The common part of Planner.follow and MedaPlanner.follow: one env handle and follower per (B, blocks per task, health
        given, stall), made by the subclass's _follower."""
        import torch
        W, L, n, T = self.width, self.length, self.n_agents, self.episode_limit
        starts, goals, blocks, avoid, health = _follow_inputs(self.geo, W, L, starts, goals, blocks, avoid, health, 0.0)
        # torch takes no read-only array
        own = lambda a: a.copy() if isinstance(a, np.ndarray) and not a.flags.writeable else a
        starts, goals, blocks, health, uniforms = own(starts), own(goals), own(blocks), own(health), own(uniforms)
        B = starts.shape[0]
        if B == 0:
            res = _blank(0, T, n, self.geo.constraints, follow=True)
            res.reward = np.zeros(0)
            return res
        nb = 0 if blocks is None else blocks.shape[1]
        key = (B, nb, health is not None, stall)
        if not hasattr(self, '_followers'):
            self._followers = {}
        f = self._followers.get(key)
        with torch.cuda.device(self.device):
            if f is None:
                f = self._followers[key] = self._follower(B, nb, health is not None, stall)
            env = f.env
            f.min_health, f.use_graph = float(min_health), bool(use_graph)
            f.set_avoid(avoid)
            env.set_task(starts, goals)
            if nb:
                env.set_blocks(blocks)
            if health is not None:
                env.set_map('health', health)
            env.restart()
            if uniforms is None and health is not None:
                g = torch.Generator(device=self.device)
                g.manual_seed(int(seed))
                uniforms = torch.empty((T, B, n), dtype=torch.float64, device=self.device).uniform_(0.0, 1.0, generator=g)
            res = f.play(uniforms=uniforms, record=False)
            host = lambda t: t.cpu().numpy()
            return FollowResult(host(res.positions), host(res.actions), host(res.steps), host(res.success), host(res.constraints),
                                host(res.replans), host(res.gave_up), host(res.lower_bound), reward=host(res.reward))

class _Follower:
    """What Follower (DMFB) and MedaFollower share: the episode's buffers, the T lock-steps (route append, the library's lock-step
    kernel, env.step) eagerly or as one captured graph, and `play`.  A subclass names its library, the limit of its header, the
    dtype of the env's constraints and, in _kernel, the call of its lock-step function (`state`: the eleven state pointers both
    headers take in one order: route, route_u, cursor, partial, replans, gave_up, active, steps, lower bound, actions, u)."""
    library = max_dim = limit_msg = constraints_dtype = None

    def __init__(self, env, min_health=0.0, avoid=None, use_graph=False, reserve=0, retries=0):
        import torch
        self.reserve, self.retries = self._rule(reserve, retries)
        if env.width > self.max_dim or env.length > self.max_dim:
            raise NotImplementedError(self.limit_msg)
        self.env, self.min_health, self.use_graph = env, float(min_health), bool(use_graph)
        self.lib = _lib.checked(self.library)
        B, n, T, dev = env.n_envs, env.n_agents, env.max_step, env.device
        self.T = T
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.goals = z((B, n, 2), torch.int32)
        self.blocks = z((B, max(1, getattr(env, 'n_blocks', 0)), 4), torch.int32)
        self.n_blocks = 0
        self.mask = z((B, env.width, env.length), torch.uint8)
        self.positions, self.actions = z((B, T + 1, n, 2), torch.uint8), z((B, T, n), torch.int8)
        self._route, self._route_u = z((B, T + 1, n, 2), torch.uint8), z((B, T, n), torch.int8)
        self._i32 = z((4, B), torch.int32)     # cursor, replans, steps, lower bound
        self._u8 = z((3, B), torch.uint8)      # partial, gave up, active
        self._act = z((B, n), torch.int32)
        self._active_in = torch.ones(B, dtype=torch.uint8, device=dev)
        self._draws = None
        self.success, self.reward = z(B, torch.uint8), z(B, torch.float64)
        self.constraints = z(B, getattr(torch, self.constraints_dtype))
        self.avoid = None
        self.set_avoid(avoid)
        self._graphs = {}

    @staticmethod
    def _rule(reserve, retries):
        """The geometry's check of (reserve, retries): only DMFB has them."""
        if reserve or retries:
            raise ValueError('reserve and retries belong to the DMFB rule alone')
        return 0, 0

    def set_avoid(self, avoid):
        import torch
        env = self.env
        if avoid is not None:
            avoid = torch.as_tensor(np.asarray(avoid) != 0, device=env.device)
            if tuple(avoid.shape) != (env.n_envs, env.width, env.length):
                raise ValueError('avoid must have shape (%d, %d, %d), got %s' % (env.n_envs, env.width, env.length, tuple(avoid.shape)))
        self.avoid = avoid

    def _prepare(self):
        """What holds for the whole episode, read from the env: goals, blocks and the blocked mask."""
        env = self.env
        self.goals.copy_(env.get_task()[1])
        self._prepare_blocks()
        self.mask.zero_()
        if self.avoid is not None:
            self.mask.copy_(self.avoid)
        if env.has_maps and self.min_health > 0.0:
            self.mask.bitwise_or_((env.get_map('health') < self.min_health).to(self.mask.dtype))

    def _prepare_blocks(self):
        pass

    def _episode(self, uniforms, record):
        env, T = self.env, self.T
        cursor, replans, steps, lower = self._i32
        partial, gave_up, active = self._u8
        self._i32.zero_()
        cursor.fill_(-1)
        self._u8.zero_()
        active.copy_(self._active_in)
        self.actions.fill_(-1)
        self._act.zero_()
        self.success.zero_()
        self.constraints.zero_()
        self.reward.zero_()
        blocks = self.blocks[:, :self.n_blocks].contiguous() if self.n_blocks else None
        state = [x.data_ptr() for x in (self._route, self._route_u, cursor, partial, replans, gave_up, active, steps, lower, self._act,
                                        self.actions)]
        env.restart()     # droplets on their starts, counters zero: nothing new after a reset or a restart, and what lets a
        for t in range(T):   # warm-up episode be played before a capture
            env.route_append(t - 1, T, self.positions)
            self._kernel(t, blocks, state)
            _, _, _, info = env.step(self._act, None if uniforms is None else uniforms[t], record=record, active=active)
            self.success.bitwise_or_(info['success'])
            self.constraints.add_(info['constraints'])
            self.reward.add_(info['team_reward'])
        env.route_append(T - 1, T, self.positions)

    def play(self, uniforms=None, record=True, active=None):
        """Plays one episode on every chip whose `active` byte is set (all when None).  uniforms: float64 (T, B, n) move draws on
        the device or as an array, None = the handle's Philox stream.  Returns a FollowResult of device tensors, which the next
        call reuses."""
        import torch
        env, T = self.env, self.T
        with torch.cuda.device(env.device):
            self._prepare()
            self._active_in.fill_(1) if active is None else self._active_in.copy_(env._dev(active, torch.uint8))
            if uniforms is not None:
                if self._draws is None:
                    self._draws = torch.zeros((T, env.n_envs, env.n_agents), dtype=torch.float64, device=env.device)
                u = env._dev(uniforms, torch.float64)
                if tuple(u.shape) != tuple(self._draws.shape):
                    raise ValueError('uniforms must have shape %s, got %s' % (tuple(self._draws.shape), tuple(u.shape)))
                self._draws.copy_(u)
            draws = self._draws if uniforms is not None else None
            if not self.use_graph:
                self._episode(draws, record)
            else:
                key = (draws is not None, bool(record), self.n_blocks, self.reserve, self.retries)
                g = self._graphs.get(key)
                if g is None:
                    cur = torch.cuda.current_stream(env.device)
                    side = torch.cuda.Stream(device=env.device)
                    side.wait_stream(cur)
                    with torch.cuda.stream(side):   # warm-up outside capture (code objects, the LDS limit); it wears nothing
                        self._episode(draws, False)
                    cur.wait_stream(side)
                    torch.cuda.synchronize(env.device)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self._episode(draws, record)
                    self._graphs[key] = g
                g.replay()
        cursor, replans, steps, lower = self._i32
        partial, gave_up, active = self._u8
        return FollowResult(self.positions, self.actions, steps.long(), self.success > 0, self.constraints, replans, gave_up > 0,
                            lower, reward=self.reward)


class Follower(_Follower):
    """Closed-loop routing of the tasks a VecDMFB holds (include/route_plan.h: route_follow_dmfb), everything on the device.

        env.set_task(starts, goals); env.restart()          # or env.reset()
        res = Follower(env, min_health=0.5).play()          # FollowResult of device tensors

    Goals, blocks and (on a handle with maps) health are read from the env when `play` starts; `avoid` (B, width, length), non-zero =
    a cell no droplet may enter, and the cells with health < min_health make the blocked mask.  The T lock-steps (route append,
    route_follow_dmfb_opt, env.step) run eagerly or, with `use_graph`, as one captured graph that is replayed by later calls.
    `reserve`, `retries`: R and Q of the rule, in every replan; they may be set between calls of `play` on the eager path, a
    captured graph keeps those it was captured with (`play` captures one per pair)."""
    library, max_dim, constraints_dtype = 'route_plan', MAX_DIM, 'int64'
    limit_msg = 'chip larger than the planner takes (include/route_plan.h: ROUTE_PLAN_MAX_DIM)'
    _rule = staticmethod(_check_rule)

    def _prepare_blocks(self):
        blocks = self.env.get_blocks()
        self.n_blocks = int(blocks.shape[1])
        if self.n_blocks:
            self.blocks[:, :self.n_blocks].copy_(blocks)

    def _kernel(self, t, blocks, state):
        env = self.env
        self.lib.route_follow_dmfb_opt(env.n_envs, env.width, env.length, env.n_agents, self.n_blocks, t, self.goals.data_ptr(),
                                       None if blocks is None else blocks.data_ptr(), self.mask.data_ptr(), self.positions.data_ptr(),
                                       *state, self.reserve, self.retries, env._stream().value)


class MedaFollower(_Follower):
    """Closed-loop routing of the tasks a VecMEDA holds (include/meda_follow.h: meda_follow_step): `Follower` for MEDA.  Every plan
    is made with the failure-safe rule; a centre is blocked if its 5x5 box touches a cell of `avoid` or one with health <
    min_health; the end of an episode is what the env's step reported (`terminated`); `constraints` is the summed `fail`."""
    library, max_dim, constraints_dtype = 'meda_follow', MEDA_MAX_DIM, 'float64'
    limit_msg = 'chip larger than the follower takes (include/meda_follow.h: MEDA_FOLLOW_MAX_DIM)'

    def _kernel(self, t, blocks, state):
        env = self.env
        self.lib.meda_follow_step(env.n_envs, env.width, env.length, env.n_agents, t, self.goals.data_ptr(), self.mask.data_ptr(),
                                  self.positions.data_ptr(), env.terminated.data_ptr(), *state, env._stream().value)


class MedaWideFollower(_Follower):
    """`MedaFollower` on chips up to MEDA_WIDE_MAX_DIM = 128 rows and columns (include/meda_follow_wide.h: meda_follow_wide_step;
    smaller chips included, where it equals MedaFollower).  The levels of a plan that do not fit the LDS of a workgroup go to a
    device workspace, sized by meda_follow_wide_work_bytes and allocated here, once: the lock-steps of `play` may be captured as a
    graph.  `lds_levels`: at most that many levels stay in LDS (None: as many as fit); the episodes do not depend on it."""
    library, max_dim, constraints_dtype = 'meda_follow_wide', MEDA_WIDE_MAX_DIM, 'float64'
    limit_msg = 'chip larger than the wide follower takes (include/meda_follow_wide.h: MEDA_FOLLOW_WIDE_MAX_DIM)'

    def __init__(self, env, min_health=0.0, avoid=None, use_graph=False, lds_levels=None):
        import torch
        self.lds_levels = 0 if lds_levels is None else int(lds_levels)
        if self.lds_levels < 0:
            raise ValueError('lds_levels must be positive or None, got %d' % self.lds_levels)
        super().__init__(env, min_health=min_health, avoid=avoid, use_graph=use_graph)
        # a negative byte count is the error code the first lock-step is about to raise for the same sizes
        self._work_bytes = max(0, self.lib.meda_follow_wide_work_bytes(env.n_envs, env.width, env.length, env.n_agents, self.lds_levels))
        self._work = torch.empty(self._work_bytes, dtype=torch.uint8, device=env.device) if self._work_bytes else None

    def _kernel(self, t, blocks, state):
        env = self.env
        self.lib.meda_follow_wide_step(env.n_envs, env.width, env.length, env.n_agents, t, self.goals.data_ptr(), self.mask.data_ptr(),
                                       self.positions.data_ptr(), env.terminated.data_ptr(), *state,
                                       None if self._work is None else self._work.data_ptr(), self._work_bytes, self.lds_levels,
                                       env._stream().value)


class Planner(_DevicePlanner):
    """include/route_plan.h on `device`.  `reserve`, `retries`: R and Q of the rule, for `plan` and for every replan of `follow`."""
    geo, entry = _Dmfb, ('route_plan', 'route_plan_dmfb_opt')

    def __init__(self, width, length, n_agents, device=None, reserve=0, retries=0):
        super().__init__(width, length, n_agents, device)
        self.reserve, self.retries = _check_rule(reserve, retries)

    def plan(self, starts, goals, blocks=None, avoid=None, health=None):
        return self._plan(self.entry, starts, goals, blocks, avoid, health)

    def _launch(self, route, B, nb, s, g, blocks, avoid, out, stream):
        route(B, self.width, self.length, self.n_agents, nb, s, g, blocks, avoid, *out, self.reserve, self.retries, stream)

    def follow(self, starts, goals, blocks=None, avoid=None, health=None, min_health=0.0, seed=0, uniforms=None, stall=True,
               use_graph=False):
        """Closed-loop routing of given tasks, numpy in and out: what follow_reference gives, bit for bit, when `uniforms`
        (float64 (T, B, n)) are given; without them the move draws come from a torch.Generator seeded with `seed`.  One env handle
        (and its Follower) is kept per (B, blocks per task, health given, stall)."""
        return self._follow(starts, goals, blocks, avoid, health, min_health, seed, uniforms, use_graph, bool(stall))

    def _follower(self, B, nb, maps, stall):
        from .env.dmfb import VecDMFB
        return Follower(VecDMFB(self.width, self.length, self.n_agents, nb, fov=5, stall=stall, n_envs=B, seed=0, with_maps=maps,
                                device=self.device), reserve=self.reserve, retries=self.retries)


class MedaPlanner(_DevicePlanner):
    """include/meda_plan.h on `device`: chips up to MEDA_MAX_DIM = 64 rows and columns.  Larger chips, up to 128 x 128, are planned
    by MedaWidePlanner, and followed in the closed loop by MedaWideFollowPlanner."""
    geo, entry, safe_entry = _Meda, ('meda_plan', 'meda_plan_route'), ('meda_follow', 'meda_follow_plan')

    def plan(self, starts, goals, avoid=None, health=None, safe=False):
        """`safe`: the failure-safe rule (include/meda_follow.h: meda_follow_plan), what plan_reference_meda(safe=True) gives."""
        return self._plan(self.safe_entry if safe else self.entry, starts, goals, None, avoid, health)

    def _launch(self, route, B, nb, s, g, blocks, avoid, out, stream):
        route(B, self.width, self.length, self.n_agents, s, g, avoid, *out, stream)

    def follow(self, starts, goals, avoid=None, health=None, min_health=0.0, seed=0, uniforms=None, use_graph=False):
        """Closed-loop routing of given tasks, numpy in and out: what follow_reference_meda gives, bit for bit, when `uniforms`
        (float64 (T, B, n)) are given; without them the move draws come from a torch.Generator seeded with `seed`.  One VecMEDA
        (version 2, fov 19) and its MedaFollower are kept per (B, health given)."""
        return self._follow(starts, goals, None, avoid, health, min_health, seed, uniforms, use_graph)

    def _follower(self, B, nb, maps, stall):
        from .env.meda import VecMEDA
        return MedaFollower(VecMEDA(self.width, self.length, self.n_agents, fov=19, n_envs=B, seed=0, with_maps=maps,
                                    device=self.device, version=2))


class MedaWidePlanner(_DevicePlanner):
    """include/meda_plan_wide.h on `device`: the rule of MedaPlanner.plan, plain and safe, on chips up to MEDA_WIDE_MAX_DIM = 128 rows
    and columns (smaller chips included, where it equals MedaPlanner).  The levels that do not fit the LDS of a workgroup go to a
    device workspace, sized by meda_plan_wide_work_bytes and kept per batch size.  `lds_levels`: at most that many levels stay in
    LDS (None: as many as fit); the planned routes do not depend on it.  The open loop only: MedaWideFollowPlanner adds `follow`,
    the closed loop on the same chips."""
    geo, entry = _Meda, ('meda_plan_wide', 'meda_plan_wide_route')

    def __init__(self, width, length, n_agents, device=None, lds_levels=None):
        super().__init__(width, length, n_agents, device)
        self.lds_levels = 0 if lds_levels is None else int(lds_levels)
        if self.lds_levels < 0:
            raise ValueError('lds_levels must be positive or None, got %d' % self.lds_levels)
        self._work = {}     # batch size -> the workspace

    def plan(self, starts, goals, avoid=None, health=None, safe=False):
        """`safe`: the failure-safe rule, what plan_reference_meda(safe=True) gives."""
        self._safe = bool(safe)
        return self._plan(self.entry, starts, goals, None, avoid, health)

    def _launch(self, route, B, nb, s, g, blocks, avoid, out, stream):
        import torch
        # a negative byte count is the error code `route` is about to raise for the same sizes
        need = max(0, _lib.meda_plan_wide().meda_plan_wide_work_bytes(B, self.width, self.length, self.n_agents, self.lds_levels))
        work = self._work.get(B)
        if need and (work is None or work.numel() < need):
            work = self._work[B] = torch.empty(need, dtype=torch.uint8, device=self.device)
        route(B, self.width, self.length, self.n_agents, int(self._safe), s, g, avoid, *out, work.data_ptr() if need else None, need,
              self.lds_levels, stream)


class MedaWideFollowPlanner(MedaWidePlanner):
    """MedaWidePlanner with the closed loop (include/meda_follow_wide.h): `plan` as there, and `follow` with the semantics of
    MedaPlanner.follow on chips up to MEDA_WIDE_MAX_DIM = 128 rows and columns.  `lds_levels` holds for both."""

    def follow(self, starts, goals, avoid=None, health=None, min_health=0.0, seed=0, uniforms=None, use_graph=False):
        """Closed-loop routing of given tasks, numpy in and out: what follow_reference_meda gives, bit for bit, when `uniforms`
        (float64 (T, B, n)) are given; without them the move draws come from a torch.Generator seeded with `seed`.  One VecMEDA
        (version 2, fov 19) and its MedaWideFollower, workspace included, are kept per (B, health given)."""
        return self._follow(starts, goals, None, avoid, health, min_health, seed, uniforms, use_graph)

    def _follower(self, B, nb, maps, stall):
        from .env.meda import VecMEDA
        return MedaWideFollower(VecMEDA(self.width, self.length, self.n_agents, fov=19, n_envs=B, seed=0, with_maps=maps,
                                        device=self.device, version=2), lds_levels=self.lds_levels or None)
