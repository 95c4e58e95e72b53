"""The action shields of the policy play: the best-Q action that breaks no constraint.  DMFB first, MEDA below.

`shield_reference` is the DMFB rule in batched numpy; the HIP kernel behind `VecDMFB.shield` (include/dmfb_vec.h:
dmfb_vec_shield, marl_dmfb_amd/csrc/dmfb_shield.h) equals it bit for bit.  `meda_shield_reference` is the MEDA rule, and the
kernel behind `VecMEDA.shield` (include/meda_vec.h: meda_vec_shield, marl_dmfb_amd/csrc/meda_shield.h) equals that one.

The env's constraint rule is local and one-step.  For droplets i != j a step counts a static conflict if
cheb(new_i, new_j) < 2 and a dynamic conflict if cheb(old_i, new_j) < 2 (moveDroplets, dmfb.py:254-271), with cheb the
Chebyshev distance: `< 2` is "within the 3x3 box".

The rule.  Per chip, droplets in index order i = 0 .. n-1 (the order in which the env moves them):
  * old_j = the positions before the step; frozen_i = stall and droplet i is on its goal.
  * exec(i, u) = old_i if frozen_i; else old_i + delta(u), each axis clamped onto the chip (Droplet.move, dmfb.py:103-124), and
    old_i again if that cell lies in a block (dmfb.py:338-340).  Actions: 0 STALL, 1 RIGHT (x + 1), 2 LEFT (x - 1), 3 DOWN
    (y - 1), 4 UP (y + 1).
  * candidates of droplet i: first the action that was picked (greedy or exploratory) if it lies in [0, 5), then the remaining
    actions by descending q[i][a] with float `>`; ties go to the lower action, a NaN orders below every number.
  * a candidate u with c = exec(i, u) is SAFE iff cheb(c, old_j) >= 2 for every j != i and cheb(c, new_j) >= 2 for every j < i.
  * droplet i takes its first safe candidate, new_i = c.
  * if no candidate is safe the chip was not conflict-free before the step: the pick stays, new_i = exec(i, pick) (old_i for a
    pick outside [0, 5)), and the chip's `unsafe` byte is set.
  * overrides[e] = the number of droplets whose action changed.
Chips whose `active` byte is 0 are not touched.

Why it holds.  Call a state conflict-free when every two droplets are at least 2 apart.  Take a pair i < j of a conflict-free
chip after the shield: old_i / old_j are 2 apart (the state), new_j / old_i and new_i / old_j are 2 apart (each new cell was
tested against every other old cell), and new_j / new_i are 2 apart (j was tested against the new cells decided before it).  A
move that fails on a degraded electrode leaves its droplet on its old cell, so whichever subset of the moves fails, the cells
the env compares are one of {old_i, new_i} against one of {old_j, new_j}: all four combinations are 2 apart.  Hence no static
and no dynamic conflict, the overlap revert (_isinvalidaction, dmfb.py:310-323) never fires, so exec() is what the env executes,
and the next state is conflict-free again.  STALL is always safe in a conflict-free state (exec = old_i, which every old_j and
every new_j keeps 2 away from), so a safe candidate always exists there.  Env-drawn tasks start conflict-free: all 2n start and
goal cells are drawn with squared distance > 2 (dmfb.py:207-226).

MEDA.  One step with two centres closer than 6 sets the chip's `failed`, and success = in_time && all && !failed (calPunish and
MEDAEnv.step, meda.py:321-330,522-531): every proximity event turns a routed episode into a failed one.  A droplet whose centre
is inside its goal disc at the start of a step is put on its goal whatever its action (meda.py:273-277), so STALL is not always
safe and the DMFB rule does not carry over.  All arithmetic is integer:
  * d2 = the squared Euclidean distance of two centres; near(a, b) = d2(a, b) < 36; in_disc_i(c) = d2(c, g_i) < 16.
  * move(c, u) = meda_move of plan.py: the delta of actions 0..8 (8 = STALL), each axis clamped into [2, length - 3] /
    [2, width - 3] on its own.
Per chip, before the step:
  * done_i = status bit i of the env; forced_i = done_i or in_disc_i(old_i): the env moves such a droplet to g_i, or leaves it
    there, whatever its action and with no failure draw.
  * anchor a_i = g_i if forced_i, else old_i: where droplet i is after the step if it "does nothing".
  * land_i(c) = g_i if in_disc_i(c), else c: where a droplet that reaches c is one step later if it does nothing.
Droplets in index order i = 0 .. n-1:
  * a forced droplet keeps its pick untouched; its new_i = land_i = a_i.
  * a free droplet has the candidates of the DMFB shield: first the picked action if it lies in [0, 9), then the remaining
    actions by descending q[i][a] with float `>`; ties go to the lower action, a NaN orders below every number.
  * a candidate u with c = move(old_i, u) is SAFE iff neither c nor land_i(c) is near a_j of any j != i, or new_j or
    land_j(new_j) of any j < i.
  * droplet i takes its first safe candidate.
  * if none is safe the pick stays, new_i = move(old_i, pick) (old_i for a pick outside [0, 9)), and the chip's `unsafe` byte is
    set.
  * overrides[e] grows by the number of droplets whose action changed.
Chips whose `active` byte is 0 are not touched.

Why it holds.  Call a chip safe when its anchors are pairwise not near.  After the step droplet i stands on one of {a_i, new_i}
(just a_i if forced): a failed move leaves it on old_i = a_i.  Its next anchor is one of {a_i, land_i(new_i)}.  For every pair,
all combinations of {a, new, land(new)} were tested, by whichever droplet was decided later: new and land of the later droplet
against the anchor, new and land of the earlier one, and new and land of the earlier droplet against the later one's anchor when
the earlier one was decided; anchor against anchor is the state.  So no subset of failed moves brings two centres within 6, and
the next state is safe again.  STALL is always safe in a safe state: c = land = a_i, which every later test of the others keeps
away from, so a safe candidate always exists there.  Env-drawn tasks start safe: starts are pairwise at least 9 apart, and no
start box overlaps its own goal box, so no droplet starts in its disc (meda.py:78-81,175-185)."""
import numpy as np

N_ACTIONS = 5
# Droplet.move (dmfb.py:103-124): 0 STALL, 1 RIGHT, 2 LEFT, 3 DOWN, 4 UP as (dx, dy)
DELTAS = np.array([[0, 0], [1, 0], [-1, 0], [0, -1], [0, 1]], np.int64)


def exec_cells(width, length, pos, done, blocks, stall):
    """exec(i, u) of every droplet and action: int64 (E, n, 5, 2)."""
    pos = np.asarray(pos, np.int64)
    E, n = pos.shape[:2]
    cells = pos[:, :, None, :] + DELTAS[None, None]
    cells[..., 0] = np.clip(cells[..., 0], 0, width - 1)
    cells[..., 1] = np.clip(cells[..., 1], 0, length - 1)
    stay = np.zeros((E, n, N_ACTIONS), bool)
    if blocks is not None:
        blocks = np.asarray(blocks, np.int64).reshape(E, -1, 4)
        for b in range(blocks.shape[1]):
            x0, x1, y0, y1 = (blocks[:, b, k][:, None, None] for k in range(4))
            stay |= (cells[..., 0] >= x0) & (cells[..., 0] <= x1) & (cells[..., 1] >= y0) & (cells[..., 1] <= y1)
    if stall:
        stay |= np.asarray(done).astype(bool).reshape(E, n)[:, :, None]
    return np.where(stay[..., None], pos[:, :, None, :], cells)


def candidate_order(q, picked):
    """The candidate actions of every droplet, first to last: int64 (E, n, A) for q of A actions."""
    q = np.asarray(q, np.float32)
    E, n, A = q.shape
    picked = np.asarray(picked, np.int64).reshape(E, n)
    nan = np.isnan(q)
    act = np.broadcast_to(np.arange(A), q.shape)
    # lexsort: the last key is the primary one -- numbers before NaNs, then descending q, then the lower action
    order = np.lexsort((act, -np.where(nan, np.float32(0), q), nan), axis=-1)
    in_range = (picked >= 0) & (picked < A)
    rest = order != picked[:, :, None]                        # the pick leaves the q order (stable) ...
    shifted = np.take_along_axis(order, np.argsort(~rest, axis=-1, kind='stable'), axis=-1)
    with_pick = np.concatenate([picked[:, :, None], shifted[:, :, :A - 1]], axis=-1)   # ... and goes first
    return np.where(in_range[:, :, None], with_pick, order)


def shield_reference(width, length, pos, done, blocks, stall, q, picked, active=None):
    """pos int (E, n, 2) droplet cells (x, y) before the step; done (E, n): droplet on its goal; blocks int (E, nb, 4) =
    (x_min, x_max, y_min, y_max) or None; q float32 (E, n, 5); picked int (E, n): what the pick kernel chose; active (E,) or
    None (all).  Returns (actions int32 (E, n), overrides int32 (E,), unsafe uint8 (E,)) by the rule of the module docstring."""
    pos = np.asarray(pos, np.int64)
    E, n = pos.shape[:2]
    picked = np.asarray(picked, np.int64).reshape(E, n)
    act = np.ones(E, bool) if active is None else np.asarray(active).reshape(E) != 0
    cells = exec_cells(width, length, pos, done, blocks, stall)
    cand = candidate_order(q, picked)
    rows = np.arange(E)
    new = pos.copy()
    final = picked.copy()
    unsafe = np.zeros(E, bool)
    for i in range(n):
        c = cells[:, i]                                        # (E, 5, 2)
        near_old = np.abs(c[:, :, None, :] - pos[:, None, :, :]).max(-1) < 2      # (E, 5, n)
        near_old[:, :, i] = False
        hit = near_old.any(-1)
        if i:
            hit |= (np.abs(c[:, :, None, :] - new[:, None, :i, :]).max(-1) < 2).any(-1)
        safe = ~np.take_along_axis(hit, cand[:, i], axis=1)    # (E, 5) in candidate order
        ok = safe.any(-1)
        take = cand[rows, i, np.argmax(safe, axis=-1)]
        final[:, i] = np.where(ok, take, picked[:, i])
        in_range = (final[:, i] >= 0) & (final[:, i] < N_ACTIONS)
        moved = c[rows, np.where(in_range, final[:, i], 0)]
        new[:, i] = np.where(in_range[:, None], moved, pos[:, i])
        unsafe |= ~ok
    actions = np.where(act[:, None], final, picked).astype(np.int32)
    overrides = (actions != picked).sum(-1).astype(np.int32)
    return actions, overrides, (unsafe & act).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------- MEDA
MEDA_ACTIONS = 9
# Droplet.move (meda.py:106-138) as (dx, dy): 0 N, 1 E, 2 S, 3 W, 4 NE, 5 SE, 6 SW, 7 NW, 8 STALL  (MEDA_DELTA of plan.py)
MEDA_DELTAS = np.array([[0, -3], [3, 0], [0, 3], [-3, 0], [2, -2], [2, 2], [-2, 2], [-2, -2], [0, 0]], np.int64)


def _d2(a, b):
    return ((a - b) ** 2).sum(-1)


def meda_targets(width, length, pos):
    """move(old_i, u) of every droplet and action: int64 (E, n, 9, 2) centres (x, y)."""
    pos = np.asarray(pos, np.int64)
    cells = pos[:, :, None, :] + MEDA_DELTAS[None, None]
    cells[..., 0] = np.clip(cells[..., 0], 2, length - 3)
    cells[..., 1] = np.clip(cells[..., 1], 2, width - 3)
    return cells


def meda_anchors(pos, goals, done):
    """(forced bool (E, n), anchors int64 (E, n, 2)) of the module docstring."""
    pos, goals = np.asarray(pos, np.int64), np.asarray(goals, np.int64)
    forced = np.asarray(done).astype(bool).reshape(pos.shape[:2]) | (_d2(pos, goals) < 16)
    return forced, np.where(forced[..., None], goals, pos)


def meda_shield_reference(width, length, pos, goals, done, q, picked, active=None):
    """pos int (E, n, 2) droplet centres (x, y) before the step; goals int (E, n, 2); done (E, n): the env's status; q float32
    (E, n, 9); picked int (E, n): what the pick kernel chose; active (E,) or None (all).  Returns (actions int32 (E, n),
    overrides int32 (E,), unsafe uint8 (E,)) by the MEDA rule of the module docstring."""
    pos, goals = np.asarray(pos, np.int64), np.asarray(goals, np.int64)
    E, n = pos.shape[:2]
    picked = np.asarray(picked, np.int64).reshape(E, n)
    act = np.ones(E, bool) if active is None else np.asarray(active).reshape(E) != 0
    forced, anchor = meda_anchors(pos, goals, done)
    cells = meda_targets(width, length, pos)                                          # (E, n, 9, 2)
    lands = np.where((_d2(cells, goals[:, :, None]) < 16)[..., None], goals[:, :, None], cells)
    cand = candidate_order(q, picked)
    rows = np.arange(E)
    new, land = anchor.copy(), anchor.copy()
    final = picked.copy()
    unsafe = np.zeros(E, bool)
    for i in range(n):
        free = ~forced[:, i]
        hit = np.zeros((E, MEDA_ACTIONS), bool)
        for pts in (cells[:, i], lands[:, i]):                                        # (E, 9, 2)
            near = _d2(pts[:, :, None], anchor[:, None]) < 36                         # (E, 9, n)
            near[:, :, i] = False
            hit |= near.any(-1)
            for earlier in (new, land):
                hit |= (_d2(pts[:, :, None], earlier[:, None, :i]) < 36).any(-1)
        safe = ~np.take_along_axis(hit, cand[:, i], axis=1)                           # (E, 9) in candidate order
        ok = safe.any(-1)
        take = cand[rows, i, np.argmax(safe, axis=-1)]
        final[:, i] = np.where(free & ok, take, picked[:, i])
        in_range = (final[:, i] >= 0) & (final[:, i] < MEDA_ACTIONS)
        u = np.where(in_range, final[:, i], MEDA_ACTIONS - 1)
        moved = np.where(in_range[:, None], cells[rows, i, u], pos[:, i])
        new[:, i] = np.where(free[:, None], moved, anchor[:, i])
        land[:, i] = np.where(free[:, None], np.where((_d2(moved, goals[:, i]) < 16)[:, None], goals[:, i], moved), anchor[:, i])
        unsafe |= free & ~ok
    actions = np.where(act[:, None], final, picked).astype(np.int32)
    overrides = (actions != picked).sum(-1).astype(np.int32)
    return actions, overrides, (unsafe & act).astype(np.uint8)
