"""The action shield of the DMFB policy play: the best-Q action that breaks no constraint.

`shield_reference` is the rule in batched numpy; the HIP kernel behind `VecDMFB.shield` (include/dmfb_vec.h: dmfb_vec_shield,
marl_dmfb_amd/csrc/dmfb_shield.h) equals it bit for bit.

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
goal cells are drawn with squared distance > 2 (dmfb.py:207-226)."""
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
    """The candidate actions of every droplet, first to last: int64 (E, n, 5)."""
    q = np.asarray(q, np.float32)
    E, n = q.shape[:2]
    picked = np.asarray(picked, np.int64).reshape(E, n)
    nan = np.isnan(q)
    act = np.broadcast_to(np.arange(N_ACTIONS), q.shape)
    # lexsort: the last key is the primary one -- numbers before NaNs, then descending q, then the lower action
    order = np.lexsort((act, -np.where(nan, np.float32(0), q), nan), axis=-1)
    in_range = (picked >= 0) & (picked < N_ACTIONS)
    rest = order != picked[:, :, None]                        # the pick leaves the q order (stable) ...
    shifted = np.take_along_axis(order, np.argsort(~rest, axis=-1, kind='stable'), axis=-1)
    with_pick = np.concatenate([picked[:, :, None], shifted[:, :, :N_ACTIONS - 1]], axis=-1)   # ... and goes first
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
