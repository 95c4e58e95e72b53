"""Shared by tests/test_shield_host.py and tests/test_gpu_shield.py: the seeded noisy goal-seeking Q, random conflict-free
states and the lock-step driver of the CPU oracle under the shield rule."""
import numpy as np

from marl_dmfb_amd.shield import DELTAS, shield_reference
from oracle.dmfb_oracle import DmfbOracle

# the five configurations of the shield's CPU check: constructor arguments of the oracle, and whether health is redrawn
CONFIGS = {
    '10x10_4d': (dict(width=10, length=10, n_agents=4), None),
    '10x10_4d_2b_health': (dict(width=10, length=10, n_agents=4, n_blocks=2, with_maps=True), (0.3, 1.0)),
    '10x10_4d_nostall': (dict(width=10, length=10, n_agents=4, stall=False), None),
    '12x12_10d_3b_degrade': (dict(width=12, length=12, n_agents=10, n_blocks=3, b_degrade=True), None),
    '20x20_10d': (dict(width=20, length=20, n_agents=10), None),
}
N_CHIPS = 48


def cheb(a, b):
    return np.abs(np.asarray(a, np.int64) - np.asarray(b, np.int64)).max(-1)


def goal_q(rng, width, length, pos, goals, noise=0.5):
    """float32 (E, n, 5): minus the Manhattan distance to the goal after the (clamped) move, plus seeded noise."""
    cells = pos[:, :, None, :].astype(np.int64) + DELTAS[None, None]
    cells[..., 0] = np.clip(cells[..., 0], 0, width - 1)
    cells[..., 1] = np.clip(cells[..., 1], 0, length - 1)
    dist = np.abs(cells - goals[:, :, None, :]).sum(-1)
    return (-dist + noise * rng.standard_normal(dist.shape)).astype(np.float32)


def noisy_picks(rng, q, greedy=0.9):
    """The arg-max with probability `greedy`, a uniform action otherwise: int32 (E, n)."""
    pick = q.argmax(-1)
    rand = rng.integers(0, 5, pick.shape)
    return np.where(rng.random(pick.shape) < greedy, pick, rand).astype(np.int32)


def play_oracle(name, shielded, seed=0):
    """One whole episode length of lock-steps on N_CHIPS oracle chips, terminated chips reset on the spot.  Returns the summed
    constraints, the most constraints of one lock-step, the overridden picks and the chips ever flagged unsafe."""
    kw, health = CONFIGS[name]
    W, L, n = kw['width'], kw['length'], kw['n_agents']
    stall = kw.get('stall', True)
    rng = np.random.default_rng(seed)
    ora = DmfbOracle(fov=5, n_envs=N_CHIPS, seed=seed + 1, **kw)
    ora.reset()
    if health is not None:
        ora.set_map('health', rng.uniform(health[0], health[1], (N_CHIPS, W, L)))
    total = worst = overrides = unsafe = 0
    for _ in range(ora.max_step):
        st = ora.get_state()
        goals = ora.get_task()[1]
        blocks = ora.get_blocks() if kw.get('n_blocks') else None
        q = goal_q(rng, W, L, st['pos'], goals)
        act = noisy_picks(rng, q)
        if shielded:
            act, ov, un = shield_reference(W, L, st['pos'], st['dist'] == 0, blocks, stall, q, act)
            overrides += int(ov.sum())
            unsafe += int(un.sum())
        _, dones, cons, _ = ora.step(act, uniforms=rng.random((N_CHIPS, n)))
        total += int(cons.sum())
        worst = max(worst, int(cons.max()))
        term = dones.all(axis=1)
        if term.any():
            ora.reset(mask=term.astype(np.uint8))
    return total, worst, overrides, unsafe


def random_states(rng, count, width, length, n, crowded=False, tries=200):
    """`count` random states of n droplets on a width x length chip: int64 (count, n, 2).  Conflict-free (every pair 2 apart)
    unless `crowded`, where any distinct cells will do.  Droplets are placed one after the other, each on a random cell that
    keeps its distance from those before it; a chip that jams starts again."""
    dmin = 1 if crowded else 2
    out = np.zeros((count, n, 2), np.int64)
    for e in range(count):
        for _ in range(tries):
            cells = []
            for _ in range(n):
                for _ in range(tries):
                    c = np.array([rng.integers(0, width), rng.integers(0, length)])
                    if all(cheb(c, o) >= dmin for o in cells):
                        cells.append(c)
                        break
                else:
                    break
            if len(cells) == n:
                break
        else:
            raise RuntimeError('no state found: chip too small for %d droplets' % n)
        out[e] = np.stack(cells)
    return out


def kernel_case_state(rng, E, n, W, L, nb, crowded):
    """Positions, goals and blocks (or None) of one kernel-against-reference case.  Half the chips of a crowded case are
    conflict-free all the same; a quarter of the droplets sit on their goals; on a 255 x 255 chip the droplets (and most
    blocks) gather within a few cells of the far or the near edge of either axis, corners included."""
    if W == 255:
        side = 6 if n <= 4 else 12
        pos = random_states(rng, E, side, side, n, crowded=crowded)
        far = rng.integers(0, 2, (E, 1, 2)).astype(bool)
        pos = np.where(far, 254 - pos, pos)
    else:
        pos = random_states(rng, E, W, L, n, crowded=crowded)
        if crowded and E > 1:
            pos[:E // 2] = random_states(rng, E // 2, W, L, n)
    goals = np.stack([rng.integers(0, W, (E, n)), rng.integers(0, L, (E, n))], -1)
    goals = np.where((rng.random((E, n)) < 0.25)[..., None], pos, goals)
    blocks = None
    if nb:
        x0, y0 = rng.integers(0, W - 1, (E, nb)), rng.integers(0, L - 1, (E, nb))
        if W == 255:
            near = rng.random((E, nb)) < 0.8
            x0 = np.where(near, np.where(rng.random((E, nb)) < 0.5, 253 - rng.integers(0, 12, (E, nb)), rng.integers(0, 12, (E, nb))), x0)
            y0 = np.where(near, np.where(rng.random((E, nb)) < 0.5, 253 - rng.integers(0, 12, (E, nb)), rng.integers(0, 12, (E, nb))), y0)
        blocks = np.stack([x0, x0 + 1, y0, y0 + 1], -1)
    return pos, goals, blocks


def kernel_case_rounds(rng, E, n):
    """Three rounds of (q, picks, active) for one state: q quantised to three values so that ties abound (NaNs in the last
    round), picks half arg-max and half random (some outside [0, 5) in the second round), every chip active in the first round
    and a random mask after it."""
    for rnd in range(3):
        q = (rng.integers(0, 3, (E, n, 5)) * 0.5).astype(np.float32)
        if rnd == 2:
            q[rng.random(q.shape) < 0.1] = np.nan
        picks = np.where(rng.random((E, n)) < 0.5, np.nan_to_num(q, nan=-1.0).argmax(-1), rng.integers(0, 5, (E, n))).astype(np.int32)
        if rnd == 1:
            odd = rng.random((E, n)) < 0.1
            picks[odd] = rng.choice([-1, 5, 9, -128], int(odd.sum()))
        active = (rng.random(E) < 0.8).astype(np.uint8) if rnd else np.ones(E, np.uint8)
        yield rnd, q, picks, active
