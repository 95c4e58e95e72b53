"""Shared by tests/test_meda_shield_host.py and tests/test_gpu_meda_shield.py: the seeded noisy goal-seeking Q of MEDA, random
states whose anchors keep their distance, the lock-step driver of the CPU oracle under the MEDA shield rule, and the injected
states and rounds of the kernel-against-reference cases."""
import numpy as np

from marl_dmfb_amd import plan
from marl_dmfb_amd.shield import MEDA_ACTIONS, meda_anchors, meda_shield_reference, meda_targets
from oracle.meda_oracle import MedaOracle

# the three configurations of the CPU check (constructor arguments of the oracle); each runs with and without a health map.
# The env, like the reference, admits (width // 15) * (length // 15) droplets at the most (meda.py:151-154), so neither it nor the
# oracle can be created for 20x20 / 2 droplets: that configuration plays on RuleChips below, the env's step and the reference's
# task acceptance rule in plain Python.
CONFIGS = {
    '30x30_4d': dict(width=30, length=30, n_agents=4),
    '20x20_2d': dict(width=20, length=20, n_agents=2),
    '30x60_8d': dict(width=30, length=60, n_agents=8),
}
HEALTH = (0.6, 1.0)
N_CHIPS = 32


def d2(a, b):
    return ((np.asarray(a, np.int64) - np.asarray(b, np.int64)) ** 2).sum(-1)


def pairwise_clear(pts):
    """bool (E,): every two of the n points (E, n, 2) are at least 6 apart (not `near`)."""
    n = pts.shape[1]
    d = d2(pts[:, :, None], pts[:, None]) + 36 * np.eye(n, dtype=np.int64)
    return (d >= 36).all((1, 2))


def goal_q(rng, width, length, pos, goals, noise=0.5):
    """float32 (E, n, 9): minus the Euclidean distance to the goal after the (clamped) move, plus seeded noise."""
    dist = np.sqrt(d2(meda_targets(width, length, pos), np.asarray(goals, np.int64)[:, :, None]))
    return (-dist + noise * rng.standard_normal(dist.shape)).astype(np.float32)


def noisy_picks(rng, q, greedy=0.9):
    """The arg-max with probability `greedy`, a uniform action otherwise: int32 (E, n)."""
    pick = q.argmax(-1)
    rand = rng.integers(0, MEDA_ACTIONS, pick.shape)
    return np.where(rng.random(pick.shape) < greedy, pick, rand).astype(np.int32)


class RuleChips:
    """E chips with the oracle's interface as far as play_oracle uses it, for a configuration the oracle refuses: tasks by the
    reference's acceptance rule (addTask / _genLegalDroplet, meda.py:175-233: centres uniform in the valid range, starts
    pairwise 9 apart, goals pairwise 9 apart, no goal box overlapping its own start box) and the step of plan._meda_env_step."""

    def __init__(self, width, length, n_agents, n_envs, seed):
        self.W, self.L, self.n, self.E = width, length, n_agents, n_envs
        self.max_step = width + length
        self.rng = np.random.default_rng(seed)
        self.health = None
        self.pos = np.zeros((n_envs, n_agents, 2), np.int64)
        self.goals, self.status, self.steps = self.pos.copy(), np.zeros((n_envs, n_agents), np.uint8), np.zeros(n_envs, np.int64)

    def _draw(self, earlier, own=None):
        while True:
            c = np.array([self.rng.integers(2, self.L - 2), self.rng.integers(2, self.W - 2)])
            if all(d2(c, o) >= 81 for o in earlier) and (own is None or not (abs(own - c) <= 4).all()):
                return c

    def reset(self, mask=None):
        for e in range(self.E):
            if mask is not None and not mask[e]:
                continue
            for i in range(self.n):
                self.pos[e, i] = self._draw(self.pos[e, :i])
                self.goals[e, i] = self._draw(self.goals[e, :i], self.pos[e, i])
            self.status[e], self.steps[e] = 0, 0

    def set_map(self, which, arr):
        self.health = np.asarray(arr, np.float64)

    def get_state(self):
        return dict(pos=self.pos.copy(), status=self.status.copy())

    def get_task(self):
        return None, self.goals.copy()

    def step(self, actions, uniforms):
        fail, dones = np.zeros(self.E), np.zeros((self.E, self.n), np.uint8)
        for e in range(self.E):
            p, d = [tuple(x) for x in self.pos[e].tolist()], [bool(x) for x in self.status[e]]
            g = [tuple(x) for x in self.goals[e].tolist()]
            fail[e] = plan._meda_env_step(self.W, self.L, p, g, d, actions[e].tolist(), uniforms[e].tolist(),
                                          None if self.health is None else self.health[e])
            self.pos[e], self.status[e] = p, d
            self.steps[e] += 1
            dones[e] = 1 if self.steps[e] >= self.max_step else self.status[e]
        return None, dones, fail, None


def play_oracle(name, shielded, health, seed=0):
    """One whole episode length of lock-steps on N_CHIPS oracle chips with tasks of the oracle's own reset, terminated chips
    reset on the spot.  Returns the (chip, lock-step) pairs with a proximity penalty, the summed penalty (`fail` is -0.6 per
    droplet of a near pair), the overridden picks and the chips ever flagged unsafe."""
    kw = CONFIGS[name]
    W, L, n = kw['width'], kw['length'], kw['n_agents']
    rng = np.random.default_rng(seed)
    if n > (W // 15) * (L // 15):
        ora = RuleChips(n_envs=N_CHIPS, seed=seed + 1, **kw)
    else:
        ora = MedaOracle(fov=19, n_envs=N_CHIPS, seed=seed + 1, with_maps=health, **kw)
    ora.reset()
    if health:
        ora.set_map('health', rng.uniform(HEALTH[0], HEALTH[1], (N_CHIPS, W, L)))
    events = overrides = unsafe = 0
    penalty = 0.0
    for _ in range(ora.max_step):
        st = ora.get_state()
        goals = ora.get_task()[1]
        q = goal_q(rng, W, L, st['pos'], goals)
        act = noisy_picks(rng, q)
        if shielded:
            act, ov, un = meda_shield_reference(W, L, st['pos'], goals, st['status'], q, act)
            overrides += int(ov.sum())
            unsafe += int(un.sum())
        _, dones, fail, _ = ora.step(act, uniforms=rng.random((N_CHIPS, n)))
        events += int((fail != 0.0).sum())
        penalty += float(-fail.sum())
        term = dones.all(axis=1)
        if term.any():
            ora.reset(mask=term.astype(np.uint8))
    return events, penalty, overrides, unsafe


def random_safe_states(rng, count, width, length, n, tries=400):
    """`count` random states of n droplets whose anchors are pairwise 6 apart: (pos, goals int64 (count, n, 2), done bool
    (count, n)).  Every droplet is, with equal chance, free anywhere, free one move from its goal disc, inside the disc but not
    done, or done on its goal; a chip that jams starts again."""
    pos, goals, done = (np.zeros((count, n, 2), np.int64), np.zeros((count, n, 2), np.int64), np.zeros((count, n), bool))
    lo, hx, hy = 2, length - 3, width - 3

    def centre():
        return np.array([rng.integers(lo, hx + 1), rng.integers(lo, hy + 1)])

    def near_goal(g, d2_min, d2_max):
        for _ in range(tries):
            c = g + rng.integers(-6, 7, 2)
            c = np.array([min(max(c[0], lo), hx), min(max(c[1], lo), hy)])
            if d2_min <= d2(c, g) < d2_max:
                return c
        return None

    for e in range(count):
        for _ in range(tries):
            chip = []
            for _ in range(n):
                for _ in range(tries):
                    g, kind = centre(), int(rng.integers(0, 4))
                    p = (centre(), near_goal(g, 16, 50), near_goal(g, 0, 16), g)[kind]
                    if p is None:
                        continue
                    a = g if kind >= 2 else p
                    if kind < 2 and d2(p, g) < 16:
                        continue                         # a free droplet is outside its disc
                    if all(d2(a, o) >= 36 for o in (c[3] for c in chip)):
                        chip.append((p, g, kind == 3, a))
                        break
                else:
                    break
            if len(chip) == n:
                break
        else:
            raise RuntimeError('no state found: chip too small for %d droplets' % n)
        pos[e], goals[e], done[e] = np.stack([c[0] for c in chip]), np.stack([c[1] for c in chip]), [c[2] for c in chip]
    return pos, goals, done


# ---------------------------------------------------------------------------------------------------- kernel cases (GPU)
def kernel_case_task(rng, E, n, W, L):
    """(starts, goals int32 (E, n, 2), first actions int32 (E, n)) of one kernel-against-reference case: set_task(starts, goals)
    and one step of the first actions (on healthy electrodes) leave a mix of free droplets, droplets inside their disc and done
    droplets.  Most centres are drawn within 9 of an earlier one, so that the droplets stand in packs; on the even chips every
    two centres are 6 apart all the same (where they fit), on the odd ones any distance will do, so that safe and unsafe chips
    occur.  On a 128-wide chip every other chip gathers within 12 of the far edge of both axes (the byte range), and some have a
    droplet in the far corner itself."""
    lo, hx, hy = 2, L - 3, W - 3
    starts, goals = np.zeros((E, n, 2), np.int64), np.zeros((E, n, 2), np.int64)
    first = np.full((E, n), MEDA_ACTIONS - 1, np.int64)
    for e in range(E):
        far = W >= 128 and e % 2 == 1
        x0, y0 = (hx - 12, hy - 12) if far else (lo, lo)
        placed = []
        for i in range(n):
            for k in range(200):
                if placed and rng.random() < 0.8:
                    c = placed[rng.integers(len(placed))] + rng.integers(-9, 10, 2)
                    c = np.array([min(max(c[0], x0), hx), min(max(c[1], y0), hy)])
                else:
                    c = np.array([rng.integers(x0, hx + 1), rng.integers(y0, hy + 1)])
                if e % 4 >= 2 or all(d2(c, o) >= 36 for o in placed):
                    break
            corner = far and i == 0 and e % 4 == 1
            if corner:
                c = np.array([hx, hy])
            placed.append(c)
            g = np.array([rng.integers(lo, hx + 1), rng.integers(lo, hy + 1)])
            kind = int(rng.integers(0, 4))
            if corner:
                g, kind = np.array([lo, lo]), 0           # it stays in the corner, free
            if kind == 1:       # starts inside the disc of a goal next to it: done after the first step
                g = np.array([min(max(c[0] - 2, lo), hx), min(max(c[1] - 1, lo), hy)])
            elif kind == 2:     # 5 from the goal, first action towards it: inside the disc after the first step, not done
                if c[0] - 5 >= lo:
                    g, first[e, i] = np.array([c[0] - 5, c[1]]), 3
                elif c[0] + 5 <= hx:
                    g, first[e, i] = np.array([c[0] + 5, c[1]]), 1
            starts[e, i], goals[e, i] = c, g
    return starts.astype(np.int32), goals.astype(np.int32), first.astype(np.int32)


def kernel_case_rounds(rng, E, n):
    """Three rounds of (q, picks, active) for one state: q quantised to three values so that ties abound (NaNs in the last
    round), picks half arg-max and half random (some outside [0, 9) in the second round), every chip active in the first round
    and a random mask after it."""
    A = MEDA_ACTIONS
    for rnd in range(3):
        q = (rng.integers(0, 3, (E, n, A)) * 0.5).astype(np.float32)
        if rnd == 2:
            q[rng.random(q.shape) < 0.1] = np.nan
        picks = np.where(rng.random((E, n)) < 0.5, np.nan_to_num(q, nan=-1.0).argmax(-1), rng.integers(0, A, (E, n))).astype(np.int32)
        if rnd == 1:
            odd = rng.random((E, n)) < 0.25
            picks[odd] = rng.choice([-1, 9, 15, 16, -128], int(odd.sum()))
        active = (rng.random(E) < 0.8).astype(np.uint8) if rnd else np.ones(E, np.uint8)
        yield rnd, q, picks, active


def next_anchors(pos, goals, done):
    """Anchors of a state (one chip: pos / goals lists of n centres, done list of n flags) as int64 (1, n, 2)."""
    return meda_anchors(np.asarray(pos, np.int64)[None], np.asarray(goals, np.int64)[None], np.asarray(done, bool)[None])[1]
