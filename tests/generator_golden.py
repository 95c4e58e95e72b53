"""Shared by tests/test_generator_golden.py (CPU oracles) and tests/test_gpu_generator_golden.py (HIP envs): the
recordings of what the reference's own task, block and degrade-map generators accepted on the build's candidate stream
(tools/oracle/gen_generator_golden.py -> tests/golden/gen_*.npz; layout in that script's docstring), and the walk that
compares an env object with them generation by generation."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
N_CHIPS = 64

# the committed cases, by file name: a recording that goes missing fails the tests instead of shrinking them
DMFB_FILES = ['gen_dmfb_10x10_4d_fov9_0b_s7', 'gen_dmfb_10x10_4d_fov9_4b_s2', 'gen_dmfb_10x10_4d_fov9_5b_s1',
              'gen_dmfb_10x10_4d_fov9_6b_s6', 'gen_dmfb_12x9_3d_fov7_2b_s3', 'gen_dmfb_20x20_10d_fov9_12b_deg10_s4',
              'gen_dmfb_50x50_10d_fov9_0b_deg50_s5']
MEDA_FILES = ['gen_meda_v0_30x30_4d_fov19_s11', 'gen_meda_v0_45x30_6d_fov9_s13', 'gen_meda_v0_80x80_10d_fov19_deg10_s14',
              'gen_meda_v2_30x60_8d_fov19_s12']

# the autoreset walks: the case, and steps enough for second episodes (DMFB: past max_step = 40, which ends every first one)
DMFB_AUTORESET, DMFB_AUTORESET_STEPS = 'gen_dmfb_10x10_4d_fov9_4b_s2', 44
MEDA_AUTORESET, MEDA_AUTORESET_STEPS = 'gen_meda_v0_30x30_4d_fov19_s11', 22


def committed(kind):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'gen_%s_*.npz' % kind)))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def dmfb_kwargs(g):
    W, L, n, fov, nb, deg = (int(v) for v in g['cfg'])
    return dict(width=W, length=L, n_agents=n, n_blocks=nb, fov=fov, b_degrade=bool(deg), per_degrade=float(g['per_degrade']),
                n_envs=N_CHIPS, seed=int(g['seed']))


def meda_kwargs(g):
    W, L, n, fov, version, deg = (int(v) for v in g['cfg'])
    return dict(width=W, length=L, n_agents=n, fov=fov, version=version, b_degrade=bool(deg),
                per_degrade=float(g['per_degrade']), n_envs=N_CHIPS, seed=int(g['seed']))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def check_generation(B, g, p, blocks):
    """Env object `B` (oracle or HIP adapter: get_task / get_blocks / get_map as numpy) against generation `p` of `g`:
    tasks and blocks as integers, the degrade map as float64 bit patterns (the map of generation 0 until a new one)."""
    s, e = B.get_task()
    np.testing.assert_array_equal(np.asarray(s, np.int64), g['p%d_starts' % p].astype(np.int64), err_msg='starts, generation %d' % p)
    np.testing.assert_array_equal(np.asarray(e, np.int64), g['p%d_ends' % p].astype(np.int64), err_msg='ends, generation %d' % p)
    if blocks:
        b = np.asarray(B.get_blocks(), np.int64)
        want = g['p%d_blocks' % p].astype(np.int64)
        assert b.shape == want.shape, 'blocks per chip: %r, the reference drew %r' % (b.shape, want.shape)
        np.testing.assert_array_equal(b, want, err_msg='blocks, generation %d' % p)
    if 'p0_degrade' in g:
        want = g['p%d_degrade' % p] if 'p%d_degrade' % p in g else g['p0_degrade']
        got = B.get_map('degrade')[:len(want)]
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg='degrade map, generation %d' % p)


def walk_dmfb(B, g):
    """constructor, reset(), reset(new=True)  ==  the reference's __init__, refresh(), refresh(new=True)."""
    assert 'p2_degrade' in g or 'p0_degrade' not in g
    check_generation(B, g, 0, True)
    B.reset()
    check_generation(B, g, 1, True)
    B.reset(new=True)
    check_generation(B, g, 2, True)


def walk_meda(B, g):
    check_generation(B, g, 0, False)
    B.reset()
    check_generation(B, g, 1, False)
    B.reset()
    check_generation(B, g, 2, False)


# ---- the reset a terminated chip gets while the others go on (the step kernel's autoreset; reset(mask) on the oracle)
def dmfb_toward(st, ends, rng, greedy=0.8):
    """Mostly one cell towards the goal, along x or y at random (a droplet that always closes x first stays behind a block
    or a neighbour, and nearly every episode would run into the step limit at the same step)."""
    dx = ends[..., 0] - st['pos'][..., 0]
    dy = ends[..., 1] - st['pos'][..., 1]
    ax = np.where(dx > 0, 1, np.where(dx < 0, 2, 0))
    ay = np.where(dy < 0, 3, np.where(dy > 0, 4, 0))
    toward = np.where((rng.random(dx.shape) < 0.5) & (ax != 0) | (ay == 0), ax, ay)
    return np.where(rng.random(toward.shape) < greedy, toward, rng.integers(0, 5, toward.shape)).astype(np.int32)


def meda_toward(st, ends, rng, greedy=0.8):
    dx = ends[..., 0] - st['pos'][..., 0]
    dy = ends[..., 1] - st['pos'][..., 1]
    toward = np.where(np.abs(dx) >= np.abs(dy), np.where(dx > 0, 1, np.where(dx < 0, 3, 8)), np.where(dy > 0, 2, 0))
    return np.where(rng.random(toward.shape) < greedy, toward, rng.integers(0, 9, toward.shape)).astype(np.int32)


def _check_by_count(B, g, count, blocks, t):
    """A chip that has terminated c times holds the task (and blocks) of rng_ep = c; the recordings go up to rng_ep 2.
    The task and block streams do not depend on `new`, so generation 2 serves although the DMFB files recorded it
    from refresh(new=True)."""
    s, e = B.get_task()
    b = B.get_blocks() if blocks else None
    for p in range(3):
        m = count == p
        np.testing.assert_array_equal(s[m], g['p%d_starts' % p][m], err_msg='starts of rng_ep %d after step %d' % (p, t))
        np.testing.assert_array_equal(e[m], g['p%d_ends' % p][m], err_msg='ends of rng_ep %d after step %d' % (p, t))
        if blocks:
            np.testing.assert_array_equal(b[m], g['p%d_blocks' % p][m], err_msg='blocks of rng_ep %d after step %d' % (p, t))


def autoreset_walk(B, g, step, toward, blocks, steps):
    """Mostly-greedy actions; `step(actions)` steps `B`, resets the chips that terminated and returns which did.  After
    every step each chip must hold the recorded task of the generation it is in.  The actions depend on the seed and the
    state alone, so the walk is the same for the oracle and the HIP env; `steps` is chosen so that chips end their
    episodes at many different steps and, at the end, some are in generation 1 and some in generation 2."""
    rng = np.random.default_rng(int(g['seed']) + 1)
    count = np.zeros(N_CHIPS, np.int64)
    when = set()
    _check_by_count(B, g, count, blocks, -1)
    for t in range(steps):
        term = np.asarray(step(toward(B.get_state(), B.get_task()[1], rng)), np.int64)
        count += term
        if term.any():
            when.add(t)
        _check_by_count(B, g, count, blocks, t)
    assert (count == 1).sum() >= 4 and (count == 2).sum() >= 4 and len(when) >= 8, (np.bincount(count), sorted(when))
    return count
