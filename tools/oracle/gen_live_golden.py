"""Record the reference's side of tests/test_oracle_vs_live_reference.py (container-only).

For every case of that test this runs the real reference env (env/DMFB/dmfb.py, env/MEDA/meda.py) on the
seeded inputs the test draws -- tasks, blocks, health maps, actions and per-agent uniforms, in the same order
from the same `np.random.default_rng(seed)` -- and writes what the reference returned to
tests/golden/live_<dmfb|meda>_<case>.npz:
  e<k>_obs0          the observation of restart()                      (int8, n x ...)
  e<k>_obs           the observation after every step                  (int8, steps x n x ...)
  e<k>_r             per-agent float64 rewards                          (steps x n)
  e<k>_d             per-agent dones                                    (steps x n)
  e<k>_c, e<k>_s     constraints (float64) and success of every step    (steps)
  e<k>_usage         the usage map after every step                     (uint8 / uint16, steps x W x L)
The number of steps of an episode is where the test's loop stopped (all droplets done past W + L steps, or the
step limit).  Every narrowed array is checked to round-trip to the reference's values exactly.

Run:  python tools/oracle/gen_live_golden.py
"""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'tests', 'golden')

# (W, L, n, fov, stall, n_blocks, seed) and (W, L, n, fov, version, seed): the parametrisation of the test
DMFB_CASES = [(10, 10, 4, 9, True, 0, 1), (10, 10, 4, 9, False, 0, 2), (14, 11, 5, 7, True, 3, 3), (20, 20, 10, 9, True, 6, 4),
              (50, 50, 10, 9, True, 0, 5), (9, 13, 3, 5, True, 2, 6), (10, 10, 4, 8, True, 0, 7)]
MEDA_CASES = [(30, 30, 4, 19, 0, 1), (30, 60, 8, 19, 2, 2), (45, 30, 6, 9, 0, 3), (60, 75, 14, 19, 2, 4), (80, 80, 10, 19, 0, 5)]


def dmfb_name(W, L, n, fov, stall, nb, seed):
    return 'live_dmfb_%dx%d_%dd_fov%d_%s_%db_s%d' % (W, L, n, fov, 'stall' if stall else 'nostall', nb, seed)


def meda_name(W, L, n, fov, version, seed):
    return 'live_meda_v%d_%dx%d_%dd_fov%d_s%d' % (version, W, L, n, fov, seed)


def narrow(a, dtype):
    a = np.asarray(a)
    b = a.astype(dtype)
    assert np.array_equal(b.astype(a.dtype), a), 'values do not fit %s' % np.dtype(dtype).name
    return b


def usage_maps(maps):
    a = np.asarray(maps, dtype=np.float64)
    return narrow(a, np.uint8 if a.max() <= 255 else np.uint16)


def save(name, cfg, episodes):
    out = {'cfg': np.asarray(cfg, dtype=np.int64)}
    for k, ep in enumerate(episodes):
        for key, v in ep.items():
            out['e%d_%s' % (k, key)] = v
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **out)
    print('%s: %d episodes, %d steps, %.0f kB' % (name, len(episodes), sum(len(e['r']) for e in episodes), os.path.getsize(path) / 1e3))


def record_dmfb(rd, Q, W, L, n, fov, stall, nb, seed):
    rng = np.random.default_rng(seed)
    env = rd.DMFBenv(W, L, n, nb, fov=fov, stall=stall)
    rmgr = env.routing_manager
    episodes = []
    for ep in range(6):
        pts = np.stack([rng.integers(0, W, 2 * n), rng.integers(0, L, 2 * n)], axis=1)
        while len({(x, y) for x, y in pts[:n]}) < n:
            pts = np.stack([rng.integers(0, W, 2 * n), rng.integers(0, L, 2 * n)], axis=1)
        blocks = []
        while len(blocks) < nb:
            x0, y0 = int(rng.integers(0, W - 3)), int(rng.integers(0, L - 3))
            if any(x0 <= px <= x0 + 1 and y0 <= py <= y0 + 1 for px, py in pts):
                continue
            if any(not (x0 > b[1] or b[0] > x0 + 1) and not (y0 > b[3] or b[2] > y0 + 1) for b in blocks):
                continue
            blocks.append((x0, x0 + 1, y0, y0 + 1))
        h = np.where(rng.random((W, L)) < 0.4, 1.0, rng.random((W, L)) * 0.8 + 0.2)
        rmgr.blocks = [rd.Block(*b) for b in blocks]
        rmgr.m_health = h.copy()
        rmgr.m_usage = np.zeros((W, L))
        rmgr.starts, rmgr.ends = pts[:n].copy(), pts[n:].copy()
        obs0 = narrow(np.stack(env.restart()), np.int8)
        rec = {'obs': [], 'r': [], 'd': [], 'c': [], 's': [], 'usage': []}
        for t in range(2 * (W + L) + 3):
            acts = [int(a) for a in rng.integers(0, 5, n)]
            drawing = [not (stall and rmgr.distances[i] == 0) for i in range(n)]
            u = rng.random(n)
            Q.feed([u[i] for i in range(n) if drawing[i]])
            o, r, d, info = env.step(list(acts))
            rec['obs'].append(narrow(np.stack(o), np.int8))
            rec['r'].append(np.array([r[a] for a in env.agents], dtype=np.float64))
            rec['d'].append(np.array([d[a] for a in env.agents], dtype=bool))
            rec['c'].append(float(info['constraints']))
            rec['s'].append(bool(info['success']))
            rec['usage'].append(np.array(rmgr.m_usage, dtype=np.float64))
            if all(d[a] for a in env.agents) and t > W + L:
                break
        episodes.append(dict(obs0=obs0, obs=np.stack(rec['obs']), r=np.stack(rec['r']), d=np.stack(rec['d']),
                             c=np.array(rec['c'], np.float64), s=np.array(rec['s'], bool), usage=usage_maps(rec['usage'])))
    save(dmfb_name(W, L, n, fov, stall, nb, seed), (W, L, n, fov, int(stall), nb, seed), episodes)


def record_meda(rm, Q, W, L, n, fov, version, seed):
    rng = np.random.default_rng(seed)
    cls = rm.MEDAEnv_v0_2 if version == 2 else rm.MEDAEnv
    env = cls(W, L, n, fov=fov)
    mgr = env.routing_manager
    episodes = []
    for ep in range(4):
        pts = np.stack([rng.integers(2, L - 2, 2 * n), rng.integers(2, W - 2, 2 * n)], axis=1)
        h = np.where(rng.random((W, L)) < 0.5, 1.0, rng.random((W, L)) * 0.7 + 0.3)
        mgr.starts = [rm.Droplet(x - 2, x + 2, y - 2, y + 2) for x, y in pts[:n]]
        mgr.destinations = [rm.Droplet(x - 2, x + 2, y - 2, y + 2) for x, y in pts[n:]]
        env.m_health, env.m_usage, env.fails = h.copy(), np.zeros((W, L)), 0
        obs0 = np.stack(env.restart()).astype(np.int8)   # the test compares the reference's observation cast to int8
        rec = {'obs': [], 'r': [], 'd': [], 'c': [], 's': [], 'usage': []}
        for t in range(W + L + 2):
            acts = [int(a) for a in rng.integers(0, 9, n)]
            drawing = [(not mgr.status[i]) and not (mgr.distances[i] < 4) for i in range(n)]
            u = rng.random(n)
            Q.feed([u[i] for i in range(n) if drawing[i]])
            o, r, d, info = env.step(list(acts))
            rec['obs'].append(np.stack(o).astype(np.int8))
            rec['r'].append(np.array([r[a] for a in env.agents], dtype=np.float64))
            rec['d'].append(np.array([d[a] for a in env.agents], dtype=bool))
            rec['c'].append(float(info['constraints']) + 0.0)
            rec['s'].append(bool(info['success']))
            rec['usage'].append(np.array(env.m_usage, dtype=np.float64))
        episodes.append(dict(obs0=obs0, obs=np.stack(rec['obs']), r=np.stack(rec['r']), d=np.stack(rec['d']),
                             c=np.array(rec['c'], np.float64), s=np.array(rec['s'], bool), usage=usage_maps(rec['usage'])))
    save(meda_name(W, L, n, fov, version, seed), (W, L, n, fov, version, seed), episodes)


def main():
    ref_shim.install()
    Q = ref_shim.DrawQueue()
    original = random.random
    ref_shim.patch_random(Q)
    try:
        from env.DMFB import dmfb as rd
        from env.MEDA import meda as rm
        for case in DMFB_CASES:
            record_dmfb(rd, Q, *case)
        for case in MEDA_CASES:
            record_meda(rm, Q, *case)
    finally:
        random.random = original


if __name__ == '__main__':
    main()
