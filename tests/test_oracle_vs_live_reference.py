"""Differential test of the CPU oracles against the reference on fresh seeded inputs, beyond what the other
committed goldens hold: random tasks, actions, draws, health maps and blocks drawn here from
`np.random.default_rng(seed)` for every case of the seed list.

The reference's side was recorded by running the live reference on exactly these inputs
(tools/oracle/gen_live_golden.py -> tests/golden/live_*.npz: observations, rewards, dones, constraints,
success and the usage map after every step).  The oracle is driven with the same inputs and must reproduce
every recorded value bit for bit."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _load(name, cfg):
    g = dict(np.load(os.path.join(GOLDEN, name + '.npz')))
    assert g['cfg'].tolist() == [int(v) for v in cfg], 'golden %s was recorded for another case' % name
    return g


@pytest.mark.parametrize('W,L,n,fov,stall,nb,seed', [
    (10, 10, 4, 9, True, 0, 1), (10, 10, 4, 9, False, 0, 2), (14, 11, 5, 7, True, 3, 3), (20, 20, 10, 9, True, 6, 4),
    (50, 50, 10, 9, True, 0, 5), (9, 13, 3, 5, True, 2, 6), (10, 10, 4, 8, True, 0, 7)])
def test_dmfb_oracle_matches_live_reference(W, L, n, fov, stall, nb, seed):
    from oracle.dmfb_oracle import DmfbOracle
    g = _load('live_dmfb_%dx%d_%dd_fov%d_%s_%db_s%d' % (W, L, n, fov, 'stall' if stall else 'nostall', nb, seed),
              (W, L, n, fov, stall, nb, seed))
    rng = np.random.default_rng(seed)
    ora = DmfbOracle(W, L, n, n_blocks=nb, fov=fov, stall=stall, n_envs=1, with_maps=True)
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
        ora.set_map('health', h[None])
        ora.set_map('usage', np.zeros((1, W, L)))
        if nb:
            ora.set_blocks(np.array(blocks, np.int32)[None])
        ora.set_task(pts[:n][None], pts[n:][None])
        np.testing.assert_array_equal(ora.observe()[0], g['e%d_obs0' % ep])
        steps = len(g['e%d_r' % ep])
        for t in range(steps):
            acts = rng.integers(0, 5, n)
            u = rng.random(n)
            ro, do, co, so = ora.step(np.array(acts, np.int32)[None], u[None])
            np.testing.assert_array_equal(_bits(ro[0]), _bits(g['e%d_r' % ep][t]))
            np.testing.assert_array_equal(do[0], g['e%d_d' % ep][t])
            assert co[0] == g['e%d_c' % ep][t] and so[0] == g['e%d_s' % ep][t]
            np.testing.assert_array_equal(ora.observe()[0], g['e%d_obs' % ep][t])
            np.testing.assert_array_equal(ora.get_map('usage')[0], g['e%d_usage' % ep][t])
        # the recording stops where every droplet is done past W + L steps, or at the step limit
        assert steps == 2 * (W + L) + 3 or (do[0].all() and steps - 1 > W + L)


@pytest.mark.parametrize('W,L,n,fov,version,seed', [
    (30, 30, 4, 19, 0, 1), (30, 60, 8, 19, 2, 2), (45, 30, 6, 9, 0, 3), (60, 75, 14, 19, 2, 4), (80, 80, 10, 19, 0, 5)])
def test_meda_oracle_matches_live_reference(W, L, n, fov, version, seed):
    from oracle.meda_oracle import MedaOracle
    g = _load('live_meda_v%d_%dx%d_%dd_fov%d_s%d' % (version, W, L, n, fov, seed), (W, L, n, fov, version, seed))
    rng = np.random.default_rng(seed)
    ora = MedaOracle(W, L, n, fov=fov, n_envs=1, with_maps=True, version=version)
    for ep in range(4):
        pts = np.stack([rng.integers(2, L - 2, 2 * n), rng.integers(2, W - 2, 2 * n)], axis=1)
        h = np.where(rng.random((W, L)) < 0.5, 1.0, rng.random((W, L)) * 0.7 + 0.3)
        ora.set_map('health', h[None]); ora.set_map('usage', np.zeros((1, W, L)))
        ora.set_task(pts[:n][None], pts[n:][None])
        np.testing.assert_array_equal(ora.observe()[0], g['e%d_obs0' % ep])
        assert len(g['e%d_r' % ep]) == W + L + 2
        for t in range(W + L + 2):
            acts = rng.integers(0, 9, n)
            u = rng.random(n)
            ro, do, fo, so = ora.step(np.array(acts, np.int32)[None], u[None])
            np.testing.assert_array_equal(_bits(ro[0]), _bits(g['e%d_r' % ep][t]))
            np.testing.assert_array_equal(do[0], g['e%d_d' % ep][t])
            np.testing.assert_array_equal(_bits(fo[0] + 0.0), _bits(g['e%d_c' % ep][t]))
            assert so[0] == g['e%d_s' % ep][t]
            np.testing.assert_array_equal(ora.observe()[0], g['e%d_obs' % ep][t])
            np.testing.assert_array_equal(ora.get_map('usage')[0], g['e%d_usage' % ep][t])
