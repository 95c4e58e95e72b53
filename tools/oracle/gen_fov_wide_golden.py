"""Generate the learn goldens of the two wide fields of view by RUNNING THE REFERENCE (container-only), with
gen_vdn_golden.gen_learn: fov 11 with 4 droplets (od 24) on 14x14, B = 6, and fov 13 with 3 droplets (od 32) on 16x16, B = 5.

  tests/golden/fovlearn_4d_od24_fov11.npz
  tests/golden/fovlearn_3d_od32_fov13.npz

gen_learn prints the valid steps per episode: they must differ, with padded steps in some (checked here).
Run: python tools/oracle/gen_fov_wide_golden.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_vdn_golden as G  # noqa: E402

CASES = [('4d_od24_fov11', 4, 14, 11, 6), ('3d_od32_fov13', 3, 16, 13, 5)]
SEED = 13   # as the fov 5 / 7 goldens

if __name__ == '__main__':
    for tag, n, W, fov, B in CASES:
        G.gen_learn(tag, n, W, W, fov, B=B, seed=SEED)
        src, dst = os.path.join(G.OUT, 'vdn_learn_%s.npz' % tag), os.path.join(G.OUT, 'fovlearn_%s.npz' % tag)
        os.replace(src, dst)
        g = np.load(dst)
        lens = (1 - g['padded'][:, :, 0].astype(int)).sum(1)
        T = g['padded'].shape[1]
        assert len(set(lens.tolist())) >= 3 and (lens < T).any(), lens
        assert int(g['cfg'][4]) == (24 if n == 4 else 32)
        print(os.path.basename(dst), 'T=%d lengths=%s bytes=%d' % (T, lens.tolist(), os.path.getsize(dst)))
