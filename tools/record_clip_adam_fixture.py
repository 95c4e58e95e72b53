"""Records tests/golden/clip_adam_bits.npz: what vdn_clip_adam_step of the library in use computes for the seeded cases of
tests/test_gpu_clip_adam_bits.py (the inputs are regenerated from the seeds there; only outputs are stored: the small tensors whole,
of the large one a sample and a SHA-256).  The committed file was recorded on an MI355X with the build of the commit BEFORE the loads
of k_sqnorm_partials and k_clip_adam were moved ahead of their arithmetic (marl_dmfb_amd/csrc/vdn_ops.hip); run it again only from a
build whose bits are meant to become the new record.

    python tools/record_clip_adam_fixture.py OUT.npz        (MARL_DMFB_VARIANT_VDN_OPS=_tag picks a variant library)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np

import test_gpu_clip_adam_bits as T


def main(path):
    rec = {}
    for div, clip in T.CASES:
        res = T.run_case(div, clip)
        for q in T.QUANTITIES + ('norm',):
            assert np.isfinite(res[q]).all(), (div, clip, q)
        for name, a in T.pack(res).items():
            rec['%s__%s' % (T.case_key(div, clip), name)] = a
    np.savez_compressed(path, **rec)
    print('recorded', path, os.path.getsize(path), 'bytes;', len(rec), 'arrays')


if __name__ == '__main__':
    main(sys.argv[1])
