"""Records tests/golden/td_block_bits.npz: what the TD block of the library in use (vdn_td_forward_sums, vdn_td_backward, their packed
forms and the two lambda entry points) computes for the seeded cases of tests/test_gpu_td_block_bits.py (the inputs are regenerated
from the seeds there; only the outputs are stored).  The committed file was recorded on an MI355X with the build of the commit
BEFORE the one-step and lambda kernels were folded into one row rule (marl_dmfb_amd/csrc/vdn_ops.hip); run it again only from a
build whose bits are meant to become the new record.

    python tools/record_td_block_fixture.py OUT.npz        (MARL_DMFB_VARIANT_VDN_OPS=_tag picks a variant library)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np

import test_gpu_td_block_bits as T


def main(path):
    rec = {}
    for key, run in T.all_runs().items():
        out = run()
        again = run()                     # fixed-order sums: a second launch gives the same words, or the record would be a coin toss
        for f in T.fields(key):
            assert np.array_equal(out[f].view(np.int32), again[f].view(np.int32)), (key, f)
            assert key.endswith('_bad') or np.isfinite(out[f]).all(), (key, f)
            rec[key + '.' + f] = out[f]
    np.savez_compressed(path, **rec)
    print('recorded', path, os.path.getsize(path), 'bytes;', len(rec), 'arrays of', len(T.all_runs()), 'cases')


if __name__ == '__main__':
    main(sys.argv[1])
