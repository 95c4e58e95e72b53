"""Records tests/golden/front_bwd_bits.npz: what crnn_mlp_backward and crnn_conv9_backward of the library in use compute for the
seeded cases of tests/test_gpu_front_bwd_bits.py (the inputs are regenerated from the seeds there; only the outputs are stored).
The committed file was recorded on an MI355X with the build of the commit BEFORE the loads of k_mlp_bwd and k_conv9_bwd_reduce were
reordered (marl_dmfb_amd/csrc/crnn_ops.hip); run it again only from a build whose bits are meant to become the new record.

    python tools/record_front_bwd_fixture.py OUT.npz        (MARL_DMFB_VARIANT_CRNN_OPS=_tag picks a variant library)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np

import test_gpu_front_bwd_bits as T


def main(path):
    rec = {}
    for rows, stride in T.MLP_CASES:
        rec[T.mlp_key(rows, stride)] = T.run_mlp(rows, stride)
    for od, n_part in T.RED_CASES:
        rec[T.red_key(od, n_part)] = T.run_reduce(od, n_part)
    for k, v in rec.items():
        assert np.isfinite(v).all(), k
    np.savez_compressed(path, **rec)
    print('recorded', path, os.path.getsize(path), 'bytes;', ', '.join('%s %d' % (k, v.size) for k, v in rec.items()))


if __name__ == '__main__':
    main(sys.argv[1])
