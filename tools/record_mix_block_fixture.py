"""Records tests/golden/mix_block_bits.npz: what the mixing + TD block of the libqmix_ops.so in use computes for the seeded cases of
tests/test_gpu_mix_block_bits.py (the inputs are regenerated from the seeds there; only the outputs are stored, large arrays as one
digest per row), and, with a second path, tests/golden/qmix_cabi_returns.json: the return codes of the argument lists of
tests/test_qmix_cabi_returns.py (needs no GPU).  The committed files were recorded on an MI355X with the build of the commit BEFORE
the entry points of marl_dmfb_amd/csrc/qmix_ops.hip were folded into one launch path and its selector and the shared pieces of its
lambda walk moved into csrc/td_rules.h; run it again only from a build whose bits are meant to become the new record.

    python tools/record_mix_block_fixture.py OUT.npz [OUT.json]     (MARL_DMFB_VARIANT_QMIX_OPS=_tag picks a variant library)
    python tools/record_mix_block_fixture.py - OUT.json              (the return codes only)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np


def bits(path):
    import test_gpu_mix_block_bits as T
    rec = {}
    for key, run in T.all_runs().items():
        out = run()
        again = run()                     # no float atomics in the block: a second launch gives the same words
        assert int(out['bad'][0]) == T.expected_bad(key), (key, int(out['bad'][0]))
        for f in T.fields(key):
            a, b = T.words(out[f]), T.words(again[f])
            assert np.array_equal(a, b), (key, f)
            rec[key + '.' + f] = a
    np.savez_compressed(path, **rec)
    print('recorded', path, os.path.getsize(path), 'bytes;', len(rec), 'arrays of', len(T.all_runs()), 'cases')


def returns(path):
    import test_qmix_cabi_returns as R
    rec = R.record()
    with open(path, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print('recorded', path, sum(len(v) for v in rec.values()), 'rows of', len(rec), 'entry points')


if __name__ == '__main__':
    if sys.argv[1] != '-':
        bits(sys.argv[1])
    if len(sys.argv) > 2:
        returns(sys.argv[2])
