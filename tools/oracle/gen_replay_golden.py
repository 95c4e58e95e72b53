"""Record the reference ReplayBuffer's side of tests/test_replay_buffer.py::test_against_live_reference_class
(container-only).

The reference class (common/replay_buffer.py) is fed the test's episode batches (`_batch`, sizes `INCS`, zeroed
buffers first) and after every store_episode its (current_idx, current_size) and every buffer are written to
tests/golden/replay_buffer_ref.npz as step<k>_state and step<k>_<key>, in the reference's own dtypes.

Run:  python tools/oracle/gen_replay_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, '..', '..')
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'replay_buffer_ref.npz')


def main():
    ref_shim.install()
    from common.replay_buffer import ReplayBuffer as RefBuffer
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_replay_buffer import INCS, _args, _batch   # the test's inputs, not a copy of them
    a = _args()
    ref = RefBuffer(a)
    for k in ref.buffers:
        ref.buffers[k][...] = 0
    out = {'incs': np.asarray(INCS, np.int64)}
    eid = 0
    for step, inc in enumerate(INCS):
        batch = _batch(eid, inc, a)
        eid += inc
        ref.store_episode(batch)
        out['step%d_state' % step] = np.array([ref.current_idx, ref.current_size], np.int64)
        for k, v in ref.buffers.items():
            out['step%d_%s' % (step, k)] = np.array(v)
    np.savez_compressed(OUT, **out)
    print('%s: %d insertions, %.0f kB' % (os.path.basename(OUT), len(INCS), os.path.getsize(OUT) / 1e3))


if __name__ == '__main__':
    main()
