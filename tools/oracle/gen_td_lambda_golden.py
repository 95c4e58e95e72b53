"""Record the reference's `td_lambda_target` (common/utils.py:33-79; never called by the reference's own learners) on one small
seeded batch, for tests/test_td_lambda_host.py (container-only).

The batch: B = 8 episodes of T = 9 slots, lengths 1, 2, 9 and five between, every last valid step terminated, the padded steps as
the reference's rollout pads them (r = 0, padded = 1, terminated = 1; common/rollout.py:130-141), one agent, gamma 0.99, lambda 0.8
and 0.5.  Inputs and the function's outputs go to tests/golden/td_lambda_ref.npz: q_targets, r, terminated, padded (B, T, 1)
float32, lens, gamma, lambdas, and target_<k> (B, T, 1) float32 for lambdas[k].

Run:  python tools/oracle/gen_td_lambda_golden.py
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, '..', '..')
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'td_lambda_ref.npz')
B, T, GAMMA, LAMBDAS = 8, 9, 0.99, (0.8, 0.5)
LENS = (9, 1, 2, 5, 7, 3, 9, 4)


def main():
    ref_shim.install()
    import torch
    from common.utils import td_lambda_target
    rng = np.random.default_rng(20)
    lens = np.asarray(LENS, np.int64)
    steps = np.arange(T)[None, :]
    padded = (steps >= lens[:, None]).astype(np.float32)[:, :, None]
    terminated = (steps >= lens[:, None] - 1).astype(np.float32)[:, :, None]        # the last valid step and every padded one
    r = (rng.standard_normal((B, T, 1)) * (1 - padded)).astype(np.float32)          # padded rewards are 0
    q_targets = (rng.standard_normal((B, T, 1)) * 2).astype(np.float32)             # padded slots keep values: they must not leak
    batch = {'o': torch.zeros((B, T, 1, 1)), 'r': torch.as_tensor(r), 'padded': torch.as_tensor(padded),
             'terminated': torch.as_tensor(terminated)}
    out = {'q_targets': q_targets, 'r': r, 'terminated': terminated, 'padded': padded, 'lens': lens,
           'gamma': np.float64(GAMMA), 'lambdas': np.asarray(LAMBDAS, np.float64)}
    for k, lam in enumerate(LAMBDAS):
        args = SimpleNamespace(n_agents=1, gamma=GAMMA, td_lambda=lam)
        out['target_%d' % k] = td_lambda_target(batch, T, torch.as_tensor(q_targets), args).numpy().astype(np.float32)
    np.savez_compressed(OUT, **out)
    print('%s: %d episodes x %d steps, %.1f kB' % (os.path.basename(OUT), B, T, os.path.getsize(OUT) / 1e3))


if __name__ == '__main__':
    main()
