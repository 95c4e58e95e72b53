"""The VDN learn on lambda-returns (args.td_lambda) restated on top of tests/learn_f64.py, in float64 (ground truth) or float32:
`learn_f64.agent_q_values` (both Q-networks), the VDN sum, the backward walk of the rule (marl_dmfb_amd.policy.td_lambda:
`lambda_targets_reference`, the numpy statement, in the run's precision), the masked squared error, `learn_f64.two_learns`.
Helper module: no tests in it.  tests/test_td_lambda_host.py and tests/test_gpu_td_lambda_learn.py bound the shipped learn paths by
the float32 noise of this restatement (`envelope`, five episode orders), as tests/test_gpu_learn_f64.py does for the one-step learn."""
import os

import numpy as np
import torch

import learn_f64
from marl_dmfb_amd.policy.td_lambda import lambda_targets_reference

LAMBDA = 0.8

# golden -> (path, learn) -> {tensor: factor} where the bound err <= factor x E_ref needs more than learn_f64.FACTOR: the next power
# of two above the measured err / E_ref (in brackets).  'cpu' is the tensor-op learn on CPU tensors, 'fused_td' and 'packed' the
# GPU learns.  profiles/td_lambda/NOTES.md has the same rows.
FACTORS = {
    'vdn_learn_4d_od24_short.npz': {
        ('cpu', 0): {'grad_norm': 4, 'grad/conv1.bias': 4},       # [2.05, 2.31]
        ('cpu', 1): {'grad/fc1.bias': 4},                         # [2.19]
        ('fused_td', 0): {'w/rnn.weight_hh': 4},                                        # [2.88]
        ('fused_td', 1): {'grad_norm': 4, 'w/rnn.weight_hh': 4, 'w/fc1.bias': 4},       # [2.16, 2.89, 2.78]
        ('packed', 0): {'w/rnn.weight_hh': 4},                                          # [2.86]
        ('packed', 1): {'grad_norm': 4, 'w/rnn.weight_hh': 4, 'w/fc1.bias': 4},         # [2.16, 2.86, 2.78]
    },
    'vdn_learn_4d_od24_b64.npz': {
        ('fused_td', 0): {'loss': 4, 'w/rnn.weight_ih': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_ih': 4,
            'w/rnn.bias_hh': 4},                                                        # [2.75, 2.25, 2.11, 2.07, 2.45]
        ('fused_td', 1): {'w/rnn.weight_ih': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_ih': 4, 'w/rnn.bias_hh': 4},   # [2.24, 2.12, 2.42, 2.56]
        ('packed', 1): {'grad/fc1.bias': 4},                                            # [2.43]
    },
}


def path_factors(name, path, step):
    return FACTORS.get(name, {}).get((path, step), {})


def lambda_learn_once(batch, P_eval, P_target, fov, gamma, lam):
    """loss of one VDN learn on lambda-returns on the (already trimmed) batch; the graph reaches the tensors of P_eval only."""
    chosen, best_next = learn_f64.agent_q_values(batch, P_eval, P_target, fov)
    q_tot, q_tot_target = chosen.sum(dim=2, keepdim=True), best_next.sum(dim=2, keepdim=True)   # the VDN mixer
    np_dtype = np.float64 if q_tot.dtype == torch.float64 else np.float32
    targets = lambda_targets_reference(q_tot_target.detach().numpy(), batch['r'].numpy(), batch['terminated'].numpy(),
                                       batch['padded'].numpy(), gamma, lam, np_dtype)
    mask = 1 - batch['padded']
    return ((mask * (torch.as_tensor(targets) - q_tot)) ** 2).sum() / mask.sum()


def reference_lambda_learn(path, dtype, episode_order=None, lam=LAMBDA):
    """`learn_f64.reference_learn` with the lambda-return targets."""
    def run():
        from marl_dmfb_amd.common.arguments import make_args
        g = np.load(path)
        kind, W, L, n, fov, od, clip, A = learn_f64.golden_config(g)
        args = make_args(name=kind, drop_num=n, width=W, length=L, fov=fov, cuda=False)      # hyper-parameters only
        P_eval, P_target = learn_f64.make_weights(fov, od, A, 0.0, dtype), learn_f64.make_weights(fov, od, A, 0.5, dtype)
        return learn_f64.two_learns(P_eval, list(P_eval.values()), args,
                                    lambda: lambda_learn_once(learn_f64.load_batch(g, dtype, episode_order), P_eval, P_target, fov,
                                                              args.gamma, lam))
    return learn_f64.with_threads(run)


def envelope(path, lam=LAMBDA):
    """`learn_f64.envelope` of the lambda learn: the float64 run and the float32 noise of five episode orders."""
    return learn_f64.envelope_of('%s@td_lambda=%g' % (os.path.basename(path), lam),
                                 lambda dtype, order: reference_lambda_learn(path, dtype, order, lam), np.load(path)['o'].shape[0])
