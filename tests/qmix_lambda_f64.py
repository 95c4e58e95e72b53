"""The QMIX learn on lambda-returns (args.qmix_lambda) restated on top of tests/qmix_learn_f64.py, in float64 (ground truth) or
float32: `qmix_learn_f64.qmix_learn_once` with the one-step target replaced by the backward walk of the rule
(marl_dmfb_amd.policy.td_lambda: `lambda_targets_reference`, the numpy statement, in the run's precision) on the target mixer's
q_tot.  Helper module: no tests in it.  tests/test_qmix_lambda_host.py and tests/test_gpu_qmix_lambda_learn.py bound the shipped
learn paths by the float32 noise of this restatement (`envelope`, five episode orders), as tests/test_gpu_qmix_learn_f64.py does
for the one-step learn."""
import numpy as np
import torch

import learn_f64
import qmix_learn_f64 as Q
from marl_dmfb_amd.policy.td_lambda import lambda_targets_reference

LAMBDA = 0.8
MAX_TENSOR_FACTOR = Q.MAX_TENSOR_FACTOR

# spec -> (path, learn) -> {tensor: factor} where the bound err <= factor x E_ref needs more than learn_f64.FACTOR: the next power of
# two above the measured err / E_ref (in brackets), never above MAX_TENSOR_FACTOR.  'cpu' is the tensor-op learn on CPU tensors, the
# others the paths of qmix_helpers.F64_PATHS on the GPU.  profiles/qmix_lambda/NOTES.md has the same rows.
FACTORS = {
    'qmix_learn_4d_od24': {
        ('cpu', 0): {'grad/conv2.bias': 4},                               # [2.19]
        ('cpu', 1): {'grad/conv2.weight': 4, 'grad/conv2.bias': 4},       # [2.42, 2.09]
        ('fused_ring', 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 8, 'grad/rnn.bias_ih': 4, 'grad/rnn.bias_hh': 4,
            'grad/mix.hyper_w2.2.bias': 4},                               # [2.95, 4.22, 2.34, 2.30, 2.86]
        ('fused_ring', 1): {'loss': 4, 'grad/rnn.weight_ih': 4, 'grad/mix.hyper_b2.2.bias': 16},          # [2.73, 2.04, 11.79]
        ('fused_two_tensors', 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 8, 'grad/rnn.bias_ih': 4, 'grad/rnn.bias_hh': 4,
            'grad/mix.hyper_w2.2.bias': 4},                               # [2.95, 4.22, 2.34, 2.30, 2.86]
        ('fused_two_tensors', 1): {'loss': 4, 'grad/rnn.weight_ih': 4, 'grad/mix.hyper_b2.2.bias': 16},   # [2.73, 2.04, 11.79]
        ('torch_ops', 0): {'w/conv2.weight': 4, 'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 8, 'w/rnn.weight_hh': 4,
            'grad/rnn.bias_ih': 4},                                       # [2.44, 3.39, 4.94, 2.03, 2.10]
        ('torch_ops', 1): {'loss': 4, 'grad/rnn.weight_ih': 4, 'w/rnn.weight_hh': 4,
            'grad/mix.hyper_b2.2.bias': 16},                              # [2.73, 2.37, 2.04, 11.79]
        ('packed', 0): {'w/conv2.weight': 4, 'grad/rnn.weight_ih': 4, 'w/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 8, 'w/rnn.weight_hh': 4,
            'grad/rnn.bias_ih': 4, 'grad/rnn.bias_hh': 4, 'grad/fc1.weight': 4},             # [2.44, 2.78, 2.06, 4.71, 2.38, 2.34, 2.30, 2.10]
        ('packed', 1): {'grad/rnn.weight_ih': 4, 'w/rnn.weight_ih': 4, 'w/rnn.weight_hh': 4,
            'grad/mix.hyper_b2.2.bias': 16},                              # [2.31, 2.02, 2.39, 11.79]
        ('packed_valu', 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 8, 'grad/rnn.bias_ih': 4,
            'grad/rnn.bias_hh': 4},                                       # [2.96, 4.22, 2.34, 2.30]
        ('packed_valu', 1): {'grad/rnn.weight_ih': 4, 'grad/mix.hyper_b2.2.bias': 16},       # [2.16, 11.79]
    },
    'fov5_4d_od24': {
        ('fused_ring', 0): {'grad_norm': 4, 'grad/conv1.weight': 4, 'w/conv1.weight': 16, 'grad/mlp1.weight': 4, 'grad/mlp1.bias': 4,
            'grad/rnn.weight_ih': 8, 'grad/rnn.weight_hh': 4},            # [2.41, 2.15, 8.82, 2.30, 2.68, 4.46, 2.19]
        ('fused_ring', 1): {'w/conv1.weight': 16, 'grad/rnn.weight_ih': 8, 'grad/rnn.weight_hh': 4},     # [8.82, 6.82, 2.56]
        ('packed', 0): {'w/conv1.weight': 4, 'grad/mlp1.weight': 4, 'grad/rnn.weight_ih': 8, 'grad/mix.hyper_w1.2.bias': 4,
            'grad/mix.hyper_w2.2.bias': 4},                               # [2.56, 2.41, 4.75, 2.05, 2.04]
        ('packed', 1): {'w/conv1.weight': 4, 'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4},          # [2.56, 3.59, 2.04]
    },
}


def path_factors(spec, path, step):
    return FACTORS.get(spec, {}).get((path, step), {})


def lambda_learn_once(batch, P_eval, P_target, PM_eval, PM_target, fov, gamma, lam):
    """loss of one QMIX learn on lambda-returns on the (already trimmed) batch; the graph reaches P_eval and PM_eval only."""
    chosen, best_next = learn_f64.agent_q_values(batch, P_eval, P_target, fov)
    q_tot = Q.mixer(PM_eval, chosen, batch['s'])
    with torch.no_grad():
        q_tot_target = Q.mixer(PM_target, best_next, batch['s_next'])
    np_dtype = np.float64 if q_tot.dtype == torch.float64 else np.float32
    targets = lambda_targets_reference(q_tot_target.numpy(), batch['r'].numpy(), batch['terminated'].numpy(), batch['padded'].numpy(),
                                       gamma, lam, np_dtype)
    mask = 1 - batch['padded']
    return ((mask * (q_tot - torch.as_tensor(targets))) ** 2).sum() / mask.sum()


def reference_lambda_learn(spec, dtype, episode_order=None, lam=LAMBDA):
    """`qmix_learn_f64.qmix_reference_learn` with the lambda-return targets."""
    def run():
        from marl_dmfb_amd.common.arguments import make_args
        g = Q.load_spec(spec)
        kind, W, L, n, fov, hh, clip, A, S = Q.spec_config(spec)
        args = make_args(name=kind, drop_num=n, width=W, length=L, fov=fov, alg='qmix', cuda=False)      # hyper-parameters only
        P_eval, P_target = learn_f64.make_weights(fov, hh, A, 0.0, dtype), learn_f64.make_weights(fov, hh, A, 0.5, dtype)
        PM_eval = Q.make_mixer_weights(S, hh, n, dtype)
        PM_target = {k: v.clone() for k, v in PM_eval.items()}
        named = dict(P_eval)
        named.update({Q.MIX + k: v for k, v in PM_eval.items()})
        return learn_f64.two_learns(named, list(PM_eval.values()) + list(P_eval.values()), args, lambda: lambda_learn_once(
            learn_f64.load_batch(g, dtype, episode_order, Q.STATE_KEYS), P_eval, P_target, PM_eval, PM_target, fov, args.gamma, lam))
    return learn_f64.with_threads(run)


def envelope(spec, lam=LAMBDA):
    """`learn_f64.envelope` of the lambda learn: the float64 run and the float32 noise of five episode orders."""
    return learn_f64.envelope_of('qmix/%s@qmix_lambda=%g' % (spec, lam), lambda dtype, order: reference_lambda_learn(spec, dtype, order, lam),
                                 Q.load_spec(spec)['o'].shape[0])
