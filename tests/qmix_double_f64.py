"""The QMIX learn with double-Q targets (args.qmix_double_q) restated from the existing pieces, in float64 (ground truth) or float32:
the eval network unrolled over T + 1 inputs as in `double_q_f64.double_learn_once` (`learn_f64.q_network`), the selector
q_eval[t + 1] detached, the picks by marl_dmfb_amd.policy.double_q.double_pick_reference in the run's precision -- or GIVEN, as the
(B, T, n) array a shipped learn path reported --, the target network valued at the picks, `qmix_learn_f64.mixer` in the place of the
VDN sums, QMIX's sign (q_tot - targets), and under lambda the walk of marl_dmfb_amd.policy.td_lambda.lambda_targets_reference on the
target mixer's q_tot.  Helper module: no tests in it.

Batches: the specs of tests/qmix_learn_f64.py, edited as `double_q_f64.edited` does: `terminated` cleared on the last valid step of
every second episode, on a copy in memory.  The goldens terminate every episode (all six of qmix_learn_4d_od24 do; `edited` asserts it
for the episodes it touches and `load_edited` for all), so without the edit every tail pick is multiplied by zero and the selector's
step behind an episode goes untested.  The lengths and the trim come from `padded` (`double_q_f64.load_batch`): the reference's trim
reads `terminated`, which the edit changes.

tests/test_qmix_double_host.py and tests/test_gpu_qmix_double_learn.py bound the shipped learn paths by the float32 noise of this
restatement with the path's picks given (`envelope`), and hold the picks themselves to the float64 picks by
`double_q_f64.pick_report`."""
import hashlib

import numpy as np
import torch

import double_q_f64
import learn_f64
import qmix_learn_f64 as Q
from marl_dmfb_amd.policy.double_q import double_pick_reference
from marl_dmfb_amd.policy.td_lambda import lambda_targets_reference
from qmix_helpers import F64_PATHS, replay_batch

LAMBDA = 0.8
MAX_TENSOR_FACTOR = Q.MAX_TENSOR_FACTOR

# spec (+ '@edited') -> (path, lam, learn) -> {tensor: factor} where the bound err <= factor x E_ref needs more than learn_f64.FACTOR:
# the next power of two above the measured err / E_ref (in brackets), never above MAX_TENSOR_FACTOR.  'cpu' is the tensor-op learn on
# CPU tensors, the others the paths of qmix_helpers.F64_PATHS on the GPU.  profiles/qmix_double_q/NOTES.md has the same rows.
FACTORS = {
    'qmix_learn_4d_od24@edited': {
        # the CPU rows were measured on two hosts' CPUs (such ratios depend on the host: profiles/td_block/NOTES.md); the larger counts
        ('cpu', 0.0, 0): {'grad/conv2.bias': 4},                          # [1.19 | 2.64]
        ('cpu', 0.0, 1): {'grad/conv1.bias': 4, 'grad/conv2.bias': 8},    # [2.43, 4.69 | below 2, 3.65]
        ('cpu', 0.8, 0): {'grad/conv1.bias': 4, 'grad/conv2.weight': 4, 'grad/conv2.bias': 8,
            'grad/mlp1.weight': 4},                                       # [2.62, 2.22, 3.03, below 2 | below 2, 2.47, 4.76, 2.14]
        ('fused_ring', 0.0, 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_ih': 8,
            'w/rnn.bias_hh': 8, 'w/mix.hyper_w1.2.weight': 4},    # [3.03, 2.97, 2.44, 4.79, 4.24, 2.20]
        ('fused_ring', 0.0, 1): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_ih': 4,
            'w/rnn.bias_hh': 4, 'w/mix.hyper_w1.2.weight': 4},    # [2.52, 2.17, 2.41, 3.22, 3.56, 2.30]
        ('fused_ring', 0.8, 0): {'w/conv2.weight': 4, 'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'grad/fc1.weight': 4,
            'w/mix.hyper_w1.2.weight': 4, 'grad/mix.hyper_w2.2.bias': 4},    # [3.86, 2.51, 2.52, 2.27, 3.08, 2.03]
        ('fused_ring', 0.8, 1): {'w/mix.hyper_w1.2.weight': 4},    # [2.84]
        ('fused_two_tensors', 0.0, 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4,
            'w/rnn.bias_ih': 8, 'w/rnn.bias_hh': 8, 'w/mix.hyper_w1.2.weight': 4},    # [3.03, 2.97, 2.44, 4.79, 4.24, 2.20]
        ('fused_two_tensors', 0.0, 1): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4,
            'w/rnn.bias_ih': 4, 'w/rnn.bias_hh': 4, 'w/mix.hyper_w1.2.weight': 4},    # [2.52, 2.17, 2.41, 3.22, 3.56, 2.30]
        ('fused_two_tensors', 0.8, 0): {'w/conv2.weight': 4, 'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4,
            'grad/fc1.weight': 4, 'w/mix.hyper_w1.2.weight': 4, 'grad/mix.hyper_w2.2.bias': 4},    # [3.86, 2.51, 2.52, 2.27, 3.08, 2.03]
        ('fused_two_tensors', 0.8, 1): {'w/mix.hyper_w1.2.weight': 4},    # [2.84]
        ('torch_ops', 0.0, 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_ih': 8,
            'w/rnn.bias_hh': 8, 'grad/fc1.weight': 4},    # [3.46, 3.07, 2.17, 5.53, 5.72, 2.17]
        ('torch_ops', 0.0, 1): {'w/mlp1.bias': 4, 'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4,
            'w/rnn.bias_ih': 4, 'w/rnn.bias_hh': 8},    # [2.14, 2.18, 2.33, 2.15, 3.85, 4.27]
        ('torch_ops', 0.8, 0): {'grad_norm': 4, 'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'grad/fc1.weight': 4,
            'w/mix.hyper_w1.2.weight': 4},    # [2.17, 3.00, 2.98, 3.04, 2.56]
        ('torch_ops', 0.8, 1): {'w/mix.hyper_w1.2.weight': 4},    # [2.38]
        ('packed', 0.0, 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_ih': 4,
            'w/rnn.bias_hh': 4, 'w/mix.hyper_w1.2.weight': 4},    # [3.03, 2.86, 2.87, 2.21, 2.76, 2.79]
        ('packed', 0.0, 1): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_ih': 4,
            'w/rnn.bias_hh': 4, 'w/mix.hyper_w1.2.weight': 4},    # [2.68, 2.32, 2.84, 2.28, 2.23, 3.17]
        ('packed', 0.8, 0): {'w/conv2.weight': 4, 'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'grad/fc1.weight': 4},    # [3.86, 2.60, 2.73, 2.22]
        ('packed_valu', 0.0, 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_ih': 8,
            'w/rnn.bias_hh': 8, 'w/mix.hyper_w1.2.weight': 4},    # [3.03, 2.97, 2.59, 4.79, 4.24, 2.20]
        ('packed_valu', 0.0, 1): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_ih': 4,
            'w/rnn.bias_hh': 4, 'w/mix.hyper_w1.2.weight': 4},    # [2.68, 2.13, 2.57, 3.22, 3.56, 2.30]
        ('packed_valu', 0.8, 0): {'w/conv2.weight': 4, 'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'grad/fc1.weight': 4,
            'w/mix.hyper_w1.2.weight': 4},    # [2.24, 2.52, 2.60, 2.22, 2.04]
    },
    'fov5_4d_od24@edited': {
        ('fused_ring', 0.8, 0): {'grad_norm': 4, 'grad/conv1.weight': 4, 'grad/conv1.bias': 4, 'grad/mlp1.bias': 4,
            'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4},    # [2.43, 2.37, 3.16, 2.36, 3.43, 2.46, 3.61]
        ('fused_ring', 0.8, 1): {'grad_norm': 16, 'grad/rnn.weight_ih': 4, 'w/rnn.weight_hh': 4, 'w/mix.hyper_w2.2.bias': 4},    # [8.34, 2.52, 3.61, 2.13]
        ('packed', 0.8, 0): {'grad/conv1.weight': 4, 'grad/conv1.bias': 4, 'grad/mlp1.bias': 4, 'grad/rnn.weight_ih': 4,
            'grad/rnn.weight_hh': 4},    # [2.58, 3.48, 2.78, 2.86, 2.08]
        ('packed', 0.8, 1): {'grad_norm': 16, 'grad/rnn.weight_ih': 4},    # [8.34, 2.47]
    },
    'meda_4d_od32': {
        ('fused_ring', 0.0, 0): {'loss': 4, 'grad/conv2.bias': 4, 'w/mix.hyper_b1.weight': 4},    # [2.23, 2.87, 2.12]
        ('fused_ring', 0.0, 1): {'w/conv2.bias': 4, 'w/fc1.bias': 4, 'w/mix.hyper_b1.weight': 4},    # [2.65, 2.26, 2.12]
    },
}


def path_factors(spec, edit, path, lam, step):
    return FACTORS.get(spec + ('@edited' if edit else ''), {}).get((path, lam, step), {})


_EDITED = {}


def load_edited(spec, edit=True):
    """`qmix_learn_f64.load_spec` with the batch arrays edited by `double_q_f64.edited` (a copy: the cached spec stays as stored)."""
    if (spec, edit) not in _EDITED:
        g = Q.load_spec(spec)
        lens = (g['padded'][:, :, 0] == 0).sum(1)
        assert all(g['terminated'][e, lens[e] - 1, 0] == 1 for e in range(len(lens))), 'every episode of the golden terminates'
        out = double_q_f64.edited(g, edit)
        out['s'], out['s_next'] = np.array(g['s']), np.array(g['s_next'])
        _EDITED[(spec, edit)] = out
    return _EDITED[(spec, edit)]


def load_batch(g, dtype, episode_order=None):
    """`double_q_f64.load_batch` (the trim taken from `padded`) with the global states behind the batch tensors."""
    batch = double_q_f64.load_batch(g, dtype, episode_order)
    T = batch['o'].shape[1]
    order = None if episode_order is None else torch.as_tensor(np.asarray(episode_order, dtype=np.int64))
    for k in ('s', 's_next'):
        v = torch.as_tensor(g[k])
        batch[k] = (v if order is None else v[order]).to(torch.float32).to(dtype)[:, :T]
    return batch


def learn_step(g, agents, path, device, step):
    """One learn of the (edited) batch `g` through a path of qmix_helpers.F64_PATHS ('cpu': the tensor-op learn on CPU tensors), as
    `qmix_helpers.f64_case_learn` runs it but trimmed by `padded` like the restatement.  The path's precondition is asserted first.
    Returns the permutation the path applied to the episodes (None: none)."""
    pol = agents.policy
    batch = replay_batch(g, device, F64_PATHS[path][0] if path != 'cpu' else True)
    lens = (~batch['padded'][:, :, 0]).sum(1).cpu().numpy()
    if path.startswith('packed'):
        assert pol.packed_ok(batch) is True, 'the packed learn must apply to this batch'
        assert int(lens.sum()) < batch['o'].shape[0] * batch['o'].shape[1], 'the batch must have padded steps to leave out'
        order = np.argsort(-lens, kind='stable')
        pol.learn_packed(batch, order, lens[order], step)
        return order
    assert pol._mix_fused_ok(batch) is (path not in ('torch_ops', 'cpu')), 'the path under test must be the one the learn takes'
    agents.train(batch, step, max_len=int(lens.max()))
    return None


def double_learn_once(batch, P_eval, P_target, PM_eval, PM_target, fov, gamma, lam, picks, record):
    """loss of one QMIX learn with double-Q targets on the (already trimmed) batch; the graph reaches P_eval and PM_eval only.
    picks: None (the run's own, from its detached selector in its precision) or (B, T, n); record receives (picks, selector)."""
    B, T, n = batch['o'].shape[:3]
    rows = B * n
    dtype = batch['o'].dtype
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    h_e = torch.zeros((rows, learn_f64.HIDDEN), dtype=dtype)
    h_t = torch.zeros((rows, learn_f64.HIDDEN), dtype=dtype)
    q_evals, q_targets = [], []
    for t in range(T + 1):                      # the eval network over inputs 0 .. T, the target network over 1 .. T from zero
        inputs = learn_f64._step_inputs(batch, t, rows)
        q_e, h_e = learn_f64.q_network(P_eval, fov, inputs, h_e)
        q_evals.append(q_e.view(B, n, -1))
        if t >= 1:
            with torch.no_grad():
                q_t, h_t = learn_f64.q_network(P_target, fov, inputs, h_t)
            q_targets.append(q_t.view(B, n, -1))
    q_evals, q_targets = torch.stack(q_evals, dim=1), torch.stack(q_targets, dim=1)      # (B, T + 1, n, A), (B, T, n, A)
    chosen = torch.gather(q_evals[:, :T], 3, batch['u']).squeeze(3)
    q_sel = q_evals[:, 1:].detach()
    if picks is None:
        picks = double_pick_reference(q_sel.numpy(), q_targets.numpy(), batch['avail_u_next'].numpy(), np_dtype)[0]
    record.append((np.asarray(picks, np.int8), q_sel.numpy().astype(np.float64)))
    valued = q_targets.masked_fill(batch['avail_u_next'] == 0, -9999999)
    valued = torch.gather(valued, 3, torch.as_tensor(np.asarray(picks, np.int64)).unsqueeze(3)).squeeze(3)
    q_tot = Q.mixer(PM_eval, chosen, batch['s'])
    with torch.no_grad():
        q_tot_target = Q.mixer(PM_target, valued, batch['s_next'])
    if lam:
        targets = torch.as_tensor(lambda_targets_reference(q_tot_target.numpy(), batch['r'].numpy(), batch['terminated'].numpy(),
                                                           batch['padded'].numpy(), gamma, lam, np_dtype))
    else:
        targets = batch['r'] + gamma * q_tot_target * (1 - batch['terminated'])
    mask = 1 - batch['padded']
    return ((mask * (q_tot - targets.detach())) ** 2).sum() / mask.sum()      # QMIX's sign


def reference_double_learn(spec, edit, dtype, episode_order=None, lam=0.0, picks=None, weights=None):
    """`qmix_learn_f64.qmix_reference_learn` with double-Q targets on the (edited) spec.  picks: None or the two learns' (B, T, n)
    arrays in the golden's episode order (they follow `episode_order`).  Every learn's dict also holds 'picks' (B, T, n) and 'q_sel'
    (B, T, n, A) float64 values of the run's selector, both back in the golden's episode order.  weights: None (the deterministic
    ones) or ({name: tensor} of the eval network, the same of the target network), converted to `dtype`."""
    def run():
        from marl_dmfb_amd.common.arguments import make_args
        g = load_edited(spec, edit)
        kind, W, L, n, fov, hh, clip, A, S = Q.spec_config(spec)
        args = make_args(name=kind, drop_num=n, width=W, length=L, fov=fov, alg='qmix', cuda=False)      # hyper-parameters only
        if weights is None:
            P_eval, P_target = learn_f64.make_weights(fov, hh, A, 0.0, dtype), learn_f64.make_weights(fov, hh, A, 0.5, dtype)
        else:
            P_eval, P_target = ({k: v.detach().cpu().to(dtype).clone() for k, v in w.items()} for w in weights)
        PM_eval = Q.make_mixer_weights(S, hh, n, dtype)
        PM_target = {k: v.clone() for k, v in PM_eval.items()}
        named = dict(P_eval)
        named.update({Q.MIX + k: v for k, v in PM_eval.items()})
        order = np.arange(g['o'].shape[0]) if episode_order is None else np.asarray(episode_order)
        record = []

        def loss():
            given = None if picks is None else np.asarray(picks[len(record)])[order]
            return double_learn_once(load_batch(g, dtype, episode_order), P_eval, P_target, PM_eval, PM_target, fov, args.gamma, lam,
                                     given, record)
        out = learn_f64.two_learns(named, list(PM_eval.values()) + list(P_eval.values()), args, loss)
        back = np.argsort(order)
        for step, (p, s) in enumerate(record):
            out[step]['picks'], out[step]['q_sel'] = p[back], s[back]
        return out
    return learn_f64.with_threads(run)


def envelope(spec, edit, lam, picks=None):
    """`learn_f64.envelope` of the double-Q learn on a spec, edited or as stored: the float64 run and the float32 noise of five
    episode orders, every run on its own picks (picks None) or on the given ones.  Cached per spec, edit, lambda and picks."""
    tag = 'own' if picks is None else hashlib.sha1(b''.join(np.ascontiguousarray(p, np.int8).tobytes() for p in picks)).hexdigest()
    return learn_f64.envelope_of('qmix/%s@qmix_double_q edit=%d lam=%g picks=%s' % (spec, edit, lam, tag),
                                 lambda dtype, order: reference_double_learn(spec, edit, dtype, order, lam, picks),
                                 Q.load_spec(spec)['o'].shape[0])
