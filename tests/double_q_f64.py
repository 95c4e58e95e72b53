"""The VDN learn with double-Q targets (args.double_q) restated on top of tests/learn_f64.py, in float64 (ground truth) or float32:
the eval network unrolled over T + 1 inputs (`learn_f64.q_network`), the selector q_eval[t + 1] detached, the picks by
marl_dmfb_amd.policy.double_q.double_pick_reference in the run's precision -- or GIVEN, as the (B, T, n) array a shipped learn path
reported, so that a pick that falls the other way at a near-tie does not count as arithmetic error --, the target network valued at
the picks, then the one-step loss or the lambda loss (marl_dmfb_amd.policy.td_lambda.lambda_targets_reference) and
`learn_f64.two_learns`.  Helper module: no tests in it.

Own loader: the lengths come from `padded`, and `edited` clears `terminated` on the last valid step of every second episode, on a
copy in memory.  The goldens terminate every episode, so without that edit every tail pick is multiplied by zero and the selector's
last step is not tested at all.

tests/test_double_q_host.py and tests/test_gpu_double_q_learn.py bound the shipped learn paths by the float32 noise of this
restatement with the path's picks given (`envelope`), and hold the picks themselves to the float64 picks by `pick_report`."""
import hashlib

import numpy as np
import torch

import learn_f64
from marl_dmfb_amd.policy.double_q import double_pick_reference
from marl_dmfb_amd.policy.td_lambda import lambda_targets_reference

LAMBDA = 0.8
GAP_FACTOR = 64          # picks may differ from the float64 picks where the float64 selector's top-two gap is <= GAP_FACTOR x E_sel:
                         # 2 (two values, each off by E_sel) x 4 (the factor the learn tests grant a path's first learn over E_ref; the
                         # larger factors of FACTORS below are second-learn rows of gradients and weights, not Q values) x 8 (headroom)
MAX_DIFFER = 0.01        # and in at most this share of the valid (step, agent) picks

# golden name (+ '@edited') -> (path, lam, learn) -> {tensor: factor} where err <= factor x E_ref needs more than learn_f64.FACTOR:
# the next power of two above the measured err / E_ref (in brackets), in the form of td_lambda_f64.FACTORS.
# profiles/double_q/NOTES.md has the same rows.
FACTORS = {
    'vdn_learn_4d_od24_short.npz': {
        ('cpu', 0.0, 0): {'grad/conv1.bias': 4},                       # [2.05]
        ('cpu', 0.8, 0): {'grad_norm': 4, 'grad/conv1.bias': 4},       # [2.05, 2.31]: the rows of td_lambda_f64.FACTORS (the picks agree)
    },
    'vdn_learn_4d_od24_short.npz@edited': {
        ('cpu', 0.0, 0): {'grad/conv1.bias': 4},                       # [2.03]
        ('fused_td', 0.0, 1): {'grad_norm': 8, 'grad/conv1.weight': 8, 'w/conv1.weight': 4, 'grad/conv2.weight': 4, 'grad/conv2.bias': 4,
            'grad/mlp1.weight': 4, 'grad/mlp1.bias': 4, 'w/mlp1.bias': 4, 'grad/rnn.weight_hh': 4, 'grad/fc1.weight': 4,
            'grad/fc1.bias': 16},                                      # [4.30, 4.00, 2.56, 2.75, 2.49, 2.28, 3.31, 2.40, 2.17, 3.85, 9.33]
        ('fused_td', 0.8, 0): {'w/conv1.weight': 4},                   # [2.44]
        ('fused_td', 0.8, 1): {'grad_norm': 8, 'grad/rnn.weight_ih': 4, 'grad/rnn.bias_ih': 4},                          # [4.93, 2.63, 2.60]
        ('packed', 0.0, 1): {'grad_norm': 8, 'grad/conv1.weight': 4, 'grad/conv2.weight': 4, 'grad/conv2.bias': 4, 'grad/mlp1.bias': 4,
            'grad/fc1.weight': 4, 'grad/fc1.bias': 16},                # [4.30, 3.70, 2.46, 2.23, 2.81, 3.35, 9.33]
        ('packed', 0.8, 0): {'w/conv1.weight': 4},                     # [3.42]
        ('packed', 0.8, 1): {'grad_norm': 8, 'grad/rnn.weight_ih': 4, 'grad/rnn.bias_ih': 4, 'grad/rnn.bias_hh': 4},     # [4.93, 2.63, 2.34, 2.19]
    },
    'vdn_learn_4d_od24_b64.npz': {
        ('fused_td', 0.0, 1): {'w/fc1.bias': 4},                       # [3.59]
        ('fused_td', 0.8, 0): {'w/rnn.weight_ih': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_ih': 4, 'w/rnn.bias_hh': 4},      # [2.21, 2.10, 2.42, 2.67]
        ('fused_td', 0.8, 1): {'loss': 4, 'w/rnn.weight_ih': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_ih': 4,
            'w/rnn.bias_hh': 4},                                       # [2.93, 2.21, 2.10, 2.05, 2.68]: the rows of td_lambda_f64.FACTORS
        ('packed', 0.0, 1): {'w/fc1.bias': 8},                         # [4.29]
    },
}


def path_factors(name, edit, path, lam, step):
    return FACTORS.get(name + ('@edited' if edit else ''), {}).get((path, lam, step), {})


def edited(g, edit=True):
    """The golden's batch arrays as a dict; edit: `terminated` cleared on the last valid step of every second episode (1, 3, ...)."""
    out = {k: np.array(g[k]) for k in learn_f64.BATCH_KEYS + ['cfg', 'names']}
    if edit:
        lens = (out['padded'][:, :, 0] == 0).sum(1)
        for e in range(1, len(lens), 2):
            assert out['terminated'][e, lens[e] - 1, 0] == 1
            out['terminated'][e, lens[e] - 1, 0] = 0
    return out


def load_batch(g, dtype, episode_order=None):
    """`learn_f64.load_batch` with the trim taken from `padded`: T = the longest run of leading valid steps."""
    order = None if episode_order is None else torch.as_tensor(np.asarray(episode_order, dtype=np.int64))
    batch = {}
    for k in learn_f64.BATCH_KEYS:
        v = torch.as_tensor(g[k])
        if order is not None:
            v = v[order]
        batch[k] = v.long() if k == 'u' else v.to(torch.float32).to(dtype)
    T = int((batch['padded'][:, :, 0] == 0).sum(1).max())
    return {k: v[:, :T] for k, v in batch.items()}


def learn_step(g, agents, device, step, packed=False):
    """One learn of the (edited) golden batch `g` through a shipped path, as vdn_helpers.learn_golden_step runs it, but trimmed by
    `padded` like the restatement (the reference's trim reads `terminated`, which the edit changes): 'cpu' the tensor-op learn, on the
    GPU the fused padded learn or (packed) learn_packed.  Returns the permutation the path applied to the episodes (None: none)."""
    batch = {k: torch.as_tensor(g[k]).to(device) for k in learn_f64.BATCH_KEYS}
    batch['padded'], batch['terminated'] = batch['padded'].bool(), batch['terminated'].bool()
    lens = (~batch['padded'][:, :, 0]).sum(1).cpu().numpy()
    if device != 'cpu':
        batch['r'] = batch['r'].float()
        for k in ('u', 'avail_u', 'avail_u_next', 'u_onehot', 'o', 'o_next'):
            batch[k] = batch[k].to(torch.int8)
        assert agents.policy._td_fused_ok(batch), 'the shipped (fused TD) learn path must be the one under test'
    else:
        assert not agents.policy._td_fused_ok(batch)
    if packed:
        assert agents.policy.packed_ok(batch), 'the packed learn path must apply to this golden'
        order = np.argsort(-lens, kind='stable')
        agents.policy.learn_packed(batch, order, lens[order], step)
        return order
    agents.train(batch, step, max_len=int(lens.max()))
    return None


def double_learn_once(batch, P_eval, P_target, fov, gamma, lam, picks, record):
    """loss of one VDN learn with double-Q targets on the (already trimmed) batch; the graph reaches the tensors of P_eval only.
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
    avail = batch['avail_u_next'].numpy()
    if picks is None:
        picks = double_pick_reference(q_sel.numpy(), q_targets.numpy(), avail, np_dtype)[0]
    record.append((np.asarray(picks, np.int8), q_sel.numpy().astype(np.float64)))
    valued = q_targets.masked_fill(batch['avail_u_next'] == 0, -9999999)
    valued = torch.gather(valued, 3, torch.as_tensor(np.asarray(picks, np.int64)).unsqueeze(3)).squeeze(3)
    q_tot, q_tot_target = chosen.sum(dim=2, keepdim=True), valued.sum(dim=2, keepdim=True)   # the VDN mixer
    mask = 1 - batch['padded']
    if lam:
        targets = torch.as_tensor(lambda_targets_reference(q_tot_target.numpy(), batch['r'].numpy(), batch['terminated'].numpy(),
                                                           batch['padded'].numpy(), gamma, lam, np_dtype))
    else:
        targets = batch['r'] + gamma * q_tot_target * (1 - batch['terminated'])
    return ((mask * (targets.detach() - q_tot)) ** 2).sum() / mask.sum()


def reference_double_learn(g, dtype, episode_order=None, lam=0.0, picks=None, weights=None):
    """`learn_f64.reference_learn` with double-Q targets on the batch dict `g`.  picks: None or the two learns' (B, T, n) arrays in
    the golden's episode order (they follow `episode_order`).  Every learn's dict also holds 'picks' (B, T, n) and 'q_sel'
    (B, T, n, A) float64 values of the run's selector, both back in the golden's episode order.  weights: None (the goldens'
    deterministic ones) or ({name: tensor} of the eval network, the same of the target network), converted to `dtype`."""
    def run():
        from marl_dmfb_amd.common.arguments import make_args
        kind, W, L, n, fov, od, clip, A = learn_f64.golden_config(g)
        args = make_args(name=kind, drop_num=n, width=W, length=L, fov=fov, cuda=False)      # hyper-parameters only
        if weights is None:
            P_eval, P_target = learn_f64.make_weights(fov, od, A, 0.0, dtype), learn_f64.make_weights(fov, od, A, 0.5, dtype)
        else:
            P_eval, P_target = ({k: v.detach().cpu().to(dtype).clone() for k, v in w.items()} for w in weights)
        order = np.arange(g['o'].shape[0]) if episode_order is None else np.asarray(episode_order)
        record = []

        def loss():
            given = None if picks is None else np.asarray(picks[len(record)])[order]
            return double_learn_once(load_batch(g, dtype, episode_order), P_eval, P_target, fov, args.gamma, lam, given, record)
        out = learn_f64.two_learns(P_eval, list(P_eval.values()), args, loss)
        back = np.argsort(order)
        for step, (p, s) in enumerate(record):
            out[step]['picks'], out[step]['q_sel'] = p[back], s[back]
        return out
    return learn_f64.with_threads(run)


def envelope(name, edit, lam, picks=None):
    """`learn_f64.envelope` of the double-Q learn on a golden (file name), edited or as stored: the float64 run and the float32
    noise of five episode orders, every run on its own picks (picks None) or on the given ones.  Cached per golden, edit, lambda and
    picks."""
    g = edited(np.load(learn_f64.golden_path(name)), edit)
    tag = 'own' if picks is None else hashlib.sha1(b''.join(np.ascontiguousarray(p, np.int8).tobytes() for p in picks)).hexdigest()
    return learn_f64.envelope_of('%s@double_q edit=%d lam=%g picks=%s' % (name, edit, lam, tag),
                                 lambda dtype, order: reference_double_learn(g, dtype, order, lam, picks), g['o'].shape[0])


def selector_error(own, step):
    """E_sel of one learn: the largest |q_sel32 - q_sel64| over the envelope's five float32 runs."""
    return max(float(np.abs(run[step]['q_sel'] - own['ref'][step]['q_sel']).max()) for run in own['runs32'])


def selector_gap(q_sel64, avail):
    """(B, T, n): the gap between the two largest available values of every float64 selector row (inf with one available action,
    0 with none: every action stands at -9999999)."""
    s = np.where(np.asarray(avail) == 0, -np.inf, q_sel64)
    s = np.sort(s, axis=-1)
    with np.errstate(invalid='ignore'):
        gap = s[..., -1] - s[..., -2]
    return np.where(np.isnan(gap), 0.0, gap)


def pick_report(label, picks, own, step, g):
    """The pick-agreement condition of one learn: `picks` (B, T, n), in the golden's episode order, against the float64
    restatement's own picks on the valid steps.  They may differ only where the float64 selector's top-two gap among the available
    actions is <= GAP_FACTOR x E_sel, and in at most MAX_DIFFER of the valid picks.  Prints the figures; returns the violations."""
    ref = own['ref'][step]
    T = ref['picks'].shape[1]
    valid = np.broadcast_to((np.asarray(g['padded'])[:, :T, 0] == 0)[:, :, None], ref['picks'].shape)
    e_sel = selector_error(own, step)
    gap = selector_gap(ref['q_sel'], np.asarray(g['avail_u_next'])[:, :T])
    differ = (np.asarray(picks)[:, :T] != ref['picks']) & valid
    worst = float(gap[differ].max()) if differ.any() else 0.0
    print('double_q picks %s step %d: %d of %d valid picks differ from float64 (cap %d), largest gap there %.3e, allowed %.3e (E_sel %.3e)'
          % (label, step, differ.sum(), valid.sum(), int(MAX_DIFFER * valid.sum()), worst, GAP_FACTOR * e_sel, e_sel))
    bad = []
    if worst > GAP_FACTOR * e_sel:
        bad.append('%s step %d: a pick differs from float64 at a selector gap of %.3e > %d x E_sel = %.3e' % (label, step, worst, GAP_FACTOR,
                                                                                                              GAP_FACTOR * e_sel))
    if differ.sum() > MAX_DIFFER * valid.sum():
        bad.append('%s step %d: %d of %d valid picks differ from float64' % (label, step, differ.sum(), valid.sum()))
    return bad
