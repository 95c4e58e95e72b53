"""A plain restatement of the reference's VDN learn (policy/vdn.py:79-200 with the CRNN of network/base_net.py:23-71 and the
length trim of agent/agent.py:51-70) in torch.nn.functional calls on the CPU, in float64 (ground truth) or float32 (the
reference's own arithmetic), for the learn goldens under tests/golden.  Helper module: no tests in it.

The goldens carry the whole minibatch, and the weights come from the closed formula `vdn_helpers.det_init`, so the two consecutive
learns a golden was captured from can be recomputed here in full: every element of every clipped gradient and of every weight
after the Adam step, where the golden itself stores 512 sampled elements per tensor.

Nothing of the package's networks or learners is imported: `make_args` gives the hyper-parameters (learning rate, gamma, hidden
size), the rest is written out below.  The rewards are rounded to float32 first in either precision, as the reference does before
it computes anything (policy/vdn.py:92): the float64 run is the exact value of the function every float32 path rounds.

`envelope(path)` measures the reference's own float32 rounding noise on a golden's batch: the restatement in float32 on the
episodes in five different orders (same mathematics, different summation order) against the float64 run.  The GPU tests bound
the shipped learn paths by that noise, never by each other.

tests/qmix_learn_f64.py restates the QMIX learn on top of this module: `agent_q_values` (the Q-network half of a learn),
`load_batch` (with the global states behind the batch keys), `two_learns` (backward, one clip, one Adam, twice), `envelope_of`
and the comparisons serve both."""
import os

import numpy as np
import torch
import torch.nn.functional as f

from vdn_helpers import det_init

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
VDN_GOLDENS = ['vdn_learn_4d_od24.npz', 'vdn_learn_4d_od24_short.npz', 'vdn_learn_10d_od32.npz', 'vdn_learn_meda_4d_od32.npz',
               'vdn_learn_4d_od24_b64.npz']
FOV_GOLDENS = ['fovlearn_4d_od24_fov5.npz', 'fovlearn_3d_od32_fov7.npz', 'fovlearn_4d_od24_fov11.npz', 'fovlearn_3d_od32_fov13.npz']
ALL_GOLDENS = VDN_GOLDENS + FOV_GOLDENS
BATCH_KEYS = ['o', 'u', 'r', 'o_next', 'avail_u', 'avail_u_next', 'u_onehot', 'padded', 'terminated']

# fov -> the conv stack as (module name, stride) in the order applied; fov 19 applies the same module twice (tied weights)
_STACK = {5: [('conv1', 1)], 7: [('conv1', 1), ('conv2', 1)], 9: [('conv1', 1), ('conv2', 1)], 11: [('conv1', 1), ('conv2', 1)],
          13: [('conv1', 1), ('conv2', 1)], 19: [('conv1', 2), ('conv2', 1), ('conv2', 1)]}
HIDDEN = 128
N_ORDERS = 5                  # identity + four seeded permutations of the episodes
THREADS = 8                   # intra-op threads of every run below: the CPU's float32 GEMMs split their sums by thread count, and
                              # the envelope should depend on the machine that computes it as little as can be had
FACTOR = 2.0                  # margin for having sampled the reference's float32 noise only N_ORDERS times

# The bound of the GPU paths (tests/test_gpu_learn_f64.py): golden -> (path, learn) -> {tensor: factor} where the factor is not
# FACTOR, namely the next power of two above the err / E_ref measured for that tensor on that path and learn; every other row is
# held to FACTOR.  profiles/learn_f64/NOTES.md has every row and the evidence (tools/diag_learn_f64.py reruns it): the first
# learn's excess on the gradients comes from the float32 GEMMs of the eval network's linear layers (x W^T, g W and g^T x of
# `_LinearSplitK`), which are inside their derived bound -- with float64 products in their place every first-learn gradient of
# every golden tried is under 2 x E_ref on the padded and on both packed paths; the second learn's and the weights' is the batch's
# conditioning (Adam moves elements with |g| near eps by up to 2 lr either way); loss and norm are float32 scalars whose E_ref
# can lie far below one ulp.
FACTORS = {
    'vdn_learn_4d_od24.npz': {
        ('fused_td', 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4},
        ('fused_td', 1): {'grad_norm': 4, 'w/conv1.weight': 4, 'grad/conv2.weight': 4, 'w/conv2.weight': 4},
        ('host_len_bound', 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4},
        ('host_len_bound', 1): {'grad_norm': 4, 'w/conv1.weight': 4, 'grad/conv2.weight': 4, 'w/conv2.weight': 4},
        ('packed', 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4},
        ('packed', 1): {'grad_norm': 4, 'w/conv1.weight': 4, 'w/conv2.weight': 4, 'w/rnn.bias_ih': 4, 'w/rnn.bias_hh': 4},
        ('packed_valu', 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4},
        ('packed_valu', 1): {'grad_norm': 8, 'w/conv1.weight': 4, 'w/conv2.weight': 4, 'grad/conv2.bias': 4, 'w/rnn.bias_ih': 4,
            'w/rnn.bias_hh': 4},
    },
    'vdn_learn_4d_od24_short.npz': {
        ('fused_td', 0): {'loss': 4},
        ('fused_td', 1): {'grad_norm': 8, 'grad/mlp1.bias': 4, 'grad/fc1.bias': 4},
        ('host_len_bound', 0): {'w/rnn.bias_ih': 4, 'w/rnn.bias_hh': 4},
        ('host_len_bound', 1): {'grad_norm': 8, 'grad/mlp1.bias': 4, 'grad/fc1.bias': 4},
        ('packed', 0): {'loss': 4},
        ('packed', 1): {'grad_norm': 8, 'grad/mlp1.bias': 4, 'grad/fc1.bias': 4},
        ('packed_valu', 1): {'grad_norm': 8, 'grad/mlp1.bias': 4},
    },
    'vdn_learn_10d_od32.npz': {
        ('fused_td', 0): {'grad/conv1.weight': 4, 'w/conv1.weight': 4, 'grad/conv1.bias': 8, 'grad/rnn.weight_ih': 4,
            'grad/rnn.weight_hh': 4},
        ('fused_td', 1): {'w/conv1.weight': 4},
        ('host_len_bound', 0): {'grad/conv1.weight': 4, 'w/conv1.weight': 4, 'grad/conv1.bias': 8, 'grad/rnn.weight_ih': 4,
            'grad/rnn.weight_hh': 4},
        ('host_len_bound', 1): {'w/conv1.weight': 4},
        ('packed', 0): {'grad/conv1.weight': 4, 'w/conv1.weight': 4, 'grad/conv1.bias': 4, 'grad/rnn.weight_ih': 4,
            'grad/rnn.weight_hh': 4},
        ('packed', 1): {'w/conv1.weight': 4},
        ('packed_valu', 0): {'grad/conv1.weight': 4, 'w/conv1.weight': 4, 'grad/conv1.bias': 8, 'grad/rnn.weight_ih': 4,
            'grad/rnn.weight_hh': 4},
        ('packed_valu', 1): {'w/conv1.weight': 4},
    },
    'vdn_learn_meda_4d_od32.npz': {
        ('fused_td', 0): {'w/conv1.weight': 4, 'grad/rnn.weight_ih': 4, 'w/rnn.weight_ih': 8, 'grad/rnn.weight_hh': 4},
        ('fused_td', 1): {'w/conv1.bias': 8, 'grad/conv2.bias': 4, 'grad/mlp1.bias': 4},
        ('host_len_bound', 0): {'w/conv1.weight': 4, 'grad/rnn.weight_ih': 4, 'w/rnn.weight_ih': 8, 'grad/rnn.weight_hh': 4},
        ('host_len_bound', 1): {'w/conv1.bias': 8, 'grad/conv2.bias': 4, 'grad/mlp1.bias': 4},
        ('packed', 0): {'grad/conv1.bias': 4, 'w/conv2.weight': 4, 'w/rnn.weight_ih': 8, 'grad/rnn.weight_hh': 4},
        ('packed', 1): {'loss': 4, 'grad/conv1.weight': 8, 'w/conv1.weight': 4, 'grad/conv1.bias': 4, 'w/conv1.bias': 8,
            'grad/conv2.weight': 8, 'w/conv2.weight': 4, 'grad/conv2.bias': 8, 'w/conv2.bias': 4, 'grad/mlp1.weight': 4,
            'grad/mlp1.bias': 8, 'grad/rnn.weight_ih': 4, 'w/rnn.weight_ih': 16, 'grad/rnn.weight_hh': 4, 'grad/rnn.bias_ih': 4,
            'grad/rnn.bias_hh': 8, 'w/rnn.bias_hh': 4, 'grad/fc1.weight': 4, 'w/fc1.weight': 4, 'grad/fc1.bias': 4},
        ('packed_valu', 0): {'loss': 128, 'w/conv1.weight': 4, 'w/rnn.weight_ih': 8, 'grad/rnn.weight_hh': 4},
        ('packed_valu', 1): {'loss': 4, 'grad/conv1.weight': 4, 'grad/conv1.bias': 4, 'w/conv1.bias': 8, 'grad/conv2.weight': 4,
            'grad/conv2.bias': 4, 'grad/mlp1.bias': 4, 'grad/rnn.weight_hh': 4, 'grad/rnn.bias_ih': 4, 'grad/rnn.bias_hh': 4},
    },
    'vdn_learn_4d_od24_b64.npz': {
        ('packed', 1): {'w/fc1.bias': 4},
    },
    'fovlearn_4d_od24_fov5.npz': {
        ('packed', 0): {'loss': 8, 'w/conv1.weight': 4, 'grad/rnn.weight_ih': 8, 'grad/rnn.weight_hh': 4},
        ('packed', 1): {'grad/rnn.weight_ih': 4, 'grad/fc1.bias': 4},
        ('fused_td', 0): {'w/conv1.weight': 4, 'grad/rnn.weight_ih': 8, 'grad/rnn.weight_hh': 4},
        ('fused_td', 1): {'grad/rnn.weight_ih': 4},
    },
    'fovlearn_3d_od32_fov7.npz': {
        ('packed', 0): {'grad/conv1.bias': 4, 'grad/conv2.bias': 4, 'grad/mlp1.weight': 4, 'grad/rnn.weight_ih': 4,
            'grad/rnn.weight_hh': 4, 'grad/fc1.weight': 4},
        ('packed', 1): {'w/rnn.bias_hh': 4},
        ('fused_td', 0): {'grad/mlp1.weight': 4, 'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'grad/fc1.weight': 4},
        ('fused_td', 1): {'w/rnn.bias_hh': 4},
    },
    'fovlearn_4d_od24_fov11.npz': {
        ('packed', 0): {'grad/conv2.bias': 4, 'grad/mlp1.bias': 4, 'grad/rnn.weight_ih': 8, 'grad/rnn.weight_hh': 4,
            'w/rnn.bias_hh': 4},
        ('packed', 1): {'w/mlp1.bias': 4, 'grad/rnn.weight_ih': 4},
        ('fused_td', 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4},
        ('fused_td', 1): {'w/mlp1.bias': 4, 'w/rnn.weight_hh': 4},
    },
    'fovlearn_3d_od32_fov13.npz': {
        ('packed', 0): {'grad/conv1.weight': 4, 'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4},
        ('packed', 1): {'loss': 4},
        ('fused_td', 0): {'grad/conv1.weight': 4, 'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4},
    },
}


def path_factors(name, path, step):
    """The exceptions of FACTORS for one golden (file name), learn path and learn."""
    return FACTORS.get(name, {}).get((path, step), {})


def golden_path(name):
    return os.path.join(GOLDEN, name)


def golden_config(g):
    """(name, W, L, n_agents, fov, od, clip, n_actions) of a learn golden (tools/oracle/gen_vdn_golden.py: cfg)."""
    cfg = [int(v) for v in g['cfg']]
    W, L, n, fov, od, clip = cfg[:6]
    return ('meda', W, L, n, fov, od, clip, cfg[6]) if len(cfg) == 8 else ('dmfb', W, L, n, fov, od, clip, 5)


def _holder(fov, od, n_actions):
    """The parameter tensors of the Q-network in `named_parameters()` order of the CRNN (conv1[, conv2], mlp1, rnn, fc1), held in
    bare torch.nn modules only so that `det_init` can fill them; the arithmetic below never calls these modules."""
    m = torch.nn.Module()
    size = fov
    for k, (name, stride) in enumerate(_STACK[fov]):
        if not hasattr(m, name):
            m.add_module(name, torch.nn.Conv2d(3 if k == 0 else od, od, kernel_size=3, stride=stride))
        size = (size - 3) // stride + 1
    m.add_module('mlp1', torch.nn.Linear(2 + n_actions, 10))
    m.add_module('rnn', torch.nn.GRUCell(size * size * od + 10, HIDDEN))
    m.add_module('fc1', torch.nn.Linear(HIDDEN, n_actions))
    return m


def make_weights(fov, od, n_actions, salt, dtype):
    m = _holder(fov, od, n_actions)
    det_init(m, salt=salt)
    return {name: p.detach().to(dtype).clone() for name, p in m.named_parameters()}


def q_network(P, fov, inputs, h):
    """One step of the per-agent Q-network: inputs (R, 3*fov*fov + 2 + A) = [image, dir_x, dir_y, last action one-hot], h (R, 128)
    -> (q (R, A), h')."""
    n_pix = 3 * fov * fov
    x = inputs[:, :n_pix].reshape(-1, 3, fov, fov)
    for name, stride in _STACK[fov]:
        x = f.relu(f.conv2d(x, P[name + '.weight'], P[name + '.bias'], stride=stride))
    vec = f.relu(f.linear(inputs[:, n_pix:], P['mlp1.weight'], P['mlp1.bias']))
    x = torch.cat([x.reshape(x.shape[0], -1), vec], dim=1)
    # GRUCell: gates in the order reset, update, new
    gi = f.linear(x, P['rnn.weight_ih'], P['rnn.bias_ih'])
    gh = f.linear(h, P['rnn.weight_hh'], P['rnn.bias_hh'])
    i_r, i_z, i_n = gi.chunk(3, dim=1)
    h_r, h_z, h_n = gh.chunk(3, dim=1)
    r = torch.sigmoid(i_r + h_r)
    z = torch.sigmoid(i_z + h_z)
    new = torch.tanh(i_n + r * h_n)
    h = new + z * (h - new)
    return f.linear(h, P['fc1.weight'], P['fc1.bias']), h


def _step_inputs(batch, t, rows):
    """Network input of step t: o[:, 0] with a zero last action at t == 0, else o_next[:, t-1] with u_onehot[:, t-1]."""
    if t == 0:
        obs, last = batch['o'][:, 0], torch.zeros_like(batch['u_onehot'][:, 0])
    else:
        obs, last = batch['o_next'][:, t - 1], batch['u_onehot'][:, t - 1]
    return torch.cat([obs.reshape(rows, -1), last.reshape(rows, -1)], dim=1)


def agent_q_values(batch, P_eval, P_target, fov):
    """Both Q-networks unrolled over the (already trimmed) batch -> (Q of the action taken (B, T, n), with a graph that reaches
    P_eval; the target network's best available next Q (B, T, n), no graph): what a learn hands its mixers."""
    B, T, n = batch['o'].shape[:3]
    rows = B * n
    dtype = batch['o'].dtype
    h_e = torch.zeros((rows, HIDDEN), dtype=dtype)
    h_t = torch.zeros((rows, HIDDEN), dtype=dtype)
    q_evals, q_targets = [], []
    inputs = _step_inputs(batch, 0, rows)
    for t in range(T):                       # the hidden states run on through padded steps
        inputs_next = _step_inputs(batch, t + 1, rows)
        q_e, h_e = q_network(P_eval, fov, inputs, h_e)
        with torch.no_grad():
            q_t, h_t = q_network(P_target, fov, inputs_next, h_t)
        q_evals.append(q_e.view(B, n, -1))
        q_targets.append(q_t.view(B, n, -1))
        inputs = inputs_next
    q_evals, q_targets = torch.stack(q_evals, dim=1), torch.stack(q_targets, dim=1)      # (B, T, n, A)
    chosen = torch.gather(q_evals, 3, batch['u']).squeeze(3)
    best_next = q_targets.masked_fill(batch['avail_u_next'] == 0, -9999999).max(dim=3)[0]
    return chosen, best_next


def learn_once(batch, P_eval, P_target, fov, gamma):
    """loss of one VDN learn on the (already trimmed) batch; the graph reaches the tensors of P_eval only."""
    chosen, best_next = agent_q_values(batch, P_eval, P_target, fov)
    q_tot, q_tot_target = chosen.sum(dim=2, keepdim=True), best_next.sum(dim=2, keepdim=True)   # the VDN mixer
    targets = batch['r'] + gamma * q_tot_target * (1 - batch['terminated'])
    mask = 1 - batch['padded']
    return ((mask * (targets.detach() - q_tot)) ** 2).sum() / mask.sum()


def load_batch(g, dtype, episode_order=None, keys=BATCH_KEYS):
    """The golden's minibatch as the reference's learn sees it: everything in `dtype` but the integer actions, the rewards
    rounded to float32 first, trimmed to the batch's own longest episode (1 + the largest index of a first terminated step).
    keys: BATCH_KEYS, or with the global states 's' / 's_next' behind them (tests/qmix_learn_f64.py)."""
    order = None if episode_order is None else torch.as_tensor(np.asarray(episode_order, dtype=np.int64))
    batch = {}
    for k in keys:
        v = torch.as_tensor(g[k])
        if order is not None:
            v = v[order]
        batch[k] = v.long() if k == 'u' else v.to(torch.float32).to(dtype)
    term = batch['terminated'][:, :, 0] == 1
    assert bool(term.any(dim=1).all())
    T = int(term.int().argmax(dim=1).max()) + 1
    return {k: v[:, :T] for k, v in batch.items()}


def reference_learn(path, dtype, episode_order=None):
    """The two consecutive learns of a golden (train_step 0 and 1, no target update) -> for each a dict with 'loss' and
    'grad_norm' (the norm before clipping) as Python floats, 'grad' {name: the whole clipped gradient} and 'w' {name: the whole
    weight tensor after the Adam step}, tensors in `dtype` on the CPU."""
    return with_threads(_reference_learn, path, dtype, episode_order)


def _reference_learn(path, dtype, episode_order):
    from marl_dmfb_amd.common.arguments import make_args
    g = np.load(path)
    kind, W, L, n, fov, od, clip, A = golden_config(g)
    args = make_args(name=kind, drop_num=n, width=W, length=L, fov=fov, cuda=False)      # hyper-parameters only
    assert args.hyper_hidden_dim == od and args.grad_norm_clip == clip and args.rnn_hidden_dim == HIDDEN and args.optimizer == 'ADAM'
    P_eval, P_target = make_weights(fov, od, A, 0.0, dtype), make_weights(fov, od, A, 0.5, dtype)
    assert list(P_eval) == [str(x) for x in g['names']]
    return two_learns(P_eval, list(P_eval.values()), args,
                      lambda: learn_once(load_batch(g, dtype, episode_order), P_eval, P_target, fov, args.gamma))


def with_threads(fn, *a):
    """fn(*a) on THREADS intra-op threads."""
    threads = torch.get_num_threads()
    torch.set_num_threads(THREADS)
    try:
        return fn(*a)
    finally:
        torch.set_num_threads(threads)


def two_learns(named, params, args, loss_fn):
    """Two consecutive learns (backward, ONE clip_grad_norm_ and ONE Adam over `params`, in that order: VDN.__init__) of the loss
    `loss_fn()` builds on the tensors of `named` {name: tensor}, which are reported under their names."""
    for p in params:
        p.requires_grad_(True)
    opt = torch.optim.Adam(params, lr=args.lr, betas=(0.9, 0.99))
    out = []
    for step in range(2):
        loss = loss_fn()
        opt.zero_grad()
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(params, args.grad_norm_clip)
        opt.step()
        out.append({'loss': float(loss.detach()), 'grad_norm': float(norm),
                    'grad': {k: p.grad.detach().clone() for k, p in named.items()},
                    'w': {k: p.detach().clone() for k, p in named.items()}})
    return out


# ---------------------------------------------------------------------------------------------------------------- comparisons
def full_error(x, x64):
    """(max|x - x64| / max|x64|, relative L2, all finite) of a whole tensor against the float64 one."""
    x = torch.as_tensor(x).detach().cpu().to(torch.float64).reshape(-1)
    ref = x64.reshape(-1)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    d = x - ref
    return float(d.abs().max() / ref.abs().max()), float(d.norm() / ref.norm()), bool(torch.isfinite(x).all())


def scalar_error(x, x64):
    return abs(float(x) - x64) / abs(x64)


def episode_orders(B, count=N_ORDERS):
    orders = [np.arange(B)]
    for seed in range(1, count):
        perm = np.random.default_rng(seed).permutation(B)
        assert not np.array_equal(perm, orders[0])
        orders.append(perm)
    return orders


_ENVELOPES = {}


def envelope(path):
    """{'ref': the float64 `reference_learn`, 'E': per step {'grad': {name: E_ref}, 'w': {name: E_ref}, 'grad_norm': E_ref,
    'loss': E_ref}, 'E_l2': the same shape for the relative L2 error (tensors only), 'runs32': the float32 runs}, with E_ref the
    largest error of N_ORDERS float32 runs of the restatement against the float64 one (`full_error` / `scalar_error`).  Computed
    once per golden and process."""
    return envelope_of(os.path.basename(path), lambda dtype, order: reference_learn(path, dtype, order), np.load(path)['o'].shape[0])


def envelope_of(key, learn, B):
    """`envelope` for any restated learn: learn(dtype, episode_order) -> what `reference_learn` returns, B episodes in the batch;
    cached under `key`."""
    if key not in _ENVELOPES:
        ref = learn(torch.float64, None)
        runs = [learn(torch.float32, None if k == 0 else order) for k, order in enumerate(episode_orders(B))]
        E, E_l2 = [], []
        for step in range(2):
            errs = {kind: {name: [full_error(run[step][kind][name], x64) for run in runs] for name, x64 in ref[step][kind].items()}
                    for kind in ('grad', 'w')}
            e = {kind: {name: max(v[0] for v in vs) for name, vs in errs[kind].items()} for kind in ('grad', 'w')}
            E_l2.append({kind: {name: max(v[1] for v in vs) for name, vs in errs[kind].items()} for kind in ('grad', 'w')})
            for kind in ('grad_norm', 'loss'):
                e[kind] = max(scalar_error(run[step][kind], ref[step][kind]) for run in runs)
            E.append(e)
        _ENVELOPES[key] = {'ref': ref, 'E': E, 'E_l2': E_l2, 'runs32': runs}
    return _ENVELOPES[key]


def compare_step(label, step, env, grad_norm, loss, tensors, factors=None):
    """The full-tensor check of one learn: `tensors` yields (name, whole gradient, whole weight tensor).  Prints one line per
    tensor with err, E_ref and err / E_ref (and the same three for the relative L2 error, which is reported only), and returns the
    violations of err <= factor x E_ref (or of finiteness) as strings.  factors: {'grad/<name>' | 'w/<name>' | 'grad_norm' |
    'loss': factor} of this path and learn where it is not FACTOR (`path_factors`)."""
    ref, E, E_l2 = env['ref'][step], env['E'][step], env['E_l2'][step]
    factors = factors or {}
    bad = []

    def report(what, err, e_ref, l2, l2_ref, finite=True):
        factor = factors.get(what, FACTOR)
        line = 'learn_f64 %s step %d %-18s err %.3e E_ref %.3e ratio %6.2f (factor %g) | relL2 %.3e E_ref %.3e ratio %5.2f' % (
            label, step, what, err, e_ref, err / e_ref, factor, l2, l2_ref, l2 / l2_ref)
        print(line)
        if not finite or not err <= factor * e_ref:
            bad.append(line + ('' if finite else ' NOT FINITE'))

    e = scalar_error(grad_norm, ref['grad_norm'])
    report('grad_norm', e, E['grad_norm'], e, E['grad_norm'], np.isfinite(float(grad_norm)))
    e = scalar_error(loss, ref['loss'])
    report('loss', e, E['loss'], e, E['loss'], np.isfinite(float(loss)))
    for name, grad, w in tensors:
        for kind, x in (('grad', grad), ('w', w)):
            err, l2, finite = full_error(x, ref[kind][name])
            report('%s/%s' % (kind, name), err, E[kind][name], l2, E_l2[kind][name], finite)
    return bad
