"""A plain restatement of the reference's QMIX learn (policy/qmix.py:79-128 with the mixer of network/qmix_net.py, two
hypernetwork layers) on top of tests/learn_f64.py, on the CPU, in float64 (ground truth) or float32 (the reference's own
arithmetic).  Helper module: no tests in it.

The Q-network half, the batch loading, the two-learn loop, the envelope and the comparisons are learn_f64's; what is written out
here is the mixer (`mixer`: torch.nn.functional calls on a dict of tensors), the TD rule with the two mixers in the place of the
VDN sums (`qmix_learn_once`) and the batches.  Nothing of the package's networks or learners is imported: `make_args` gives the
hyper-parameters.  The weights are the tests' closed formula: `make_weights(salt 0.0 / 0.5)` for the Q-networks, `det_init(...,
salt=0.3)` for the eval mixer on a bare torch.nn holder with the reference's module names, the target mixer a copy.  ONE Adam
and ONE clip_grad_norm_ run over mixer and Q-network parameters together, the mixer's first (VDN.__init__: eval_parameters).

Batches (SPECS): the two reference goldens tests/golden/qmix_learn_*.npz (batch tensors of their `source` VDN golden, states
`s` / `s_next` of the golden itself; tests/test_qmix_learn_f64_reference.py ties the restatement to the reference's numbers on
them) and three batches the reference has no golden for -- MEDA (9 actions, fov 19; the reference's MEDA env has no global state)
and fov 5 / fov 13 with 4 / 3 droplets -- whose batch tensors are those of a VDN golden (which ties their Q-network half) and
whose states are SYNTHETIC: one int8 (B, T + 1, S) tensor from numpy.random.default_rng(seed), s = st[:, :T], s_next = st[:, 1:]
(the ring relation s[t + 1] == s_next[t] by construction), an entry non-zero with probability 0.03 (the DMFB goldens: 2.5 %),
non-zero values uniform in 1..10, one in twenty of them negated.  These rows are not states an env would emit and do not have to
be: the mixer is a function of any `s`, the kernels' contract is int8, and a sign-extension slip in an int8 -> float conversion is
invisible on real, non-negative states.

`qmix_envelope(spec)` is `learn_f64.envelope` for these learns: five float32 runs (episodes in the identity order and four
seeded permutations) against the float64 run, cached per process.  tests/test_gpu_qmix_learn_f64.py bounds every shipped QMIX
learn path by it; QMIX_FACTORS holds the rows with a factor other than learn_f64.FACTOR."""
import numpy as np
import torch
import torch.nn.functional as f

import learn_f64
from learn_f64 import BATCH_KEYS, golden_config, golden_path, load_batch, make_weights
from vdn_helpers import det_init

MIX = 'mix.'                     # prefix of the mixer's tensors in what `qmix_reference_learn` returns
QMIX_HIDDEN = 32
# name -> (file with the batch tensors or, for a reference golden, the QMIX golden that names it as `source`; S; seed of the
# synthetic states or None for the golden's own)
SPECS = {'qmix_learn_4d_od24': ('qmix_learn_4d_od24.npz', 300, None),
         'qmix_learn_10d_od32': ('qmix_learn_10d_od32.npz', 1200, None),
         'meda_4d_od32': ('vdn_learn_meda_4d_od32.npz', 2 * 30 * 30, 11),
         'fov5_4d_od24': ('fovlearn_4d_od24_fov5.npz', 3 * 10 * 10, 12),
         'fov13_3d_od32': ('fovlearn_3d_od32_fov13.npz', 3 * 16 * 16, 13)}
REFERENCE_GOLDENS = [k for k, v in SPECS.items() if v[2] is None]
STATE_KEYS = BATCH_KEYS + ['s', 's_next']

# spec -> (path, learn) -> {tensor: factor}: the rows of tests/test_gpu_qmix_learn_f64.py whose bound is not learn_f64.FACTOR
# but the next power of two above the measured err / E_ref, by the rule and on the evidence of profiles/learn_f64/NOTES.md
# (section QMIX; tools/diag_learn_f64.py qmix reruns it).  No tensor row may exceed MAX_TENSOR_FACTOR.
MAX_TENSOR_FACTOR = 16
QMIX_FACTORS = {
    'qmix_learn_4d_od24': {
        ('fused_ring', 0): {'grad/rnn.weight_ih': 8, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'grad/mix.hyper_w2.2.bias': 4},
        ('fused_ring', 1): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_ih': 4,
            'w/rnn.bias_hh': 4},
        ('fused_two_tensors', 0): {'grad/rnn.weight_ih': 8, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4,
            'grad/mix.hyper_w2.2.bias': 4},
        ('fused_two_tensors', 1): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_ih': 4,
            'w/rnn.bias_hh': 4},
        ('torch_ops', 0): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'grad/fc1.weight': 4},
        ('torch_ops', 1): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_hh': 4},
        ('packed', 0): {'grad/rnn.weight_ih': 8, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'grad/mix.hyper_w1.2.bias': 4},
        ('packed', 1): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_hh': 4},
        ('packed_valu', 0): {'grad/rnn.weight_ih': 8, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4},
        ('packed_valu', 1): {'grad/rnn.weight_ih': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.weight_hh': 4, 'w/rnn.bias_hh': 4},
    },
    'qmix_learn_10d_od32': {
        ('fused_ring', 0): {'w/conv1.weight': 16, 'w/conv2.weight': 4, 'w/rnn.weight_hh': 4, 'w/mix.hyper_b1.weight': 4},
        ('fused_ring', 1): {'w/conv1.weight': 16, 'w/conv2.weight': 4, 'grad/conv2.bias': 4, 'w/mlp1.bias': 4,
            'grad/rnn.weight_ih': 4, 'w/rnn.weight_hh': 4, 'grad/rnn.bias_ih': 4},
        ('fused_two_tensors', 0): {'w/conv1.weight': 16, 'w/conv2.weight': 4, 'w/rnn.weight_hh': 4, 'w/mix.hyper_b1.weight': 4},
        ('fused_two_tensors', 1): {'w/conv1.weight': 16, 'w/conv2.weight': 4, 'grad/conv2.bias': 4, 'grad/mlp1.weight': 4,
            'grad/mlp1.bias': 4, 'w/mlp1.bias': 4, 'grad/rnn.weight_ih': 4, 'w/rnn.weight_hh': 4, 'grad/rnn.bias_ih': 4},
        ('torch_ops', 0): {'w/conv1.weight': 16, 'grad/mix.hyper_w1.0.weight': 4, 'w/mix.hyper_w1.0.weight': 4,
            'w/mix.hyper_b1.weight': 8, 'w/mix.hyper_b2.0.weight': 8},
        ('torch_ops', 1): {'w/conv1.weight': 8, 'grad/conv2.bias': 4, 'grad/rnn.bias_ih': 4, 'w/mix.hyper_w1.0.weight': 4,
            'grad/mix.hyper_w1.2.weight': 4, 'w/mix.hyper_b1.weight': 4, 'w/mix.hyper_b2.0.weight': 8},
        ('packed', 0): {'grad/conv1.weight': 4, 'w/mlp1.weight': 4, 'w/rnn.weight_hh': 4, 'w/mix.hyper_w1.0.weight': 4,
            'grad/mix.hyper_w1.2.bias': 4, 'w/mix.hyper_b1.weight': 4},
        ('packed', 1): {'grad/conv2.bias': 4, 'grad/mlp1.weight': 4, 'grad/mlp1.bias': 4, 'w/mlp1.bias': 4, 'w/rnn.weight_hh': 4,
            'grad/rnn.bias_ih': 4, 'w/mix.hyper_w1.0.weight': 4},
        ('packed_valu', 0): {'w/conv1.weight': 16, 'w/conv2.weight': 4, 'w/rnn.weight_hh': 4, 'w/mix.hyper_b1.weight': 4},
        ('packed_valu', 1): {'w/conv1.weight': 16, 'w/conv2.weight': 4, 'grad/conv2.bias': 4, 'grad/mlp1.weight': 4,
            'grad/mlp1.bias': 4, 'w/mlp1.bias': 4, 'grad/rnn.weight_ih': 4, 'w/rnn.weight_hh': 4, 'grad/rnn.bias_ih': 4},
    },
    'meda_4d_od32': {
        ('fused_ring', 0): {'loss': 4, 'grad/conv2.bias': 4, 'w/mix.hyper_b1.weight': 4},
        ('fused_ring', 1): {'w/conv2.bias': 4, 'w/mix.hyper_b1.weight': 4, 'grad/mix.hyper_b1.bias': 4},
        ('torch_ops', 0): {'w/conv2.weight': 4, 'grad/conv2.bias': 4},
        ('torch_ops', 1): {'w/conv2.weight': 4, 'grad/fc1.weight': 4, 'grad/mix.hyper_b1.bias': 4},
        ('packed', 0): {'loss': 4, 'grad/conv2.weight': 4, 'grad/conv2.bias': 4, 'grad/mlp1.bias': 4, 'w/mix.hyper_b1.weight': 4},
        ('packed', 1): {'w/conv2.bias': 4, 'w/mix.hyper_b1.weight': 4, 'grad/mix.hyper_b1.bias': 4},
    },
    'fov5_4d_od24': {
        ('fused_ring', 0): {'grad/conv1.weight': 4, 'grad/conv1.bias': 4, 'w/mlp1.weight': 8, 'grad/mlp1.bias': 4,
            'w/mlp1.bias': 4, 'grad/rnn.weight_ih': 4, 'w/mix.hyper_b1.weight': 4},
        ('fused_ring', 1): {'w/mlp1.bias': 8},
        ('packed', 0): {'grad/conv1.weight': 4, 'grad/mlp1.weight': 4, 'w/mlp1.weight': 4, 'grad/mlp1.bias': 4, 'w/mlp1.bias': 8,
            'grad/rnn.weight_ih': 4, 'w/mix.hyper_b1.weight': 4},
        ('packed', 1): {'w/mlp1.bias': 16, 'grad/rnn.weight_ih': 4},
    },
    'fov13_3d_od32': {
        ('fused_ring', 0): {'w/conv1.weight': 4, 'grad/rnn.weight_hh': 4, 'w/rnn.bias_ih': 8, 'w/rnn.bias_hh': 8},
        ('fused_ring', 1): {'w/conv1.weight': 4, 'w/rnn.bias_ih': 8, 'w/rnn.bias_hh': 8, 'w/mix.hyper_w1.2.weight': 4},
        ('packed', 0): {'grad/rnn.weight_hh': 4, 'grad/rnn.bias_ih': 4, 'w/rnn.bias_ih': 4, 'w/rnn.bias_hh': 4},
        ('packed', 1): {'w/conv1.bias': 4, 'w/rnn.bias_ih': 4, 'w/rnn.bias_hh': 4},
    },
}


def qmix_path_factors(spec, path, step):
    """The exceptions of QMIX_FACTORS for one batch, learn path and learn."""
    return QMIX_FACTORS.get(spec, {}).get((path, step), {})


def synthetic_states(B, T, S, seed):
    """int8 (B, T + 1, S): see the module docstring."""
    rng = np.random.default_rng(seed)
    shape = (B, T + 1, S)
    value = rng.integers(1, 11, size=shape)
    value = np.where(rng.random(shape) < 0.05, -value, value)
    return np.where(rng.random(shape) < 0.03, value, 0).astype(np.int8)


_BATCHES = {}


def load_spec(spec):
    """{the batch tensors, 's', 's_next' (int8), 'cfg' and 'names' of the VDN golden; 'qmix': the QMIX golden or None}."""
    if spec not in _BATCHES:
        name, S, seed = SPECS[spec]
        q = None
        if seed is None:
            q = dict(np.load(golden_path(name)))
            name = str(q['source'])
        src = np.load(golden_path(name))
        g = {k: src[k] for k in BATCH_KEYS + ['cfg', 'names']}
        B, T = g['o'].shape[:2]
        if q is None:
            st = synthetic_states(B, T, S, seed)
            g['s'], g['s_next'] = st[:, :T], st[:, 1:]
        else:
            g['s'], g['s_next'] = q['s'], q['s_next']
        assert g['s'].dtype == np.int8 and g['s'].shape == g['s_next'].shape == (B, T, S)
        g['qmix'] = q
        _BATCHES[spec] = g
    return _BATCHES[spec]


def spec_config(spec):
    """(kind, W, L, n_agents, fov, hyper_hidden_dim, clip, n_actions, S) of a batch."""
    kind, W, L, n, fov, od, clip, A = golden_config(load_spec(spec))
    S = SPECS[spec][1]
    assert S == (2 if kind == 'meda' else 3) * W * L
    return kind, W, L, n, fov, od, clip, A, S


# ------------------------------------------------------------------------------------------------------------------ the mixer
def _mixer_holder(S, hh, n):
    """The parameter tensors of QMixNet with two hypernetwork layers, under the reference's module names and in its
    `named_parameters()` order, in bare torch.nn modules only so that `det_init` can fill them."""
    nn = torch.nn
    m = nn.Module()
    m.add_module('hyper_w1', nn.Sequential(nn.Linear(S, hh), nn.ReLU(), nn.Linear(hh, n * QMIX_HIDDEN)))
    m.add_module('hyper_w2', nn.Sequential(nn.Linear(S, hh), nn.ReLU(), nn.Linear(hh, QMIX_HIDDEN)))
    m.add_module('hyper_b1', nn.Linear(S, QMIX_HIDDEN))
    m.add_module('hyper_b2', nn.Sequential(nn.Linear(S, QMIX_HIDDEN), nn.ReLU(), nn.Linear(QMIX_HIDDEN, 1)))
    return m


def make_mixer_weights(S, hh, n, dtype):
    m = _mixer_holder(S, hh, n)
    det_init(m, salt=0.3)
    return {name: p.detach().to(dtype).clone() for name, p in m.named_parameters()}


def mixer(PM, q, s):
    """QMixNet.forward (network/qmix_net.py, two hypernetwork layers): q (B, T, n), s (B, T, S) -> q_tot (B, T, 1)."""
    B, n = q.shape[0], q.shape[-1]
    q = q.reshape(-1, 1, n)
    s = s.reshape(-1, s.shape[-1])

    def two(name):
        hidden = f.relu(f.linear(s, PM[name + '.0.weight'], PM[name + '.0.bias']))
        return f.linear(hidden, PM[name + '.2.weight'], PM[name + '.2.bias'])
    w1 = torch.abs(two('hyper_w1')).view(-1, n, QMIX_HIDDEN)
    b1 = f.linear(s, PM['hyper_b1.weight'], PM['hyper_b1.bias']).view(-1, 1, QMIX_HIDDEN)
    hidden = f.elu(torch.bmm(q, w1) + b1)
    w2 = torch.abs(two('hyper_w2')).view(-1, QMIX_HIDDEN, 1)
    b2 = two('hyper_b2').view(-1, 1, 1)
    return (torch.bmm(hidden, w2) + b2).view(B, -1, 1)


def qmix_learn_once(batch, P_eval, P_target, PM_eval, PM_target, fov, gamma):
    """loss of one QMIX learn on the (already trimmed) batch: `learn_f64.learn_once` with the two mixers in the place of the VDN
    sums and the TD rule of policy/qmix.py:104-122.  The graph reaches the tensors of P_eval and PM_eval only."""
    chosen, best_next = learn_f64.agent_q_values(batch, P_eval, P_target, fov)
    q_tot = mixer(PM_eval, chosen, batch['s'])
    with torch.no_grad():
        q_tot_target = mixer(PM_target, best_next, batch['s_next'])
    targets = batch['r'] + gamma * q_tot_target * (1 - batch['terminated'])
    td = q_tot - targets.detach()
    mask = 1 - batch['padded']
    return ((mask * td) ** 2).sum() / mask.sum()


def qmix_reference_learn(spec, dtype, episode_order=None):
    """The two consecutive QMIX learns of a batch (train_step 0 and 1, no target update) -> what `learn_f64.reference_learn`
    returns, the Q-network's tensors under their names and the mixer's under MIX + name."""
    return learn_f64.with_threads(_qmix_reference_learn, spec, dtype, episode_order)


def _qmix_reference_learn(spec, dtype, episode_order):
    from marl_dmfb_amd.common.arguments import make_args
    g = load_spec(spec)
    kind, W, L, n, fov, hh, clip, A, S = spec_config(spec)
    args = make_args(name=kind, drop_num=n, width=W, length=L, fov=fov, alg='qmix', cuda=False)      # hyper-parameters only
    assert args.hyper_hidden_dim == hh and args.grad_norm_clip == clip and args.rnn_hidden_dim == learn_f64.HIDDEN
    assert args.qmix_hidden_dim == QMIX_HIDDEN and args.two_hyper_layers and args.optimizer == 'ADAM'
    P_eval, P_target = make_weights(fov, hh, A, 0.0, dtype), make_weights(fov, hh, A, 0.5, dtype)
    PM_eval = make_mixer_weights(S, hh, n, dtype)
    PM_target = {k: v.clone() for k, v in PM_eval.items()}
    assert list(P_eval) == [str(x) for x in g['names']]
    if g['qmix'] is not None:
        assert list(PM_eval) == [str(x) for x in g['qmix']['mixer_names']]
    named = dict(P_eval)
    named.update({MIX + k: v for k, v in PM_eval.items()})
    return learn_f64.two_learns(named, list(PM_eval.values()) + list(P_eval.values()), args, lambda: qmix_learn_once(
        load_batch(g, dtype, episode_order, STATE_KEYS), P_eval, P_target, PM_eval, PM_target, fov, args.gamma))


def qmix_envelope(spec):
    """`learn_f64.envelope` of a QMIX batch: {'ref', 'E', 'E_l2', 'runs32'}, computed once per batch and process."""
    return learn_f64.envelope_of('qmix/' + spec, lambda dtype, order: qmix_reference_learn(spec, dtype, order),
                                 load_spec(spec)['o'].shape[0])


def split_tensors(result):
    """(CRNN tensors, mixer tensors under their own names) of one learn of `qmix_reference_learn`, each as (name, grad, w)."""
    crnn = [(k, v, result['w'][k]) for k, v in result['grad'].items() if not k.startswith(MIX)]
    mix = [(k[len(MIX):], v, result['w'][k]) for k, v in result['grad'].items() if k.startswith(MIX)]
    return crnn, mix
