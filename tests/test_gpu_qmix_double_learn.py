"""Two QMIX learns with double-Q targets (args.qmix_double_q) through the shipped GPU learn paths, by the method of
tests/test_gpu_double_q_learn.py: every element of every gradient and weight of eval_rnn and eval_qmix_net, the loss and the gradient
norm against the float64 restatement of tests/qmix_double_f64.py WITH THE PATH'S PICKS GIVEN (err <= factor x E_ref per tensor and
learn, E_ref that restatement's own float32 noise over five episode orders, the factor learn_f64.FACTOR unless
`qmix_double_f64.FACTORS` names another power of two, at most MAX_TENSOR_FACTOR), and the picks themselves against the float64
restatement's own picks (`double_q_f64.pick_report`: they may differ only at near-ties of the float64 selector; the float32
restatement's own picks are held to the same condition first).  Batches: qmix_learn_4d_od24 with `terminated` cleared on the last
valid step of every second episode (in memory: the tail picks count) through all five paths of qmix_helpers.F64_PATHS at
qmix_lambda 0 and 0.8, fov5_4d_od24 edited through two paths at 0.8, meda_4d_od32 (9 actions) as stored through one at 0.  Each path's
precondition is asserted, never skipped.  qmix_double_q off is, bit for bit, an `args` without the attribute; random weights make the
picks vary."""
import numpy as np
import pytest
import torch

import double_q_f64
import learn_f64
import qmix_double_f64 as QD
import qmix_learn_f64 as Q
from qmix_helpers import F64_PATHS, f64_case_agents

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SPEC = 'qmix_learn_4d_od24'
# (spec, edited, path, lam)
CASES = [(SPEC, True, path, lam) for path in F64_PATHS for lam in (0.0, QD.LAMBDA)] + \
        [('fov5_4d_od24', True, path, QD.LAMBDA) for path in ('fused_ring', 'packed')] + [('meda_4d_od32', False, 'fused_ring', 0.0)]


def _pair_env(monkeypatch, path):
    pair = F64_PATHS[path][2]
    if pair is not None:
        monkeypatch.setenv('MARL_DMFB_GRU_PAIR', pair)
    else:
        monkeypatch.delenv('MARL_DMFB_GRU_PAIR', raising=False)


def _golden_order(x, order):
    """A path's per-episode array back in the golden's episode order."""
    if order is None:
        return x
    out = np.empty_like(x)
    out[order] = x
    return out


def _tensors(pol):
    return [(k, p.grad.detach().clone(), p.detach().clone()) for k, p in pol.eval_rnn.named_parameters()] + \
           [(Q.MIX + k, p.grad.detach().clone(), p.detach().clone()) for k, p in pol.eval_qmix_net.named_parameters()]


@pytest.mark.parametrize('spec,edit,path,lam', CASES, ids=['%s%s-%s-lam%g' % (s, '@edited' if e else '', p, l) for s, e, p, l in CASES])
def test_double_q_learn_matches_float64_in_every_element(spec, edit, path, lam, monkeypatch):
    _pair_env(monkeypatch, path)
    own = QD.envelope(spec, edit, lam)
    g = QD.load_edited(spec, edit)
    bad = []
    print()
    for k, run in enumerate(own['runs32']):     # the restatement alone stays inside the caps on this batch
        for step in range(2):
            bad += double_q_f64.pick_report('float32 restatement, order %d' % k, run[step]['picks'], own, step, g)
    assert not bad, '\n'.join(bad)
    agents = f64_case_agents(Q.load_spec(spec), Q.spec_config(spec), path, DEV)
    pol = agents.policy
    pol.args.qmix_double_q, pol.args.qmix_lambda = True, lam          # after the set-up: the learner reads both at learn time
    pol.double_picks = []
    packed = path.startswith('packed')
    results, picks = [], []
    for step in range(2):
        order = QD.learn_step(g, agents, path, DEV, step)
        results.append((float(pol.last_grad_norm), float(pol.last_loss), _tensors(pol)))
        assert len(pol.double_picks) == step + 1
        p = _golden_order(pol.double_picks[step].cpu().numpy(), order)
        B, T, n = own['ref'][step]['picks'].shape
        assert p.shape == (B, T, n) and p.dtype == np.int8
        valid = np.broadcast_to((g['padded'][:, :T, 0] == 0)[:, :, None], p.shape)
        assert (p[valid] >= 0).all() and (p < pol.n_actions).all() and (~valid).any()
        assert (p[~valid] == -1).all() if packed else (p >= 0).all()        # -1 in the steps a packed learn does not compute
        picks.append(np.where(p < 0, own['ref'][step]['picks'], p))      # a step the packed learn does not compute: masked in any case
    pol.check_td_inputs()
    given = QD.envelope(spec, edit, lam, picks)
    label = '%s qmix_double_q lam=%g %s%s' % (path, lam, spec, '@edited' if edit else '')
    for step, (norm, loss, tensors) in enumerate(results):
        assert [k for k, _, _ in tensors] == list(given['ref'][step]['grad'])
        factors = QD.path_factors(spec, edit, path, lam, step)
        assert all(f <= QD.MAX_TENSOR_FACTOR for f in factors.values())
        bad += learn_f64.compare_step(label, step, given, norm, loss, tensors, factors)
        bad += double_q_f64.pick_report(label, picks[step], own, step, g)
    assert not bad, '\n'.join(bad)


def _two_learns(path, flag):
    g = QD.load_edited(SPEC)
    agents = f64_case_agents(Q.load_spec(SPEC), Q.spec_config(SPEC), path, DEV)
    pol = agents.policy
    if flag is None:
        del pol.args.qmix_double_q
        assert not hasattr(pol.args, 'qmix_double_q')
    else:
        pol.args.qmix_double_q = flag
    out = []
    for step in range(2):
        QD.learn_step(g, agents, path, DEV, step)
        out.append([pol.last_loss.clone(), pol.last_grad_norm.clone()] +
                   [t.detach().clone() for net in (pol.eval_rnn, pol.eval_qmix_net) for p in net.parameters() for t in (p.grad, p)])
    pol.check_td_inputs()
    return out


@pytest.mark.parametrize('path', ['fused_ring', 'packed'])
def test_flag_off_is_the_learn_without_the_attribute(path, monkeypatch):
    _pair_env(monkeypatch, path)
    without, off, on = _two_learns(path, None), _two_learns(path, False), _two_learns(path, True)
    differs = False
    for a, b, c in zip(without, off, on):
        for x, y, z in zip(a, b, c):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
            differs = differs or not torch.equal(x, z)
    assert differs, 'qmix_double_q changed nothing: the comparison above says nothing'


class _Spy:
    """Stands in for one of the two nodes of policy/qmix.py: records the arguments of every apply, then applies the node."""

    def __init__(self, node, calls):
        self.node, self.calls = node, calls

    def apply(self, *args):
        self.calls.append(args)
        return self.node.apply(*args)


def _random_weights(agents, seed):
    """The deterministic weights make every row pick the same action; these make the picks vary.  Returns the weights as
    `qmix_double_f64.reference_double_learn` takes them."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for net in (agents.policy.eval_rnn, agents.policy.target_rnn):
            for p in net.parameters():
                p.copy_((torch.randn(p.shape, generator=gen) * (0.2 if p.dim() > 1 else 0.02)).to(p.device))
    return tuple({k: p.detach().cpu().clone() for k, p in net.named_parameters()} for net in (agents.policy.eval_rnn, agents.policy.target_rnn))


@pytest.mark.parametrize('path', ['fused_ring', 'packed'])
def test_picks_that_vary_agree_with_float64(path, monkeypatch):
    """On the deterministic weights all picks are one action, so a selector from a wrong step or a wrong hidden state would pick the
    same.  Random agent-network weights, first learn of the edited batch at qmix_lambda 0: the GPU path's selector, as handed to its
    node, and its picks against the float64 restatement run with the same weights (nothing of the package's learners in it).  Bound on
    the selector: 2^-12 x max|q|: float32 dot products of under 2^10 terms, two layers and a recurrence of at most 40 steps deep; a
    selector taken from another step or state is off by the order of max|q| itself.  Picks may differ from the float64 picks only where
    the float64 selector's top-two gap is <= 2 x that bound; at least three different actions must be picked; the loss is held to
    2^-10 of the float64 loss."""
    from marl_dmfb_amd.policy import qmix
    _pair_env(monkeypatch, path)
    packed = path == 'packed'
    g = QD.load_edited(SPEC)
    calls = []
    monkeypatch.setattr(qmix, '_MixTDPacked' if packed else '_MixTD', _Spy(qmix._MixTDPacked if packed else qmix._MixTD, calls))
    agents = f64_case_agents(Q.load_spec(SPEC), Q.spec_config(SPEC), path, DEV)
    weights = _random_weights(agents, 11)
    ref = QD.reference_double_learn(SPEC, True, torch.float64, None, 0.0, None, weights)[0]
    sel64, picks64 = ref['q_sel'], ref['picks']
    B, T, n, A = sel64.shape
    valid = g['padded'][:, :T, 0] == 0
    v3 = np.broadcast_to(valid[:, :, None], picks64.shape)
    assert len(np.unique(picks64[v3])) >= 3
    agents.policy.args.qmix_double_q = True
    agents.policy.double_picks = []
    order = QD.learn_step(g, agents, path, DEV, 0)
    assert len(calls) == 1
    picks = _golden_order(agents.policy.double_picks[0].cpu().numpy(), order)
    assert picks.shape == (B, T, n)
    sel = np.zeros(sel64.shape, np.float32)
    if packed:
        q_sel, sel_units = calls[0][24].view(-1, n, A).cpu().numpy(), calls[0][25].cpu().numpy()
        counts = (valid.sum(1)[order][None, :] > np.arange(T)[:, None]).sum(1)
        assert len(sel_units) == counts.sum() and q_sel.shape[0] == counts.sum() + B
        sel[np.concatenate([order[:c] for c in counts]), np.repeat(np.arange(T), counts)] = q_sel[sel_units]
    else:
        sel = calls[0][20].view(T, B, n, A).permute(1, 0, 2, 3).cpu().numpy()
    bound = 2.0 ** -12 * float(np.abs(sel64[valid]).max())
    err = float(np.abs(sel - sel64)[valid].max())
    differ = (picks != picks64) & v3
    gap = double_q_f64.selector_gap(sel64, g['avail_u_next'][:, :T])
    worst = float(gap[differ].max()) if differ.any() else 0.0
    loss, loss64 = float(agents.policy.last_loss), ref['loss']
    print('\n%s: selector error against float64 %.3e (bound %.3e); picks %s; %d of %d differ, largest gap there %.3e; loss %.9g, float64 %.9g'
          % (path, err, bound, np.bincount(picks64[v3].astype(np.int64), minlength=A).tolist(), differ.sum(), v3.sum(), worst, loss, loss64))
    assert err <= bound and worst <= 2 * bound and differ.sum() <= double_q_f64.MAX_DIFFER * v3.sum()
    assert abs(loss - loss64) <= 2.0 ** -10 * abs(loss64)
    agents.policy.check_td_inputs()
