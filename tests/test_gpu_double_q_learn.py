"""Two learns with double-Q targets (args.double_q) through the shipped GPU learn paths, by the method of
tests/test_gpu_td_lambda_learn.py: every element of every gradient and weight against the float64 restatement of
tests/double_q_f64.py WITH THE PATH'S PICKS GIVEN (err <= factor x E_ref per tensor and learn, E_ref that restatement's own float32
noise over five episode orders, the factor 2 unless `double_q_f64.FACTORS` names another power of two), and the picks themselves
against the float64 restatement's own picks (`double_q_f64.pick_report`: they may differ only at near-ties of the float64 selector).
Goldens: vdn_learn_4d_od24_short.npz with `terminated` cleared on the last valid step of every second episode (in memory: the tail
picks count), vdn_learn_4d_od24_b64.npz as stored; td_lambda 0 and 0.8.  double_q off, or absent, is the current learn bit for bit.
On the edited golden the padded and the packed learn agree in picks and TD errors on every valid step, up to near-ties."""
import numpy as np
import pytest
import torch

import double_q_f64
import learn_f64
from vdn_helpers import learn_golden_setup, learn_golden_step

pytestmark = pytest.mark.gpu

# path name -> (packed, value of MARL_DMFB_GRU_PAIR), as tests/test_gpu_td_lambda_learn.py sets them
PATHS = {'fused_td': (False, None), 'packed': (True, '1')}
GOLDENS = [('vdn_learn_4d_od24_short.npz', True), ('vdn_learn_4d_od24_b64.npz', False)]
LAMBDAS = [0.0, double_q_f64.LAMBDA]
CASES = [(name, edit, path, lam) for name, edit in GOLDENS for path in PATHS for lam in LAMBDAS]


def _pair_env(monkeypatch, pair):
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


@pytest.mark.parametrize('name,edit,path,lam', CASES, ids=['%s%s-%s-lam%g' % (n[:-4], '@edited' if e else '', p, l) for n, e, p, l in CASES])
def test_double_q_learn_matches_float64_in_every_element(name, edit, path, lam, monkeypatch):
    packed, pair = PATHS[path]
    _pair_env(monkeypatch, pair)
    own = double_q_f64.envelope(name, edit, lam)
    g = double_q_f64.edited(np.load(learn_f64.golden_path(name)), edit)
    bad = []
    print()
    for k, run in enumerate(own['runs32']):     # the reference alone stays inside the cap on this golden
        for step in range(2):
            bad += double_q_f64.pick_report('float32 restatement, order %d' % k, run[step]['picks'], own, step, g)
    assert not bad, '\n'.join(bad)
    _, agents = learn_golden_setup(learn_f64.golden_path(name), 'cuda:0')
    policy = agents.policy
    policy.args.double_q, policy.args.td_lambda = True, lam          # after the set-up: the learner reads both at learn time
    policy.double_picks = []
    results, picks = [], []
    for step in range(2):
        order = double_q_f64.learn_step(g, agents, 'cuda:0', step, packed)
        results.append((float(policy.last_grad_norm), float(policy.last_loss),
                        [(k, p.grad.detach().clone(), p.detach().clone()) for k, p in policy.eval_rnn.named_parameters()]))
        p = _golden_order(policy.double_picks[step].cpu().numpy(), order)
        assert p.shape == own['ref'][step]['picks'].shape and p.dtype == np.int8
        valid = np.broadcast_to((g['padded'][:, :p.shape[1], 0] == 0)[:, :, None], p.shape)
        assert (p[valid] >= 0).all() and (not packed or (p[~valid] == -1).all())
        picks.append(np.where(p < 0, own['ref'][step]['picks'], p))      # a step the packed learn does not compute: masked in any case
    policy.check_td_inputs()
    given = double_q_f64.envelope(name, edit, lam, picks)
    label = '%s double_q lam=%g %s%s' % (path, lam, name[:-4], '@edited' if edit else '')
    for step, (norm, loss, tensors) in enumerate(results):
        bad += learn_f64.compare_step(label, step, given, norm, loss, tensors, double_q_f64.path_factors(name, edit, path, lam, step))
        bad += double_q_f64.pick_report(label, picks[step], own, step, g)
    assert not bad, '\n'.join(bad)


def _two_learns(golden, flags, double_q):
    g, agents = learn_golden_setup(golden, 'cuda:0')
    if double_q is None:
        if hasattr(agents.policy.args, 'double_q'):
            del agents.policy.args.double_q
    else:
        agents.policy.args.double_q = double_q
    out = []
    for step in range(2):
        learn_golden_step(g, agents, 'cuda:0', step, **flags)
        policy = agents.policy
        out.append([policy.last_loss.clone(), policy.last_grad_norm.clone()] +
                   [t.detach().clone() for p in policy.eval_rnn.parameters() for t in (p.grad, p)])
    return out


@pytest.mark.parametrize('path', list(PATHS))
def test_double_q_off_is_the_learn_without_the_attribute(path, monkeypatch):
    packed, pair = PATHS[path]
    _pair_env(monkeypatch, pair)
    flags = dict(replay_dtypes=True, packed=True) if packed else dict(replay_dtypes=True)
    golden = learn_f64.golden_path(GOLDENS[0][0])
    without, off = _two_learns(golden, flags, None), _two_learns(golden, flags, False)
    for a, b in zip(without, off):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


class _Spy:
    """Stands in for one of the two TD nodes of policy/vdn.py: records the arguments of every apply, then applies the node."""

    def __init__(self, node, calls):
        self.node, self.calls = node, calls

    def apply(self, *args):
        self.calls.append(args)
        return self.node.apply(*args)


def test_padded_and_packed_agree_in_picks_and_td_errors_on_the_edited_golden(monkeypatch):
    """First learn of the edited short golden at td_lambda 0 through both paths.  Selectors: each path's own, as handed to its TD node,
    against the float64 selector: E_a, E_b.  Picks: the two paths may differ only where the float64 selector's top-two gap is
    <= GAP_FACTOR x max(E_a, E_b).  TD errors: on the valid steps whose picks agree, |mtd_a - mtd_b| <= 8 n (E_a + E_b): a step's error
    adds 2n Q values (n taken, n picked), each off from float64 by about its path's selector error (the same networks on the same
    inputs), times 4, the largest factor the learn tests grant a path over a measured reference error."""
    from marl_dmfb_amd.policy import vdn
    name, edit = GOLDENS[0]
    own = double_q_f64.envelope(name, edit, 0.0)
    g = double_q_f64.edited(np.load(learn_f64.golden_path(name)), edit)
    q64, picks64 = own['ref'][0]['q_sel'], own['ref'][0]['picks']
    B, T, n, A = q64.shape
    valid = g['padded'][:, :T, 0] == 0
    got = {}
    for path, (packed, pair) in PATHS.items():
        _pair_env(monkeypatch, pair)
        calls, mtds = [], []
        real_forward = vdn._td_forward

        def forward(*a, **k):
            out = real_forward(*a, **k)
            mtds.append(out[0])
            return out
        monkeypatch.setattr(vdn, '_td_forward', forward)
        monkeypatch.setattr(vdn, '_TDLossPacked' if packed else '_TDLoss', _Spy(vdn._TDLossPacked if packed else vdn._TDLoss, calls))
        _, agents = learn_golden_setup(learn_f64.golden_path(name), 'cuda:0')
        agents.policy.args.double_q = True
        agents.policy.double_picks = []
        order = double_q_f64.learn_step(g, agents, 'cuda:0', 0, packed)
        monkeypatch.undo()
        assert len(calls) == 1 and len(mtds) == 1
        picks = _golden_order(agents.policy.double_picks[0].cpu().numpy(), order)
        mtd, sel = np.zeros((B, T), np.float32), np.zeros((B, T, n, A), np.float32)
        if packed:
            q_sel, sel_units = calls[0][15].view(-1, n, A).cpu().numpy(), calls[0][16].cpu().numpy()
            lens = valid.sum(1)
            counts = (lens[order][None, :] > np.arange(T)[:, None]).sum(1)
            e = np.concatenate([order[:c] for c in counts])
            t = np.repeat(np.arange(T), counts)
            assert len(e) == len(sel_units) == mtds[0].numel()
            mtd[e, t], sel[e, t] = mtds[0].cpu().numpy(), q_sel[sel_units]
        else:
            mtd = mtds[0].view(B, T).cpu().numpy()
            sel = calls[0][11].view(T, B, n, A).permute(1, 0, 2, 3).cpu().numpy()
        got[path] = (picks, mtd, sel, float(np.abs(sel.astype(np.float64) - q64)[valid].max()))
    (pa, ma, _, ea), (pb, mb, _, eb) = got['fused_td'], got['packed']
    gap = double_q_f64.selector_gap(q64, g['avail_u_next'][:, :T])
    v3 = np.broadcast_to(valid[:, :, None], pa.shape)
    differ = (pa != pb) & v3
    allowed = double_q_f64.GAP_FACTOR * max(ea, eb)
    worst = float(gap[differ].max()) if differ.any() else 0.0
    same = valid & ~differ.any(axis=2)
    err, tol = float(np.abs(ma - mb)[same].max()), 8 * n * (ea + eb)
    print('\nselector errors against float64: fused_td %.3e, packed %.3e; %d of %d valid picks differ (largest gap there %.3e, allowed '
          '%.3e); |mtd_a - mtd_b| <= %.3e on %d steps (bound %.3e)' % (ea, eb, differ.sum(), v3.sum(), worst, allowed, err, same.sum(), tol))
    for p in (pa, pb):
        d64 = (p != picks64) & v3
        assert not d64.any() or float(gap[d64].max()) <= allowed
    assert worst <= allowed and differ.sum() <= double_q_f64.MAX_DIFFER * v3.sum()
    assert same.sum() >= 0.9 * valid.sum() and err <= tol


def _random_weights(agents, seed):
    """The goldens' deterministic weights make every row pick the same action; these make the picks vary.  Returns the weights as
    `double_q_f64.reference_double_learn` takes them."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for net in (agents.policy.eval_rnn, agents.policy.target_rnn):
            for p in net.parameters():
                p.copy_((torch.randn(p.shape, generator=gen) * (0.2 if p.dim() > 1 else 0.02)).to(p.device))
    return tuple({k: p.detach().cpu().clone() for k, p in net.named_parameters()} for net in (agents.policy.eval_rnn, agents.policy.target_rnn))


@pytest.mark.parametrize('path', list(PATHS))
def test_picks_that_vary_agree_with_float64(path, monkeypatch):
    """On the goldens' own weights all picks are one action, so a selector from a wrong step or a wrong hidden state would pick the
    same.  Random weights, first learn of the edited short golden at td_lambda 0: the GPU path's selector, as handed to its TD node,
    and its picks against the float64 restatement of tests/double_q_f64.py run with the same weights (nothing of the package's
    learners in it).  Bound on the selector: 2^-12 x max|q|: float32 dot products of under 2^10 terms, two layers and a recurrence
    of at most 40 steps deep; a selector taken from another step or state is off by the order of max|q| itself.  Picks may differ
    from the float64 picks only where the float64 selector's top-two gap is <= 2 x that bound; at least three different actions must
    be picked; the loss is held to 2^-10 of the float64 loss."""
    from marl_dmfb_amd.policy import vdn
    packed, pair = PATHS[path]
    _pair_env(monkeypatch, pair)
    name, edit = GOLDENS[0]
    g = double_q_f64.edited(np.load(learn_f64.golden_path(name)), edit)
    calls = []
    monkeypatch.setattr(vdn, '_TDLossPacked' if packed else '_TDLoss', _Spy(vdn._TDLossPacked if packed else vdn._TDLoss, calls))
    _, agents = learn_golden_setup(learn_f64.golden_path(name), 'cuda:0')
    weights = _random_weights(agents, 11)
    ref = double_q_f64.reference_double_learn(g, torch.float64, None, 0.0, None, weights)[0]
    sel64, picks64 = ref['q_sel'], ref['picks']
    B, T, n, A = sel64.shape
    valid = g['padded'][:, :T, 0] == 0
    v3 = np.broadcast_to(valid[:, :, None], picks64.shape)
    assert len(np.unique(picks64[v3])) >= 3
    agents.policy.args.double_q = True
    agents.policy.double_picks = []
    order = double_q_f64.learn_step(g, agents, 'cuda:0', 0, packed)
    picks = _golden_order(agents.policy.double_picks[0].cpu().numpy(), order)
    sel = np.zeros(sel64.shape, np.float32)
    if packed:
        q_sel, sel_units = calls[0][15].view(-1, n, A).cpu().numpy(), calls[0][16].cpu().numpy()
        counts = (valid.sum(1)[order][None, :] > np.arange(T)[:, None]).sum(1)
        sel[np.concatenate([order[:c] for c in counts]), np.repeat(np.arange(T), counts)] = q_sel[sel_units]
    else:
        sel = calls[0][11].view(T, B, n, A).permute(1, 0, 2, 3).cpu().numpy()
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
