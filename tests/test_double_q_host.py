"""Host side of the double-Q targets (args.double_q): the rule in numpy and in torch ops, the packed learn's selector lists, the flag
and its refusals, and the tensor-op learn on CPU tensors against the float64 restatement of tests/double_q_f64.py.  No GPU needed."""
import numpy as np
import pytest
import torch

import double_q_f64
import learn_f64
from marl_dmfb_amd.common.arguments import get_train_args, make_args
from marl_dmfb_amd.policy.double_q import double_pick_reference, double_pick_torch, selector_units
from vdn_helpers import learn_golden_setup, learn_golden_step

SHORT = 'vdn_learn_4d_od24_short.npz'


def _rows(seed, shape=(6, 9, 4, 5)):
    rng = np.random.default_rng(seed)
    q_sel = rng.standard_normal(shape).astype(np.float32)
    q_target = rng.standard_normal(shape).astype(np.float32)
    avail = (rng.random(shape) < 0.6).astype(np.int8)
    avail[0, 0] = 0                                   # rows with no available action
    q_sel[1, 1] = q_sel[1, 1][..., :1]                # rows with every value equal
    return q_sel, q_target, avail


def test_the_rule_on_rows_written_out():
    f = np.float32
    q_sel = np.array([[[1.0, 3.0, 3.0, 2.0], [5.0, 1.0, 9.0, 2.0], [np.nan, 7.0, 1.0, 0.0], [1.0, np.nan, 0.5, 2.0], [4.0, 4.0, 4.0, 4.0]]], f)
    q_target = np.array([[[10.0, 20.0, 30.0, 40.0]] * 5], f)
    avail = np.array([[[1, 1, 1, 1], [1, 1, 0, 1], [1, 1, 1, 1], [1, 1, 1, 1], [0, 0, 0, 0]]], np.int8)
    picks, q_next = double_pick_reference(q_sel, q_target, avail, f)
    # the first maximum; the largest is unavailable; a NaN in front is never displaced; a NaN behind never displaces; none available: 0
    assert picks.tolist() == [[1, 0, 0, 3, 0]] and picks.dtype == np.int8
    want = f(0)
    for v in (20.0, 10.0, 10.0, 40.0, -9999999.0):
        want = want + f(v)
    assert q_next.dtype == f and q_next[0] == want
    picks64, q64 = double_pick_reference(q_sel, q_target, avail, np.float64)
    assert q64.dtype == np.float64 and np.array_equal(picks64, picks)


def test_selector_equal_to_the_target_is_the_current_rule_bit_for_bit():
    _, q_target, avail = _rows(1)
    q_target[1, 1] = q_target[1, 1][..., :1]
    _, q_next = double_pick_reference(q_target, q_target, avail, np.float32)
    best = np.where(avail == 0, np.float32(-9999999.0), q_target).max(axis=-1)
    want = np.zeros(best.shape[:-1], np.float32)
    for i in range(best.shape[-1]):
        want = want + best[..., i]
    assert np.array_equal(q_next.view(np.int32), want.view(np.int32))


def test_torch_form_is_the_numpy_rule():
    for seed in (2, 3):
        q_sel, q_target, avail = _rows(seed)
        picks, q_next = double_pick_reference(q_sel, q_target, avail, np.float32)
        got_picks, values = double_pick_torch(torch.as_tensor(q_sel), torch.as_tensor(q_target), torch.as_tensor(avail).float())
        assert np.array_equal(got_picks.numpy(), picks)
        tot = values.sum(dim=-1).numpy()                  # the VDN mixer's sum may round in another order: a few ulp
        assert np.abs(tot - q_next).max() <= 4 * 2.0 ** -24 * np.abs(values.numpy()).sum(-1).max()
        want = np.take_along_axis(np.where(avail == 0, np.float32(-9999999.0), q_target), picks.astype(np.int64)[..., None], -1)[..., 0]
        assert np.array_equal(values.numpy().view(np.int32), want.view(np.int32))


def test_selector_units_map_every_unit_to_the_next_one_or_to_its_tail():
    lens = np.array([7, 5, 5, 2, 1])
    counts = (lens[None, :] > np.arange(7)[:, None]).sum(1)
    sel, last = selector_units(counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    U = int(off[-1])
    assert sel.dtype == np.int32 and last.dtype == np.int32 and len(sel) == U == lens.sum() and len(last) == len(lens)
    for t in range(7):
        for e in range(counts[t]):
            assert sel[off[t] + e] == (off[t + 1] + e if t + 1 < lens[e] else U + e)
    assert last.tolist() == [off[l - 1] + e for e, l in enumerate(lens)]
    assert sorted(sel.tolist()) == sorted(set(sel.tolist())) and sel.max() == U + len(lens) - 1


def test_flag_and_default(capsys):
    assert make_args().double_q is False and make_args(double_q=True).double_q is True
    assert get_train_args(['dmfb']).double_q is False and get_train_args(['dmfb', '--double_q']).double_q is True
    assert get_train_args(['dmfb', '--double_q', '--td_lambda', '0.8']).td_lambda == 0.8
    with pytest.raises(SystemExit):
        get_train_args(['dmfb', '--alg', 'qmix', '--double_q'])
    assert 'VDN-only' in capsys.readouterr().err


def test_qmix_refuses_double_q():
    from marl_dmfb_amd.policy.qmix import QMIX
    args = make_args(alg='qmix', cuda=False, double_q=True, n_actions=5, n_agents=4, obs_shape=(3, 9, 9, 2, 245), state_shape=300,
                     episode_limit=40)
    with pytest.raises(ValueError, match=r'double_q.*VDN-only'):
        QMIX(args)


def _two_cpu_learns(double_q):
    g, agents = learn_golden_setup(learn_f64.golden_path(SHORT), 'cpu')
    if double_q is None:
        if hasattr(agents.policy.args, 'double_q'):
            del agents.policy.args.double_q
    else:
        agents.policy.args.double_q = double_q
    agents.policy.double_picks = []
    out = []
    for step in range(2):
        learn_f64.with_threads(learn_golden_step, g, agents, 'cpu', step)
        policy = agents.policy
        out.append([policy.last_loss.clone(), policy.last_grad_norm.clone()] + [t.detach().clone() for p in policy.eval_rnn.parameters() for t in (p.grad, p)])
    return out, agents.policy.double_picks


def test_double_q_off_is_the_learn_without_the_attribute():
    (without, picks_a), (off, picks_b) = _two_cpu_learns(None), _two_cpu_learns(False)
    assert picks_a == [] and picks_b == []
    for a, b in zip(without, off):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    on, picks = _two_cpu_learns(True)
    assert len(picks) == 2 and picks[0].dtype == torch.int8 and picks[0].shape[2] == 4
    assert all(torch.isfinite(x).all() for x in on[0])


@pytest.mark.parametrize('lam', [0.0, double_q_f64.LAMBDA])
@pytest.mark.parametrize('edit', [False, True], ids=['stored', 'edited'])
def test_cpu_double_q_learn_matches_float64_in_every_element(edit, lam):
    """Two learns of the tensor-op path (CPU tensors, padded episodes) with double_q and td_lambda set AFTER the set-up (the learner
    reads both at learn time) against the float64 restatement WITH THE LEARNER'S PICKS GIVEN: err <= factor x E_ref per tensor, E_ref
    that restatement's own float32 noise.  The picks themselves are held to the float64 restatement's own picks by
    `double_q_f64.pick_report` -- which the float32 restatement's own picks must meet first."""
    own = double_q_f64.envelope(SHORT, edit, lam)
    g = double_q_f64.edited(np.load(learn_f64.golden_path(SHORT)), edit)
    bad = []
    print()
    for k, run in enumerate(own['runs32']):
        for step in range(2):
            bad += double_q_f64.pick_report('float32 restatement, order %d' % k, run[step]['picks'], own, step, g)
    assert not bad, 'the reference alone leaves the cap on this golden:\n' + '\n'.join(bad)
    _, agents = learn_golden_setup(learn_f64.golden_path(SHORT), 'cpu')
    policy = agents.policy
    policy.args.double_q, policy.args.td_lambda = True, lam
    policy.double_picks = []
    results = []
    for step in range(2):
        learn_f64.with_threads(double_q_f64.learn_step, g, agents, 'cpu', step)
        results.append((float(policy.last_grad_norm), float(policy.last_loss),
                        [(k, p.grad.detach().clone(), p.detach().clone()) for k, p in policy.eval_rnn.named_parameters()]))
    picks = [p.numpy() for p in policy.double_picks]
    assert len(picks) == 2 and picks[0].shape == own['ref'][0]['picks'].shape
    given = double_q_f64.envelope(SHORT, edit, lam, picks)
    label = 'cpu double_q lam=%g %s%s' % (lam, SHORT[:-4], '@edited' if edit else '')
    for step, (norm, loss, tensors) in enumerate(results):
        bad += learn_f64.compare_step(label, step, given, norm, loss, tensors, double_q_f64.path_factors(SHORT, edit, 'cpu', lam, step))
        bad += double_q_f64.pick_report(label, picks[step], own, step, g)
    if edit:   # the edit makes the tail picks count: without it the loss is the stored golden's wherever it is read
        stored = double_q_f64.envelope(SHORT, False, lam)
        gap = abs(own['ref'][0]['loss'] - stored['ref'][0]['loss']) / abs(own['ref'][0]['loss'])
        print('float64 loss edited %.9g, stored %.9g: relative gap %.3e, E_ref %.3e' % (own['ref'][0]['loss'], stored['ref'][0]['loss'], gap,
                                                                                       given['E'][0]['loss']))
        assert gap > 100 * given['E'][0]['loss']
    assert not bad, '\n'.join(bad)
