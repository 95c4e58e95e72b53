"""Host side of the double-Q targets of the QMIX learn (args.qmix_double_q): the flag, its default and its refusals, double_q still
refused under QMIX, the selector list of a packed learn against the target rows it is taken from, the flag off against a learner
without the attribute, and the tensor-op learn on CPU tensors against the float64 restatement of tests/qmix_double_f64.py.  No GPU
needed."""
import numpy as np
import pytest
import torch

import double_q_f64
import learn_f64
import qmix_double_f64 as QD
import qmix_learn_f64 as Q
from marl_dmfb_amd.common.arguments import get_train_args, make_args
from marl_dmfb_amd.policy.double_q import selector_units
from qmix_helpers import f64_case_agents

SPEC = 'qmix_learn_4d_od24'
PATH = 'torch_ops'           # qmix_helpers.F64_PATHS: on CPU tensors every learn is the tensor-op learn


def test_flag_and_default():
    assert make_args().qmix_double_q is False and make_args(alg='qmix', qmix_double_q=True).qmix_double_q is True
    assert get_train_args(['dmfb']).qmix_double_q is False
    assert get_train_args(['dmfb', '--alg', 'qmix']).qmix_double_q is False
    args = get_train_args(['dmfb', '--alg', 'qmix', '--qmix_double_q'])
    assert args.qmix_double_q is True and args.double_q is False
    args = get_train_args(['dmfb', '--alg', 'qmix', '--qmix_double_q', '--qmix_lambda', '0.8', '--stream_state', '--qmix_packed'])
    assert args.qmix_double_q is True and args.qmix_lambda == 0.8 and args.qmix_packed and args.stream_state


def test_vdn_refuses_qmix_double_q_and_points_to_double_q(capsys):
    with pytest.raises(SystemExit):
        get_train_args(['dmfb', '--alg', 'vdn', '--qmix_double_q'])
    err = capsys.readouterr().err
    assert '--qmix_double_q' in err and '--double_q' in err


def test_double_q_with_qmix_still_refuses(capsys):
    from marl_dmfb_amd.policy.qmix import QMIX
    with pytest.raises(SystemExit):
        get_train_args(['dmfb', '--alg', 'qmix', '--double_q', '--qmix_double_q'])
    assert 'VDN-only' in capsys.readouterr().err
    args = make_args(alg='qmix', cuda=False, double_q=True, qmix_double_q=True, n_actions=5, n_agents=4, obs_shape=(3, 9, 9, 2, 245),
                     state_shape=300, episode_limit=40)
    with pytest.raises(ValueError, match=r'double_q.*VDN-only'):
        QMIX(args)


def _agents():
    g = QD.load_edited(SPEC)
    return g, f64_case_agents(Q.load_spec(SPEC), Q.spec_config(SPEC), PATH, 'cpu')


def test_double_q_set_after_construction_is_refused_at_learn_time():
    g, agents = _agents()
    assert agents.policy._double_q() is False
    agents.policy.args.qmix_double_q = True
    assert agents.policy._double_q() is True
    agents.policy.args.double_q = True
    with pytest.raises(ValueError, match=r'double_q.*VDN-only'):
        QD.learn_step(g, agents, 'cpu', 'cpu', 0)


@pytest.mark.parametrize('lens', [[7, 5, 5, 3, 3, 3, 1], [9], [4, 4, 4, 4], [6, 6, 2, 1, 1], [1, 1], [40, 39, 39, 2]],
                         ids=['ties', 'single', 'all_equal', 'ties_and_ones', 'length_one', 'long'])
def test_target_rows_of_a_draw_are_its_selector_units(lens):
    """The packed learn hands the kernel `target_row` as the selector list: unit (e, t) -> unit (e, t + 1) where the episode goes on,
    else the tail unit U + e."""
    from marl_dmfb_amd.policy.qmix import QMIX
    from marl_dmfb_amd.policy.vdn import VDN
    lens = np.asarray(lens)
    idx = np.arange(len(lens))[::-1] * 3 + 1          # any slots
    counts, units = VDN.pack_units(idx, lens, 48)
    rows, target_row = QMIX.pack_state_rows(idx, lens, counts, 48)
    sel, last = selector_units(counts)
    assert target_row.dtype == sel.dtype == np.int32 and np.array_equal(target_row, sel)
    U, B = len(units), len(lens)
    assert len(last) == B and sorted(sel[sel >= U]) == list(range(U, U + B))
    assert np.array_equal(sel[last], U + np.arange(B))       # the last unit of episode e selects with tail unit U + e


def test_header_functions_are_exported_and_bound_with_their_arity():
    """include/qmix_double.h against _lib.SIGNATURES and the library (which loads without a GPU); the argument guards run on the host
    before anything touches the GPU."""
    from marl_dmfb_amd import _lib
    from test_cabi_exports import _prototypes
    declared = _prototypes('qmix_double.h')
    table = _lib.SIGNATURES['qmix_double']
    assert sorted(declared) == sorted(table) == ['qmix_mix_td_double_forward', 'qmix_mix_td_double_forward_packed']
    assert _lib._FILE['qmix_double'] == 'qmix_ops'
    raw = _lib.qmix_double()
    lam = _lib.SIGNATURES['qmix_lambda']
    assert len(table['qmix_mix_td_double_forward']) == len(lam['qmix_mix_td_lambda_forward']) + 2
    assert len(table['qmix_mix_td_double_forward_packed']) == len(lam['qmix_mix_td_lambda_forward_packed']) + 4
    for name, n in declared.items():
        assert len(table[name]) == n and len(getattr(raw, name).argtypes) == n, name
    assert raw.qmix_mix_td_double_forward(*[None] * 7, 4, 3, 8, 2, 5, None, 4, 0, None, 4, 1, 24, 32, None, None, 0.99, None, None, None,
                                          0.8, None, None, None, None, None, None) == -1
    assert raw.qmix_mix_td_double_forward_packed(None, None, None, 4, *[None] * 5, 2, 5, None, None, None, 24, 32, None, None, 0.99, None,
                                                 None, None, 0.8, None, None, None, 0, None, None, 4, None, None, None) == -1


def _two_learns(flag):
    g, agents = _agents()
    pol = agents.policy
    if flag is None:
        del pol.args.qmix_double_q
        assert not hasattr(pol.args, 'qmix_double_q')
    else:
        pol.args.qmix_double_q = flag
    out = []
    for step in range(2):
        learn_f64.with_threads(QD.learn_step, g, agents, 'cpu', 'cpu', step)
        out.append([torch.as_tensor(float(pol.last_loss)), torch.as_tensor(float(pol.last_grad_norm))] +
                   [t.detach().clone() for net in (pol.eval_rnn, pol.eval_qmix_net) for p in net.parameters() for t in (p.grad, p)])
    return out


def test_flag_off_is_the_learn_without_the_attribute():
    without, off, on = _two_learns(None), _two_learns(False), _two_learns(True)
    differs = False
    for a, b, c in zip(without, off, on):
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and x.dtype == y.dtype
            differs = differs or not torch.equal(x, z)
    assert differs, 'qmix_double_q changed nothing: the comparison above says nothing'


@pytest.mark.parametrize('lam', [0.0, QD.LAMBDA])
def test_cpu_learn_with_double_q_matches_float64_in_every_element(lam):
    """Two learns of the tensor-op path (CPU tensors, padded episodes, `terminated` edited) with qmix_double_q set AFTER the set-up
    (the learner reads it at learn time), against the float64 restatement with the path's picks given: err <= factor x E_ref per
    tensor of eval_rnn and eval_qmix_net, the loss and the gradient norm; E_ref is the restatement's own float32 noise over five
    episode orders.  The picks are held to the float64 picks, and the restatement's own float32 picks are held first."""
    own = QD.envelope(SPEC, True, lam)
    g, agents = _agents()
    assert bool(g['padded'].any())
    bad = []
    print()
    for k, run in enumerate(own['runs32']):
        for step in range(2):
            bad += double_q_f64.pick_report('float32 restatement, order %d' % k, run[step]['picks'], own, step, g)
    assert not bad, '\n'.join(bad)
    plain = Q.qmix_reference_learn(SPEC, torch.float64)
    gap = abs(own['ref'][0]['loss'] - plain[0]['loss']) / abs(own['ref'][0]['loss'])
    print('float64 loss: double-Q, edited, lambda %g %.9g, the stored one-step learn %.9g, relative gap %.3e, E_ref %.3e' % (
        lam, own['ref'][0]['loss'], plain[0]['loss'], gap, own['E'][0]['loss']))
    assert gap > 100 * own['E'][0]['loss']           # the bound below can tell the two learns apart
    pol = agents.policy
    pol.args.qmix_double_q, pol.args.qmix_lambda = True, lam
    pol.double_picks = []
    results, picks = [], []
    for step in range(2):
        learn_f64.with_threads(QD.learn_step, g, agents, 'cpu', 'cpu', step)    # the thread count of the envelope's own runs
        results.append((float(pol.last_grad_norm), float(pol.last_loss),
                        [(k, p.grad.detach().clone(), p.detach().clone()) for k, p in pol.eval_rnn.named_parameters()] +
                        [(Q.MIX + k, p.grad.detach().clone(), p.detach().clone()) for k, p in pol.eval_qmix_net.named_parameters()]))
        p = pol.double_picks[step].numpy()
        assert p.shape == own['ref'][step]['picks'].shape and p.dtype == np.int8 and (p >= 0).all() and (p < pol.n_actions).all()
        picks.append(p)
    given = QD.envelope(SPEC, True, lam, picks)
    for step, (norm, loss, tensors) in enumerate(results):
        assert [k for k, _, _ in tensors] == list(given['ref'][step]['grad'])
        factors = QD.path_factors(SPEC, True, 'cpu', lam, step)
        assert all(f <= QD.MAX_TENSOR_FACTOR for f in factors.values())
        bad += learn_f64.compare_step('cpu qmix_double_q lam=%g %s@edited' % (lam, SPEC), step, given, norm, loss, tensors, factors)
        bad += double_q_f64.pick_report('cpu lam=%g' % lam, picks[step], own, step, g)
    assert not bad, '\n'.join(bad)
