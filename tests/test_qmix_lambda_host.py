"""Host side of the lambda-return targets of the QMIX learn (args.qmix_lambda): the flag, its default and its refusals, td_lambda
still refused under QMIX, the learn-time check, qmix_lambda = 0 against a learner without the attribute, and the tensor-op learn on
CPU tensors against the float64 restatement of tests/qmix_lambda_f64.py.  No GPU needed."""
import pytest
import torch

import learn_f64
import qmix_lambda_f64 as QL
import qmix_learn_f64 as Q
from marl_dmfb_amd.common.arguments import get_train_args, make_args
from qmix_helpers import f64_case_agents, f64_case_learn

SPEC = 'qmix_learn_4d_od24'
PATH = 'torch_ops'           # qmix_helpers.F64_PATHS: on CPU tensors every learn is the tensor-op learn


def test_flag_and_default():
    assert make_args().qmix_lambda == 0.0 and make_args(alg='qmix', qmix_lambda=0.8).qmix_lambda == 0.8
    assert get_train_args(['dmfb']).qmix_lambda == 0.0
    assert get_train_args(['dmfb', '--alg', 'qmix']).qmix_lambda == 0.0
    assert get_train_args(['dmfb', '--alg', 'qmix', '--qmix_lambda', '0.8']).qmix_lambda == 0.8
    assert get_train_args(['dmfb', '--alg', 'qmix', '--qmix_lambda', '1']).qmix_lambda == 1.0
    assert get_train_args(['dmfb', '--alg', 'vdn', '--qmix_lambda', '0']).qmix_lambda == 0.0
    assert get_train_args(['dmfb', '--alg', 'qmix', '--qmix_lambda', '0.6']).td_lambda == 0.0


def test_vdn_refuses_qmix_lambda_and_points_to_td_lambda(capsys):
    with pytest.raises(SystemExit):
        get_train_args(['dmfb', '--alg', 'vdn', '--qmix_lambda', '0.8'])
    err = capsys.readouterr().err
    assert '--qmix_lambda' in err and '--td_lambda' in err


@pytest.mark.parametrize('bad', ['-0.1', '1.5', 'nan', 'x'])
def test_range_errors_at_parse_time(bad, capsys):
    with pytest.raises(SystemExit):
        get_train_args(['dmfb', '--alg', 'qmix', '--qmix_lambda', bad])
    assert 'qmix_lambda' in capsys.readouterr().err


def test_td_lambda_with_qmix_still_refuses(capsys):
    from marl_dmfb_amd.policy.qmix import QMIX
    with pytest.raises(SystemExit):
        get_train_args(['dmfb', '--alg', 'qmix', '--td_lambda', '0.8', '--qmix_lambda', '0.8'])
    assert 'VDN-only' in capsys.readouterr().err
    args = make_args(alg='qmix', cuda=False, td_lambda=0.8, qmix_lambda=0.8, n_actions=5, n_agents=4, obs_shape=(3, 9, 9, 2, 245),
                     state_shape=300, episode_limit=40)
    with pytest.raises(ValueError, match=r'td_lambda.*VDN-only'):
        QMIX(args)


def test_header_functions_are_exported_and_bound_with_their_arity():
    """include/qmix_lambda.h against _lib.SIGNATURES and the library (which loads without a GPU); the argument guards run on the
    host before anything touches the GPU."""
    from marl_dmfb_amd import _lib
    from test_cabi_exports import _prototypes
    declared = _prototypes('qmix_lambda.h')
    table = _lib.SIGNATURES['qmix_lambda']
    assert sorted(declared) == sorted(table) == ['qmix_mix_td_lambda_forward', 'qmix_mix_td_lambda_forward_packed']
    assert _lib._FILE['qmix_lambda'] == 'qmix_ops'
    raw = _lib.qmix_lambda()
    for name, n in declared.items():
        assert len(table[name]) == n and len(getattr(raw, name).argtypes) == n, name
    assert raw.qmix_mix_td_lambda_forward(*[None] * 7, 4, 3, 8, 2, 5, None, 4, 0, None, 4, 1, 24, 32, None, None, 0.99, None, None, None,
                                          0.8, None, None, None, None) == -1
    assert raw.qmix_mix_td_lambda_forward_packed(None, None, None, 4, *[None] * 5, 2, 5, None, None, None, 24, 32, None, None, 0.99, None,
                                                 None, None, 0.8, None, None, None, 0, None, None) == -1


def _agents():
    g = Q.load_spec(SPEC)
    return g, f64_case_agents(g, Q.spec_config(SPEC), PATH, 'cpu')


@pytest.mark.parametrize('bad', [1.5, -0.1, float('nan'), 'x'])
def test_learner_rejects_a_bad_lambda_at_learn_time(bad):
    g, agents = _agents()
    agents.policy.args.qmix_lambda = bad
    with pytest.raises(ValueError, match='qmix_lambda'):
        f64_case_learn(g, agents, PATH, 'cpu', 0)


def _two_learns(qmix_lambda):
    g, agents = _agents()
    pol = agents.policy
    if qmix_lambda is None:
        del pol.args.qmix_lambda
        assert not hasattr(pol.args, 'qmix_lambda')
    else:
        pol.args.qmix_lambda = qmix_lambda
    out = []
    for step in range(2):
        learn_f64.with_threads(f64_case_learn, g, agents, PATH, 'cpu', step)
        out.append([torch.as_tensor(float(pol.last_loss)), torch.as_tensor(float(pol.last_grad_norm))] +
                   [t.detach().clone() for net in (pol.eval_rnn, pol.eval_qmix_net) for p in net.parameters() for t in (p.grad, p)])
    return out


def test_qmix_lambda_zero_is_the_learn_without_the_attribute():
    without, zero, lam = _two_learns(None), _two_learns(0.0), _two_learns(QL.LAMBDA)
    differs = False
    for a, b, c in zip(without, zero, lam):
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and x.dtype == y.dtype
            differs = differs or not torch.equal(x, z)
    assert differs, 'qmix_lambda = 0.8 changed nothing: the comparison above says nothing'


def test_cpu_learn_on_lambda_returns_matches_float64_in_every_element():
    """Two learns of the tensor-op path (CPU tensors, padded episodes) at qmix_lambda 0.8, set AFTER the set-up (the learner reads it
    at learn time), against the float64 restatement: err <= factor x E_ref per tensor of eval_rnn and eval_qmix_net, the loss and the
    gradient norm; E_ref is the restatement's own float32 noise over five episode orders."""
    lam = QL.LAMBDA
    env = QL.envelope(SPEC, lam)
    one_step = Q.qmix_reference_learn(SPEC, torch.float64)
    gap = abs(env['ref'][0]['loss'] - one_step[0]['loss']) / abs(env['ref'][0]['loss'])
    print('\nfloat64 loss: lambda %g %.9g, one-step %.9g, relative gap %.3e, E_ref %.3e' % (
        lam, env['ref'][0]['loss'], one_step[0]['loss'], gap, env['E'][0]['loss']))
    assert gap > 100 * env['E'][0]['loss']           # the bound below can tell the two learns apart
    g, agents = _agents()
    assert bool(g['padded'].any())
    pol = agents.policy
    pol.args.qmix_lambda = lam
    bad = []
    for step in range(2):
        learn_f64.with_threads(f64_case_learn, g, agents, PATH, 'cpu', step)    # the thread count of the envelope's own runs
        tensors = [(k, p.grad, p) for k, p in pol.eval_rnn.named_parameters()] + \
                  [(Q.MIX + k, p.grad, p) for k, p in pol.eval_qmix_net.named_parameters()]
        assert [k for k, _, _ in tensors] == list(env['ref'][step]['grad'])
        factors = QL.path_factors(SPEC, 'cpu', step)
        assert all(f <= QL.MAX_TENSOR_FACTOR for f in factors.values())
        bad += learn_f64.compare_step('cpu qmix_lambda=%g %s' % (lam, SPEC), step, env, float(pol.last_grad_norm), float(pol.last_loss),
                                      tensors, factors)
    assert not bad, '\n'.join(bad)
