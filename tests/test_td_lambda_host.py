"""Host side of the lambda-return targets (args.td_lambda): the rule in numpy against the reference's own `td_lambda_target`
(tests/golden/td_lambda_ref.npz, tools/oracle/gen_td_lambda_golden.py), lambda 0 against the one-step target, the flag and its
refusals, and the tensor-op learn on CPU tensors against the float64 restatement of tests/td_lambda_f64.py.  No GPU needed."""
import os

import numpy as np
import pytest

import learn_f64
import td_lambda_f64
from marl_dmfb_amd.common.arguments import get_train_args, make_args
from marl_dmfb_amd.policy.td_lambda import check_lambda, lambda_targets_reference, lambda_targets_torch
from vdn_helpers import learn_golden_setup, learn_golden_step

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'td_lambda_ref.npz')
SHORT = 'vdn_learn_4d_od24_short.npz'


def test_float64_rule_matches_the_reference_function():
    """On episodes whose last valid step is terminated the rule is the reference's td_lambda_target.  Bound per valid slot:
    4 * T * 2^-24 * S_t with S_t = sum over k >= t of (|r_k| + gamma |Q'_k|) of that episode: the reference adds at most about 2T
    float32 terms, each partial sum below S_t.  About 3e-5 at this size; a wrong power of lambda or a lost bootstrap misses by 0.1."""
    g = np.load(GOLDEN)
    B, T = g['r'].shape[:2]
    assert (B, T) == (8, 9) and {1, 2, 9} <= set(g['lens'].tolist())
    gamma = float(g['gamma'])
    valid = g['padded'][:, :, 0] == 0
    last = g['lens'] - 1
    assert (g['terminated'][np.arange(B), last, 0] == 1).all() and (g['terminated'][:, :, 0][~valid] == 1).all()
    terms = np.abs(g['r'][:, :, 0].astype(np.float64)) + gamma * np.abs(g['q_targets'][:, :, 0].astype(np.float64))
    terms = terms * valid
    S = terms[:, ::-1].cumsum(axis=1)[:, ::-1]
    bound = 4 * T * 2.0 ** -24 * S
    for k, lam in enumerate(g['lambdas']):
        G = lambda_targets_reference(g['q_targets'], g['r'], g['terminated'], g['padded'], gamma, float(lam), np.float64)
        err = np.abs(G[:, :, 0] - g['target_%d' % k][:, :, 0].astype(np.float64))
        print('lambda %g: largest error %.3e, largest bound %.3e' % (lam, err[valid].max(), bound[valid].max()))
        assert (err[valid] <= bound[valid]).all(), (lam, err[valid].max())
        # the check can tell lambda from the one-step target
        one = lambda_targets_reference(g['q_targets'], g['r'], g['terminated'], g['padded'], gamma, 0.0, np.float64)
        assert np.abs(one[:, :, 0] - g['target_%d' % k][:, :, 0])[valid].max() > 0.1


def _random_batch(seed, B=7, T=9):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, T + 1, B)
    lens[0], lens[1] = T, 1
    steps = np.arange(T)[None, :]
    padded = (steps >= lens[:, None]).astype(np.uint8)
    terminated = (rng.random((B, T)) < 0.2).astype(np.uint8)
    q = (rng.standard_normal((B, T)) * 3).astype(np.float32)
    r = rng.standard_normal((B, T)).astype(np.float32)
    return q, r, terminated, padded


def test_lambda_zero_is_the_one_step_target_bit_for_bit():
    q, r, terminated, padded = _random_batch(3)
    gamma = np.float32(0.99)
    G = lambda_targets_reference(q, r, terminated, padded, 0.99, 0.0, np.float32)
    want = r + (gamma * q) * (np.float32(1) - terminated.astype(np.float32))
    assert G.dtype == np.float32 and np.array_equal(G.view(np.int32), want.view(np.int32))


def test_torch_walk_is_the_numpy_rule_bit_for_bit():
    import torch
    for seed, lam in ((5, 0.8), (6, 0.5), (7, 1.0)):
        q, r, terminated, padded = _random_batch(seed)
        want = lambda_targets_reference(q, r, terminated, padded, 0.99, lam, np.float32)
        col = [torch.as_tensor(x.astype(np.float32)).unsqueeze(2) for x in (q, r, terminated, padded)]
        got = lambda_targets_torch(*col, 0.99, lam).squeeze(2).numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), lam


def test_terminated_cuts_the_return_and_padding_does_not_leak():
    """A terminated step takes nothing from the steps behind it; a padded slot keeps the one-step target and gives nothing to the
    valid steps; an episode whose last valid step is not terminated bootstraps from Q' of that step."""
    q = np.array([[1.0, 2.0, 3.0, 4.0, 50.0]])
    r = np.array([[0.5, 0.25, 0.125, 1.0, 70.0]])
    terminated = np.array([[0, 1, 0, 0, 1]])
    padded = np.array([[0, 0, 0, 0, 1]])
    gamma, lam = 0.9, 0.5
    G = lambda_targets_reference(q, r, terminated, padded, gamma, lam, np.float64)[0]
    g3 = 1.0 + gamma * 4.0                                   # last valid step, not terminated: bootstraps
    g2 = 0.125 + gamma * (0.5 * 3.0 + 0.5 * g3)
    g1 = 0.25                                                # terminated in mid-episode
    g0 = 0.5 + gamma * (0.5 * 1.0 + 0.5 * g1)
    np.testing.assert_allclose(G, [g0, g1, g2, g3, 70.0], rtol=1e-15)


@pytest.mark.parametrize('bad', [-0.1, 1.5, float('nan'), 'x'])
def test_range_errors(bad, capsys):
    with pytest.raises(ValueError, match='td_lambda'):
        check_lambda(bad)
    with pytest.raises(ValueError):
        lambda_targets_reference(np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 2)), 0.99, bad)
    with pytest.raises(SystemExit):
        get_train_args(['dmfb', '--td_lambda', str(bad)])
    assert 'td_lambda' in capsys.readouterr().err


def test_flag_and_default(capsys):
    assert make_args().td_lambda == 0.0 and make_args(td_lambda=0.8).td_lambda == 0.8
    assert get_train_args(['dmfb']).td_lambda == 0.0
    assert get_train_args(['dmfb', '--td_lambda', '0.8']).td_lambda == 0.8
    assert get_train_args(['dmfb', '--alg', 'qmix', '--td_lambda', '0']).td_lambda == 0.0
    with pytest.raises(SystemExit):
        get_train_args(['dmfb', '--alg', 'qmix', '--td_lambda', '0.8'])
    assert 'VDN-only' in capsys.readouterr().err


def test_qmix_refuses_td_lambda():
    from marl_dmfb_amd.policy.qmix import QMIX
    args = make_args(alg='qmix', cuda=False, td_lambda=0.8, n_actions=5, n_agents=4, obs_shape=(3, 9, 9, 2, 245), state_shape=300,
                     episode_limit=40)
    with pytest.raises(ValueError, match=r'td_lambda.*VDN-only'):
        QMIX(args)


def test_learner_rejects_a_bad_lambda_at_learn_time():
    g, agents = learn_golden_setup(learn_f64.golden_path(SHORT), 'cpu')
    agents.policy.args.td_lambda = 1.5
    with pytest.raises(ValueError, match='td_lambda'):
        learn_golden_step(g, agents, 'cpu', 0)


def test_cpu_learn_on_lambda_returns_matches_float64_in_every_element():
    """Two learns of the tensor-op path (CPU tensors, padded episodes) at td_lambda 0.8, set AFTER the set-up (the learner reads it
    at learn time), against the float64 restatement: err <= factor x E_ref per tensor, E_ref the restatement's own float32 noise."""
    path = learn_f64.golden_path(SHORT)
    lam = td_lambda_f64.LAMBDA
    env = td_lambda_f64.envelope(path, lam)
    one_step = learn_f64.reference_learn(path, __import__('torch').float64)
    gap = abs(env['ref'][0]['loss'] - one_step[0]['loss']) / abs(env['ref'][0]['loss'])
    print('\nfloat64 loss: lambda %g %.9g, one-step %.9g, relative gap %.3e, E_ref %.3e' % (
        lam, env['ref'][0]['loss'], one_step[0]['loss'], gap, env['E'][0]['loss']))
    assert gap > 100 * env['E'][0]['loss']           # the bound below can tell the two learns apart
    g, agents = learn_golden_setup(path, 'cpu')
    assert bool(np.asarray(g['padded']).any())
    agents.policy.args.td_lambda = lam
    bad = []
    for step in range(2):
        learn_f64.with_threads(learn_golden_step, g, agents, 'cpu', step)    # the thread count of the envelope's own runs
        policy = agents.policy
        tensors = [(k, p.grad, p) for k, p in policy.eval_rnn.named_parameters()]
        bad += learn_f64.compare_step('cpu td_lambda=%g %s' % (lam, SHORT[:-4]), step, env, float(policy.last_grad_norm),
                                      float(policy.last_loss), tensors, td_lambda_f64.path_factors(SHORT, 'cpu', step))
    assert not bad, '\n'.join(bad)
