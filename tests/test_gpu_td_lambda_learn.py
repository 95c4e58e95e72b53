"""Two learns on lambda-returns (args.td_lambda = 0.8) through the shipped GPU learn paths, every element of every gradient and weight
against the float64 restatement of tests/td_lambda_f64.py, by the method of tests/test_gpu_learn_f64.py: err <= factor x E_ref per
tensor and learn, E_ref the restatement's own float32 noise on the same batch (five episode orders), the factor 2 unless
`td_lambda_f64.FACTORS` names another power of two for that tensor, path and learn.  And td_lambda = 0.0 set explicitly is, bit for
bit, an `args` that has no such attribute."""
import os

import pytest
import torch

import learn_f64
import td_lambda_f64
from vdn_helpers import learn_golden_setup, learn_golden_step

pytestmark = pytest.mark.gpu

# path name -> (flags of learn_golden_step, value of MARL_DMFB_GRU_PAIR): the two of tests/test_gpu_learn_f64.py that differ in
# the TD block (padded and packed)
PATHS = {'fused_td': (dict(replay_dtypes=True), None),
         'packed': (dict(replay_dtypes=True, packed=True), '1')}
GOLDENS = ['vdn_learn_4d_od24_short.npz', 'vdn_learn_4d_od24_b64.npz']
CASES = [(name, path) for name in GOLDENS for path in PATHS]


def _pair_env(monkeypatch, pair):
    if pair is not None:
        monkeypatch.setenv('MARL_DMFB_GRU_PAIR', pair)
    else:
        monkeypatch.delenv('MARL_DMFB_GRU_PAIR', raising=False)


@pytest.mark.parametrize('name,path', CASES, ids=['%s-%s' % (n[:-4], p) for n, p in CASES])
def test_lambda_learn_matches_float64_in_every_element(name, path, monkeypatch):
    flags, pair = PATHS[path]
    _pair_env(monkeypatch, pair)
    lam = td_lambda_f64.LAMBDA
    golden = learn_f64.golden_path(name)
    env = td_lambda_f64.envelope(golden, lam)
    g, agents = learn_golden_setup(golden, 'cuda:0')
    agents.policy.args.td_lambda = lam          # after the set-up: the learner reads it at learn time
    bad = []
    print()
    for step in range(2):
        learn_golden_step(g, agents, 'cuda:0', step, **flags)
        policy = agents.policy
        tensors = [(k, p.grad, p) for k, p in policy.eval_rnn.named_parameters()]
        bad += learn_f64.compare_step('%s td_lambda=%g %s' % (path, lam, os.path.basename(golden)[:-4]), step, env,
                                      float(policy.last_grad_norm), float(policy.last_loss), tensors,
                                      td_lambda_f64.path_factors(name, path, step))
    policy.check_td_inputs()
    assert not bad, '\n'.join(bad)


def _two_learns(golden, flags, td_lambda):
    g, agents = learn_golden_setup(golden, 'cuda:0')
    if td_lambda is None:
        if hasattr(agents.policy.args, 'td_lambda'):
            del agents.policy.args.td_lambda
    else:
        agents.policy.args.td_lambda = td_lambda
    out = []
    for step in range(2):
        learn_golden_step(g, agents, 'cuda:0', step, **flags)
        policy = agents.policy
        out.append([policy.last_loss.clone(), policy.last_grad_norm.clone()] +
                   [t.detach().clone() for p in policy.eval_rnn.parameters() for t in (p.grad, p)])
    return out


@pytest.mark.parametrize('path', list(PATHS))
def test_td_lambda_zero_is_the_learn_without_the_attribute(path, monkeypatch):
    flags, pair = PATHS[path]
    _pair_env(monkeypatch, pair)
    golden = learn_f64.golden_path(GOLDENS[0])
    without, zero = _two_learns(golden, flags, None), _two_learns(golden, flags, 0.0)
    for a, b in zip(without, zero):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
