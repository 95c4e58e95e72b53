"""Two QMIX learns on lambda-returns (args.qmix_lambda = 0.8) through the shipped GPU learn paths, every element of every gradient and
weight of eval_rnn and eval_qmix_net, the loss and the gradient norm against the float64 restatement of tests/qmix_lambda_f64.py, by
the method of tests/test_gpu_qmix_learn_f64.py: err <= factor x E_ref per tensor and learn, E_ref the restatement's own float32
noise on the same batch (five episode orders), the factor learn_f64.FACTOR unless `qmix_lambda_f64.FACTORS` names another power of
two (at most MAX_TENSOR_FACTOR) for that tensor, path and learn.  The paths are those of qmix_helpers.F64_PATHS, each with its
precondition asserted, never skipped.  And qmix_lambda = 0.0 set explicitly is, bit for bit, an `args` that has no such attribute."""
import pytest
import torch

import learn_f64
import qmix_lambda_f64 as QL
import qmix_learn_f64 as Q
from qmix_helpers import F64_PATHS, f64_case_agents, f64_case_learn

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = [('qmix_learn_4d_od24', path) for path in ('fused_ring', 'fused_two_tensors', 'torch_ops', 'packed', 'packed_valu')] + \
        [('fov5_4d_od24', path) for path in ('fused_ring', 'packed')]


def _pair_env(monkeypatch, path):
    pair = F64_PATHS[path][2]
    if pair is not None:
        monkeypatch.setenv('MARL_DMFB_GRU_PAIR', pair)
    else:
        monkeypatch.delenv('MARL_DMFB_GRU_PAIR', raising=False)


@pytest.mark.parametrize('spec,path', CASES, ids=['%s-%s' % c for c in CASES])
def test_lambda_learn_matches_float64_in_every_element(spec, path, monkeypatch):
    _pair_env(monkeypatch, path)
    lam = QL.LAMBDA
    env = QL.envelope(spec, lam)
    g = Q.load_spec(spec)
    agents = f64_case_agents(g, Q.spec_config(spec), path, DEV)
    pol = agents.policy
    pol.args.qmix_lambda = lam          # after the set-up: the learner reads it at learn time
    bad = []
    print()
    for step in range(2):
        f64_case_learn(g, agents, path, DEV, step)
        tensors = [(k, p.grad, p) for k, p in pol.eval_rnn.named_parameters()] + \
                  [(Q.MIX + k, p.grad, p) for k, p in pol.eval_qmix_net.named_parameters()]
        assert [k for k, _, _ in tensors] == list(env['ref'][step]['grad'])
        factors = QL.path_factors(spec, path, step)
        assert all(f <= QL.MAX_TENSOR_FACTOR for f in factors.values())
        bad += learn_f64.compare_step('%s qmix_lambda=%g %s' % (path, lam, spec), step, env, float(pol.last_grad_norm),
                                      float(pol.last_loss), tensors, factors)
    pol.check_td_inputs()
    assert not bad, '\n'.join(bad)


def _two_learns(spec, path, qmix_lambda):
    g = Q.load_spec(spec)
    agents = f64_case_agents(g, Q.spec_config(spec), path, DEV)
    pol = agents.policy
    if qmix_lambda is None:
        del pol.args.qmix_lambda
        assert not hasattr(pol.args, 'qmix_lambda')
    else:
        pol.args.qmix_lambda = qmix_lambda
    out = []
    for step in range(2):
        f64_case_learn(g, agents, path, DEV, step)
        out.append([pol.last_loss.clone(), pol.last_grad_norm.clone()] +
                   [t.detach().clone() for net in (pol.eval_rnn, pol.eval_qmix_net) for p in net.parameters() for t in (p.grad, p)])
    pol.check_td_inputs()
    return out


@pytest.mark.parametrize('path', ['fused_ring', 'packed'])
def test_qmix_lambda_zero_is_the_learn_without_the_attribute(path, monkeypatch):
    _pair_env(monkeypatch, path)
    spec = CASES[0][0]
    without, zero = _two_learns(spec, path, None), _two_learns(spec, path, 0.0)
    for a, b in zip(without, zero):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
