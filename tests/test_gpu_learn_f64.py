"""Every element of a learn's gradients and weights against a float64 learn, through every learn path the project ships.

The learn goldens pin VDN.learn / VDN.learn_packed to the reference's float32 numbers at 512 sampled elements per tensor.  Here the
same two consecutive learns (driven by the same set-up as `vdn_helpers.learn_golden_check`) are compared in full with the float64
restatement of the reference's learn (tests/learn_f64.py; tied to the goldens by tests/test_learn_f64_reference.py): after each
learn the whole p.grad and the whole p of every eval parameter, `last_grad_norm` and the loss.

Bound: err = max|x - x64| / max|x64| <= FACTOR[tensor] x E_ref per tensor and step, E_ref being the reference's OWN float32
rounding noise on the same batch (largest error of five float32 runs of the restatement, episodes in five orders) -- never a
number taken from a path under test.  The factor is 2 (the noise was sampled five times only) unless `learn_f64.FACTORS` names
another power of two for that tensor on that golden, path and learn, on the evidence in profiles/learn_f64/NOTES.md; every line
of the table in that file is printed by these tests (run with -s)."""
import os

import pytest

import learn_f64
from vdn_helpers import learn_golden_setup, learn_golden_step

pytestmark = pytest.mark.gpu

# path name -> (flags of learn_golden_step, value of MARL_DMFB_GRU_PAIR)
PATHS = {'fused_td': (dict(replay_dtypes=True), None),
         'host_len_bound': (dict(replay_dtypes=True, host_len_bound=True), None),
         'packed': (dict(replay_dtypes=True, packed=True), '1'),          # pair recurrence on the matrix cores: the default
         'packed_valu': (dict(replay_dtypes=True, packed=True), '0')}     # the 8-row VALU recurrence kernels
CASES = [(name, path) for name in learn_f64.VDN_GOLDENS for path in PATHS] + \
        [(name, path) for name in learn_f64.FOV_GOLDENS for path in ('packed', 'fused_td')]


@pytest.mark.parametrize('name,path', CASES, ids=['%s-%s' % (n[:-4], p) for n, p in CASES])
def test_learn_matches_float64_in_every_element(name, path, monkeypatch):
    flags, pair = PATHS[path]
    if pair is not None:
        monkeypatch.setenv('MARL_DMFB_GRU_PAIR', pair)
    else:
        monkeypatch.delenv('MARL_DMFB_GRU_PAIR', raising=False)
    golden = learn_f64.golden_path(name)
    env = learn_f64.envelope(golden)
    g, agents = learn_golden_setup(golden, 'cuda:0')
    bad = []
    print()
    for step in range(2):
        learn_golden_step(g, agents, 'cuda:0', step, **flags)
        policy = agents.policy
        tensors = [(k, p.grad, p) for k, p in policy.eval_rnn.named_parameters()]
        bad += learn_f64.compare_step('%s %s' % (path, os.path.basename(golden)[:-4]), step, env, float(policy.last_grad_norm),
                                      float(policy.last_loss), tensors, learn_f64.path_factors(name, path, step))
    assert not bad, '\n'.join(bad)
