"""Every element of a QMIX learn's gradients and weights against a float64 learn, through every QMIX learn path the project ships.

The QMIX goldens pin QMIX.learn / QMIX.learn_packed to the reference's float32 numbers at sampled elements, on two DMFB batches
with fov 9.  Here two consecutive learns from the deterministic weights are compared in full with the float64 restatement of the
reference's QMIX learn (tests/qmix_learn_f64.py; tied to the goldens by tests/test_qmix_learn_f64_reference.py): after each learn
the whole p.grad and the whole p of every parameter of eval_rnn AND of eval_qmix_net, `last_grad_norm` and `last_loss`.  Beside
the two reference goldens there are a MEDA batch (9 actions, fov 19, S = 1800), a fov-5 and a fov-13 batch with 3 droplets, whose
int8 states are synthetic and carry negative entries.

Paths (qmix_helpers.F64_PATHS), each with its precondition asserted, never skipped: the fused mixing / TD block on the ring's two
views of one state tensor and on two separate tensors, the torch-op QMixNet path (args.fused_mix False), and learn_packed on the
matrix-core pair recurrence and on the VALU recurrence kernels, on a draw with padded steps.

Bound: err = max|x - x64| / max|x64| <= factor x E_ref per tensor and learn, E_ref being the reference's OWN float32 rounding
noise on the same batch (five float32 runs of the restatement, episodes in five orders) -- never a number taken from a path under
test.  The factor is learn_f64.FACTOR (2) unless `qmix_learn_f64.QMIX_FACTORS` names another power of two, at most 16 for a tensor,
on the evidence in profiles/learn_f64/NOTES.md; every line of the table in that file is printed by these tests (run with -s)."""
import pytest

import learn_f64
import qmix_learn_f64 as Q
from qmix_helpers import F64_CASES, F64_PATHS, f64_case_agents, f64_case_learn

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = F64_CASES
assert len(CASES) == len(set(CASES)) == 17 and {spec for spec, _ in CASES} == set(Q.SPECS)


@pytest.mark.parametrize('spec,path', CASES, ids=['%s-%s' % c for c in CASES])
def test_qmix_learn_matches_float64_in_every_element(spec, path, monkeypatch):
    pair = F64_PATHS[path][2]
    if pair is not None:
        monkeypatch.setenv('MARL_DMFB_GRU_PAIR', pair)
    else:
        monkeypatch.delenv('MARL_DMFB_GRU_PAIR', raising=False)
    env = Q.qmix_envelope(spec)
    g = Q.load_spec(spec)
    agents = f64_case_agents(g, Q.spec_config(spec), path, DEV)
    pol = agents.policy
    bad = []
    print()
    for step in range(2):
        f64_case_learn(g, agents, path, DEV, step)
        tensors = [(k, p.grad, p) for k, p in pol.eval_rnn.named_parameters()] + \
                  [(Q.MIX + k, p.grad, p) for k, p in pol.eval_qmix_net.named_parameters()]
        assert [k for k, _, _ in tensors] == list(env['ref'][step]['grad'])
        bad += learn_f64.compare_step('%s %s' % (path, spec), step, env, float(pol.last_grad_norm), float(pol.last_loss), tensors,
                                      Q.qmix_path_factors(spec, path, step))
    pol.check_td_inputs()
    assert not bad, '\n'.join(bad)
