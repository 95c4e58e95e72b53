"""Every rocBLAS / hipBLASLt solution the shipped TunableOp file pins (marl_dmfb_amd/tuning/gemm_gfx950.csv) against a float64
product, in ONE child process (tests/gemm_solution_worker.py: exact pass with integer operands, precision pass with the fp32
element-wise and aggregate bounds, CPU spot check, every call served from the file), and `_LinearSplitK` forward and backward at
two shipped shapes through those solutions against float64 autograd.  A child that does not finish normally fails both tests
with the tail of its stderr; nothing is run again."""
import pytest

import gemm_solution_worker as W

pytestmark = pytest.mark.gpu

GRAD_TOL = 5e-6   # relative L2 per tensor against float64 autograd (tests/test_gpu_crnn_ops.py)


@pytest.fixture(scope='module')
def report():
    return W.run(W.SHIPPED, timeout=600, with_callsite=True)


def _finished(rep):
    if rep['failed']:
        pytest.fail('GEMM solution worker: %s' % rep['failed'], pytrace=False)
    if rep['mode'] != W.TUNED:
        pytest.skip('GEMM solutions: %s -- the shipped solutions do not run on this build' % rep['mode'])


def test_every_shipped_solution_matches_float64(report, capsys):
    _finished(report)
    with capsys.disabled():
        print('\n' + '\n'.join(W.summary(report)))
    expected = W.read_entries(W.SHIPPED)
    assert len(expected) == 381
    assert len(report['entries']) == len(expected)
    probs = W.verdict(report, expected)
    assert not probs, '\n'.join(probs)


def test_linear_splitk_at_shipped_shapes(report):
    _finished(report)
    shipped = {(e.op, e.key) for e in W.read_entries(W.SHIPPED)}
    untuned = {tuple(k) for k in report['untuned']}
    assert set(report['callsite']) == set(W.CALLSITE)
    for name, c in report['callsite'].items():
        for tname, rel in c['rel_l2'].items():
            assert rel <= GRAD_TOL, (name, tname, rel)
        keys = {tuple(k) for k in c['keys']}
        assert keys <= shipped, (name, keys - shipped)
        assert not keys & untuned, (name, keys & untuned)     # served from the file, not the library default
    # nothing else the call sites issued fell back to the default either (only the deliberate control calls did)
    assert untuned <= {tuple(k) for k in report['controls']}, untuned
