"""QMIX.learn parity: two consecutive learns on a fixed minibatch (tests/golden/qmix_learn_*.npz, the reference's QMIX with the
CRNN agent network, tools/oracle/gen_qmix_golden.py) -- loss, gradient norms, sampled CRNN gradients / weights and the full mixer
gradients / weights at the VDN goldens' tolerance (1e-5), on the CPU (torch-op mixer) and on the GPU through the fused
mixing / TD block (include/qmix_ops.h)."""
import glob
import os

import pytest

from qmix_helpers import qmix_learn_golden_check

FILES = sorted(glob.glob(os.path.join(os.path.dirname(__file__), 'golden', 'qmix_learn_*.npz')))


def test_goldens_exist():
    assert len(FILES) == 2


@pytest.mark.parametrize('ring_layout', [True, False], ids=['ring_views', 'two_tensors'])
@pytest.mark.parametrize('path', FILES, ids=os.path.basename)
def test_qmix_learn_matches_reference_cpu(path, ring_layout):
    qmix_learn_golden_check(path, 'cpu', fused=False, ring_layout=ring_layout)


@pytest.mark.gpu
@pytest.mark.parametrize('ring_layout', [True, False], ids=['ring_views', 'two_tensors'])
@pytest.mark.parametrize('path', FILES, ids=os.path.basename)
def test_qmix_learn_matches_reference_gpu_fused(path, ring_layout):
    qmix_learn_golden_check(path, 'cuda:0', fused=True, ring_layout=ring_layout)


@pytest.mark.gpu
@pytest.mark.parametrize('path', FILES, ids=os.path.basename)
def test_qmix_learn_matches_reference_gpu_torch_ops(path, monkeypatch):
    from marl_dmfb_amd.policy.qmix import QMIX
    monkeypatch.setattr(QMIX, '_mix_fused_ok', lambda self, batch: False)
    qmix_learn_golden_check(path, 'cuda:0')
