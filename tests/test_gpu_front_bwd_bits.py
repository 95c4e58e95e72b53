"""The order of the additions of the two backward-side sums of the fov-9 front end (marl_dmfb_amd/csrc/crnn_ops.hip), which the
float64 and exact-integer tests cannot see: crnn_mlp_backward (k_mlp_bwd) and the partial-vector sum behind crnn_conv9_backward
(k_conv9_bwd_reduce) must give, bit for bit, what the library gave BEFORE their loads were reordered.  The weights of a learn follow
these sums, and a last-bit difference there grows once a rollout action flips.

tests/golden/front_bwd_bits.npz holds only the recorded outputs (tools/record_front_bwd_fixture.py, run on an MI355X with the
library of the commit before the change); the inputs are regenerated here, on the host, from the seeds below.

  mlp1     rows 300 (two workgroups, a partial wave) and 65 536 + 300 (256 partial vectors, some threads own two rows); the ten
           columns at column 600 of a 640-float row (16-byte aligned, the packed learn's layout) and of a 613-float row (rows that
           start on any 4-byte boundary).
  reduce   the four gradient tensors of crnn_conv9_backward at od 24 and od 32, 330 rows (33 row blocks at od 24), n_part 256 and 7."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

DEV = 'cuda'
A, DIR_OFF, COL0 = 5, 243, 600
MLP_CASES = [(rows, stride) for rows in (300, 65536 + 300) for stride in (640, 613)]
RED_CASES = [(od, n_part) for od in (24, 32) for n_part in (256, 7)]
RED_ROWS = 330
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'front_bwd_bits.npz')


def _ops():
    from marl_dmfb_amd import _lib
    return _lib.crnn_ops()


def _p(t):
    return C.c_void_p(t.data_ptr())


def mlp_key(rows, stride):
    return 'mlp_rows%d_stride%d' % (rows, stride)


def red_key(od, n_part):
    return 'reduce_od%d_parts%d' % (od, n_part)


def mlp_inputs(rows):
    """Host inputs of one mlp1 case: direction bytes in -2..2, a one-hot on most rows, the ten output columns (relu of a normal
    variate: about half are zero) and their gradient."""
    g = np.random.default_rng(910000 + rows)
    d = g.integers(-2, 3, (rows, 2)).astype(np.int8)
    onehot = np.zeros((rows, A), dtype=np.int8)
    has = g.random(rows) < 0.9
    onehot[np.arange(rows)[has], g.integers(0, A, rows)[has]] = 1
    x = np.maximum(g.standard_normal((rows, 10), dtype=np.float32), 0)
    grad = g.standard_normal((rows, 10), dtype=np.float32)
    return d, onehot, x, grad


def run_mlp(rows, stride):
    """-> float32 [10 * (2 + A) + 10]: dW then db.  Everything beside the ten columns is NaN, the pixels are 127."""
    d, onehot, x, grad = mlp_inputs(rows)
    obs = torch.full((rows, DIR_OFF + 2), 127, dtype=torch.int8, device=DEV)
    obs[:, DIR_OFF:] = torch.from_numpy(d).to(DEV)
    xs = torch.full((rows, stride), float('nan'), device=DEV)
    gs = torch.full((rows, stride), float('nan'), device=DEV)
    xs[:, COL0:COL0 + 10] = torch.from_numpy(x).to(DEV)
    gs[:, COL0:COL0 + 10] = torch.from_numpy(grad).to(DEV)
    oh = torch.from_numpy(onehot).to(DEV)
    lib = _ops()
    part = torch.full((lib.crnn_mlp_backward_parts(),), float('nan'), device=DEV)
    out = torch.full((10 * (2 + A) + 10,), float('nan'), device=DEV)
    rc = lib.crnn_mlp_backward(_p(obs), obs.stride(0), DIR_OFF, _p(oh), A, rows, _p(xs), stride, _p(gs), stride, COL0, _p(part), _p(out),
                               C.c_void_p(out.data_ptr() + 4 * 10 * (2 + A)), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


def conv_inputs(od):
    g = np.random.default_rng(920000 + od)
    obs = g.integers(0, 5, (RED_ROWS, 243)).astype(np.int8)
    w1 = (g.standard_normal((od, 27), dtype=np.float32) * np.float32(0.2))
    b1 = (g.standard_normal((od,), dtype=np.float32) * np.float32(0.1))
    w2 = (g.standard_normal((od, od * 9), dtype=np.float32) * np.float32(0.07))
    a2 = np.maximum(g.standard_normal((RED_ROWS, od * 25), dtype=np.float32), 0)   # the forward's output: its sign gates the gradient
    grad = g.standard_normal((RED_ROWS, od * 25), dtype=np.float32)
    return obs, w1, b1, w2, a2, grad


def run_reduce(od, n_part):
    """-> float32 [od * od * 9 + od + od * 27 + od]: dW2 | db2 | dW1 | db1 of crnn_conv9_backward."""
    obs, w1, b1, w2, a2, grad = (torch.from_numpy(v).to(DEV) for v in conv_inputs(od))
    lib = _ops()
    part = torch.full((n_part * lib.crnn_conv9_backward_parts(od),), float('nan'), device=DEV)
    grads = torch.full((od * od * 9 + od + od * 27 + od,), float('nan'), device=DEV)
    rc = lib.crnn_conv9_backward(_p(obs), obs.stride(0), RED_ROWS, _p(a2), a2.stride(0), _p(grad), grad.stride(0), _p(w1), _p(b1), _p(w2), od,
                                 _p(part), n_part, _p(grads), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return grads.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _same_bits(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(want).all() and float(np.abs(want).max()) > 0, 'the record of %s is empty' % what
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    print('%s: %d of %d elements with other bits' % (what, len(bad), got.size))
    if len(bad):
        i = int(bad[0][0])
        raise AssertionError('%s: %d of %d elements differ from the record, first at %d: got %r (0x%08x), recorded %r (0x%08x)'
                             % (what, len(bad), got.size, i, got[i], got.view(np.uint32)[i], want[i], want.view(np.uint32)[i]))


def test_the_record_holds_every_case():
    g = _golden()
    assert sorted(g) == sorted([mlp_key(*c) for c in MLP_CASES] + [red_key(*c) for c in RED_CASES])
    for rows, stride in MLP_CASES:
        assert g[mlp_key(rows, stride)].shape == (10 * (2 + A) + 10,)
    for od, n_part in RED_CASES:
        assert g[red_key(od, n_part)].shape == (od * od * 9 + od + od * 27 + od,)
    # the two layouts of an mlp1 case feed the same numbers to the same sums
    for rows in (300, 65536 + 300):
        assert np.array_equal(g[mlp_key(rows, 640)].view(np.uint32), g[mlp_key(rows, 613)].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize('rows,stride', MLP_CASES)
def test_mlp_backward_bits_of_the_build_before(rows, stride):
    _same_bits(run_mlp(rows, stride), _golden()[mlp_key(rows, stride)], 'mlp1 backward rows %d stride %d' % (rows, stride))


@pytest.mark.gpu
@pytest.mark.parametrize('od,n_part', RED_CASES)
def test_conv9_backward_sum_bits_of_the_build_before(od, n_part):
    _same_bits(run_reduce(od, n_part), _golden()[red_key(od, n_part)], 'conv9 backward od %d n_part %d' % (od, n_part))
