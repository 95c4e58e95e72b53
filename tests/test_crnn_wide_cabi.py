"""CPU-side checks of the fov 11 / 13 front-end ABI (include/crnn_wide.h): the cross-compiled library exports every declared
symbol, the binding table matches the prototypes, sizes and block rows are reported, unsupported shapes are refused before anything
is launched, CRNN._hip_front() maps the reference's six conv stacks (network/base_net.py:23-33) to the kernels that implement them,
and the two learn goldens hold on the torch path."""
import os
import re
import types

import pytest

from marl_dmfb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {(11, 24): (1176, 1216), (11, 32): (1568, 1600), (13, 24): (1944, 1984), (13, 32): (2592, 2624)}   # features, padded_cols


def _prototypes():
    txt = open(os.path.join(ROOT, 'include', 'crnn_wide.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    txt = re.sub(r'^\s*#.*$', '', txt, flags=re.M)
    out = {}
    for name, params in re.findall(r'\b([a-z][a-z_0-9]*)\s*\(([^()]*)\)\s*;', txt):
        params = params.strip()
        out[name] = 0 if params in ('', 'void') else params.count(',') + 1
    return out


def test_crnn_wide_library_exports_every_declared_symbol():
    declared = _prototypes()
    assert sorted(declared) == ['crnn_wide_backward', 'crnn_wide_backward_block_rows', 'crnn_wide_backward_parts',
                                'crnn_wide_forward_block_rows', 'crnn_wide_front_forward', 'crnn_wide_last_hip_error',
                                'crnn_wide_padded_cols']
    table = _lib.SIGNATURES['crnn_wide']
    assert sorted(table) == sorted(declared)
    lib = _lib.crnn_wide()
    for name, n in declared.items():
        sig = table[name]
        assert len(sig[0] if isinstance(sig, tuple) else sig) == n, name
        assert len(getattr(lib, name).argtypes) == n, name
    # argument lists as the crnn_fov_* counterparts
    for name in ('front_forward', 'padded_cols', 'backward_parts', 'backward', 'last_hip_error'):
        assert table['crnn_wide_' + name] == _lib.SIGNATURES['crnn_fov']['crnn_fov_' + name], name


def test_last_error_prefix_is_matched_before_the_crnn_ops_one():
    order = list(_lib._LAST_ERROR)
    assert order.index('crnn_wide_') < order.index('crnn_')
    first = next(p for p in _lib._LAST_ERROR if 'crnn_wide_backward'.startswith(p))
    assert _lib._LAST_ERROR[first] == 'crnn_wide_last_hip_error'


@pytest.mark.parametrize('fov,od', sorted(SIZES))
def test_supported_shapes_report_their_sizes(fov, od):
    lib = _lib.crnn_wide()
    feat, pad = SIZES[(fov, od)]
    assert feat == od * (fov - 4) ** 2 and pad == (feat + 10 + 63) // 64 * 64
    assert lib.crnn_wide_padded_cols(fov, od) == pad
    assert lib.crnn_wide_backward_parts(fov, od) == od * od * 9 + od + od * 27 + od
    rb, rbb = lib.crnn_wide_forward_block_rows(fov, od), lib.crnn_wide_backward_block_rows(fov, od)
    assert rb > 0 and rbb > 0
    assert 256 * rb + rb + 1 <= 4113      # the largest forward case of tests/test_gpu_crnn_wide.py
    # argument guards run on the host: NULL pointers are a bad argument, not a launch
    assert lib.crnn_wide_front_forward(fov, None, 3 * fov * fov + 2, None, 5, 4, None, None, None, None, None, None, od, None,
                                       pad, 0, None) == -1
    assert lib.crnn_wide_backward(fov, None, 3 * fov * fov + 2, 4, None, pad, None, pad, None, None, None, od, None, 1, None, None) == -1


@pytest.mark.parametrize('fov,od', [(5, 24), (7, 32), (9, 24), (19, 32), (12, 24), (11, 16), (13, 16)])
def test_unsupported_shapes_are_refused_without_a_launch(fov, od):
    lib = _lib.crnn_wide()
    assert lib.crnn_wide_padded_cols(fov, od) == -6
    assert lib.crnn_wide_backward_parts(fov, od) == -6
    assert lib.crnn_wide_forward_block_rows(fov, od) == -6
    assert lib.crnn_wide_backward_block_rows(fov, od) == -6
    assert lib.crnn_wide_front_forward(fov, None, 600, None, 5, 4, None, None, None, None, None, None, od, None, 3000, 0, None) == -6
    assert lib.crnn_wide_backward(fov, None, 600, 4, None, 3000, None, 3000, None, None, None, od, None, 1, None, None) == -6


def _net(fov, od=24):
    from marl_dmfb_amd.network.base_net import CRNN
    a = types.SimpleNamespace(obs_shape=(3, fov, fov, 2, 3 * fov * fov + 2), hyper_hidden_dim=od, rnn_hidden_dim=128, n_actions=5, fov=fov)
    return CRNN(a)


@pytest.mark.parametrize('fov', [5, 7, 9, 11, 13, 19])
def test_hip_front_maps_the_conv_stacks(fov):
    net = _net(fov)
    assert net._hip_front() == fov
    assert net._hip_geometry() == (None if fov in (11, 13) else fov)
    if fov in (11, 13):
        assert (net.out, net.padded_cols()) == SIZES[(fov, 24)]
        net.convs[1] = net.convs[0]     # not two distinct convs: no kernel
        assert net._hip_front() is None


@pytest.mark.parametrize('name', ['fovlearn_4d_od24_fov11.npz', 'fovlearn_3d_od32_fov13.npz'])
def test_wide_learn_goldens_hold_on_the_cpu_path(name):
    """The reference's VDN.learn at fov 11 / 13 (tools/oracle/gen_fov_wide_golden.py, seed 13) reproduced by the torch path: the
    golden itself is not at a rounding knife edge (tests/test_gpu_wide_fov_loop.py checks the HIP path against it).  The episodes
    end at different lengths and some carry padded steps."""
    import numpy as np
    from vdn_helpers import learn_golden_check
    path = os.path.join(ROOT, 'tests', 'golden', name)
    assert os.path.getsize(path) <= 350 * 1024
    pad = np.load(path)['padded'][:, :, 0]
    lens = (1 - pad.astype(int)).sum(1)
    assert len(set(lens.tolist())) >= 3 and (lens < pad.shape[1]).any()
    learn_golden_check(path, 'cpu', rtol=1e-5, atol=1e-5)
