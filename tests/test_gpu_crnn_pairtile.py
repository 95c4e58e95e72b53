"""conv2 of the fov-9 front end at od 24 (marl_dmfb_amd/csrc/crnn_mfma.h): the channels 16..23 run on PAIR tiles -- 8 channels x 2
adjacent output positions over the union of their 3x3 windows -- and the tiles are dealt out to the waves by a table.  What can go
wrong there is a tap shifted by one, a neighbour's tap leaking into a position, a position left out or written twice, a channel in
the wrong column.  Through the C ABI (include/crnn_ops.h), all three entry points:

  exact     int8 pixels in 0..4 and small integer weights: every partial sum is an integer far below 2^24, so float32 is exact in
            any order; the expected values come from an int64 numpy convolution and are compared with ==.  Nine networks whose
            conv2 has exactly ONE weight per output channel -- tap (t + channel) % 9 of one input channel in network t, so every tap
            of every channel at every one of the 25 positions is singled out once -- and one dense network.  1, 15, 16, 17 and 33
            rows (row block: 16), a strided observation, the live-row list with gaps, the zero tail, the rows behind the last.
  bits      one real-valued network on 33 rows against tests/golden/crnn_front9_od24_rows33.npz, the output of the build BEFORE
            the pair tiles (tools/record_conv_fixture.py): the same bits, except that a zero may change its sign.
  float64   the same case against torch's float64 convolution (relative L2 <= GRAD_TOL of tests/test_gpu_crnn_ops.py), and an
            od-32 network, which has no pair tiles, against its own."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import front_kernel_cases as K

gpu = pytest.mark.gpu

DEV = 'cuda'
SENT = -777.25
OD, A, PAD, NF = 24, 5, 640, 610
ROW_COUNTS = (1, 15, 16, 17, 33)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'crnn_front9_od24_rows33.npz')


def _ops():
    from marl_dmfb_amd import _lib
    return _lib.crnn_ops()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------------------------------------
# integer networks and their int64 reference
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _net(t):
    """Network t: 0..8 = one conv2 weight per output channel c2, at tap (t + c2) % 9 of input channel (5 c2 + 7 t) % 24; 9 = dense
    conv2 weights in {-1, 0, 1}.  conv1 in {-1, 0, 1, 2} with biases 0..3 (activations mostly positive and all different), conv2
    biases in {-1, 0, 1}, mlp1 in {-1, 0, 1}.  int64 numpy arrays."""
    g = np.random.default_rng(100 + t)
    n = dict(w1=g.integers(-1, 3, (OD, 3, 3, 3)), b1=g.integers(0, 4, (OD,)), b2=g.integers(-1, 2, (OD,)),
             mlp_w=g.integers(-1, 2, (10, 2 + A)), mlp_b=g.integers(-1, 2, (10,)))
    if t == 9:
        n['w2'] = g.integers(-1, 2, (OD, OD, 3, 3))
    else:
        n['w2'] = np.zeros((OD, OD, 3, 3), dtype=np.int64)
        for c2 in range(OD):
            tap = (t + c2) % 9
            n['w2'][c2, (5 * c2 + 7 * t) % OD, tap // 3, tap % 3] = 1
    return n


def test_one_hot_networks_single_out_every_tap():
    """The nine one-weight networks together put a weight on each of the 9 taps of each of the 24 output channels exactly once."""
    hit = sum((_net(t)['w2'] != 0).sum(axis=1) for t in range(9))
    assert hit.shape == (OD, 3, 3) and bool((hit == 1).all())


@functools.lru_cache(maxsize=None)
def _rows(rows):
    """int8 rows: 243 pixels in 0..4, dir_x and dir_y in -2..2; a one-hot of the last action on four rows of five."""
    g = np.random.default_rng(7000 + rows)
    obs = g.integers(0, 5, (rows, 245)).astype(np.int8)
    obs[:, 243:] = g.integers(-2, 3, (rows, 2))
    onehot = np.zeros((rows, A), dtype=np.int8)
    has = g.random(rows) < 0.8
    onehot[np.arange(rows)[has], g.integers(0, A, rows)[has]] = 1
    return obs, onehot


def _conv_i64(x, w, b):
    n = x.shape[2] - 2
    z = np.zeros((x.shape[0], w.shape[0], n, n), dtype=np.int64) + b.reshape(1, -1, 1, 1)
    for ky in range(3):
        for kx in range(3):
            z += np.einsum('rcij,dc->rdij', x[:, :, ky:ky + n, kx:kx + n], w[:, :, ky, kx])
    return np.maximum(z, 0)


@functools.lru_cache(maxsize=None)
def _expected(t, rows):
    """int64 [rows][610]: relu(conv2(relu(conv1(pixels)))) flattened (channel, y, x) | relu(mlp1([dir_x, dir_y, one-hot]))."""
    n = _net(t)
    obs, onehot = _rows(rows)
    x = obs[:, :243].astype(np.int64).reshape(rows, 3, 9, 9)
    a2 = _conv_i64(_conv_i64(x, n['w1'], n['b1']), n['w2'], n['b2'])
    assert int(np.abs(a2).max()) < 2 ** 20          # |w| summed: 27 * 2 * 4 + 3 = 219 per activation, 216 * 219 + 1 in conv2
    v = np.concatenate([obs[:, 243:], onehot], axis=1).astype(np.int64)
    vec = np.maximum(v @ n['mlp_w'].T + n['mlp_b'], 0)
    out = np.concatenate([a2.reshape(rows, -1), vec], axis=1)
    out.setflags(write=False)
    return out


def _dev_net(n):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).float().reshape(v.shape[0], -1).contiguous().to(DEV) for k, v in n.items()}


def _call(entry, d, obs, onehot, rows, out, out_stride, out_cols, od=OD, live=None):
    if entry == 'conv9':
        return _ops().crnn_conv9_forward(_p(obs), obs.stride(0), rows, _p(d['w1']), _p(d['b1']), _p(d['w2']), _p(d['b2']), od, _p(out),
                                         out_stride, None)
    tail = (_p(obs), obs.stride(0), _p(onehot), A, rows, _p(d['w1']), _p(d['b1']), _p(d['w2']), _p(d['b2']), _p(d['mlp_w']), _p(d['mlp_b']),
            od, _p(out), out_stride, out_cols)
    if entry == 'front9':
        return _ops().crnn_front9_forward(*tail, None)
    chips, n_live, rpc = live
    return _ops().crnn_front9_forward_live(*tail, _p(chips), _p(n_live), rpc, None)


def _equal(got, want, what):
    got, want = got.cpu().numpy().astype(np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        r, c = (int(v) for v in bad[0])
        where = 'channel %d position %d' % (c // 25, c % 25) if c < OD * 25 else 'vector feature %d' % (c - OD * 25)
        raise AssertionError('%s: %d of %d differ, first at row %d column %d (%s): got %r, expected %r'
                             % (what, len(bad), got.size, r, c, where, got[r, c], want[r, c]))


def _strided_obs(obs_np, extra):
    """The rows at a stride of 245 + extra bytes, 127 in every byte behind a row, inside guard margins."""
    obs, chk = K.guarded((obs_np.shape[0], 245 + extra), torch.int8, 127, DEV)
    obs[:, :245] = torch.from_numpy(obs_np).to(DEV)
    return obs, chk


@gpu
@pytest.mark.parametrize('rows', ROW_COUNTS)
def test_front9_integer_networks_exact(rows):
    """crnn_front9_forward, all ten networks, 640 columns into a wider sentinel-filled buffer, observation stride 245 + 11."""
    obs_np, oh_np = _rows(rows)
    obs, chk_obs = _strided_obs(obs_np, 11)
    oh = torch.from_numpy(oh_np).to(DEV)
    for t in range(10):
        d = _dev_net(_net(t))
        out, chk_out = K.guarded((rows + 3, PAD + 4), torch.float32, SENT, DEV)
        assert _call('front9', d, obs, oh, rows, out, PAD + 4, PAD) == 0
        torch.cuda.synchronize()
        chk_out()
        chk_obs()
        _equal(out[:rows, :NF], _expected(t, rows), 'network %d rows %d' % (t, rows))
        assert bool((out[:rows, NF:PAD] == 0).all()), 'columns 610..639 are not zero'
        assert bool((out[:rows, PAD:] == SENT).all()) and bool((out[rows:] == SENT).all()), 'written beside the rows'


@gpu
@pytest.mark.parametrize('rows', ROW_COUNTS)
def test_conv9_integer_networks_exact(rows):
    """crnn_conv9_forward (no vector branch, 600 columns), contiguous rows of 243 + 2 bytes and an odd output stride."""
    obs_np, _ = _rows(rows)
    obs, chk_obs = _strided_obs(obs_np, 0)
    for t in range(10):
        d = _dev_net(_net(t))
        out, chk_out = K.guarded((rows + 2, 607), torch.float32, SENT, DEV)
        assert _call('conv9', d, obs, None, rows, out, 607, 0) == 0
        torch.cuda.synchronize()
        chk_out()
        chk_obs()
        _equal(out[:rows, :600], _expected(t, rows)[:, :600], 'conv9 network %d rows %d' % (t, rows))
        assert bool((out[:rows, 600:] == SENT).all()) and bool((out[rows:] == SENT).all()), 'written beside the rows'


@gpu
@pytest.mark.parametrize('rpc,live', [(7, [1, 4]), (11, [0, 2]), (1, [0, 3, 4]), (7, [0, 1, 2, 3, 4]), (7, [])])
def test_front9_live_list_with_gaps_exact(rpc, live):
    """crnn_front9_forward_live on 5 chips of rpc rows: the listed chips' rows, compacted, exact; every row behind them untouched."""
    rows = 5 * rpc
    obs_np, oh_np = _rows(rows)
    obs, chk_obs = _strided_obs(obs_np, 3)
    oh = torch.from_numpy(oh_np).to(DEV)
    ids, chk_ids = K.guarded((5,), torch.int32, 0, DEV)
    ids[:len(live)] = torch.tensor(live, dtype=torch.int32, device=DEV)
    n_live, chk_n = K.guarded((1,), torch.int32, len(live), DEV)
    src = np.array([c * rpc + a for c in live for a in range(rpc)], dtype=np.int64)
    for t in (0, 4, 8, 9):
        d = _dev_net(_net(t))
        out, chk_out = K.guarded((rows + 2, PAD), torch.float32, SENT, DEV)
        assert _call('live', d, obs, oh, rows, out, PAD, PAD, live=(ids, n_live, rpc)) == 0
        torch.cuda.synchronize()
        for chk in (chk_out, chk_obs, chk_ids, chk_n):
            chk()
        n = len(src)
        assert bool((out[n:] == SENT).all()), 'rows behind the live ones were written'
        if n:
            _equal(out[:n, :NF], _expected(t, rows)[src], 'live %s rows_per_chip %d network %d' % (live, rpc, t))
            assert bool((out[:n, NF:] == 0).all()), 'columns 610..639 are not zero'


# ------------------------------------------------------------------------------------------------------------------------------
# the real-valued case: the bits of the build before the pair tiles, and float64
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _run_front9(obs, onehot, params, od):
    rows, pad = obs.shape[0], K.padded_cols(9, od)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).reshape(v.shape[0], -1).contiguous().to(DEV) for k, v in params.items()}
    out, chk = K.guarded((rows + 1, pad), torch.float32, SENT, DEV)
    assert _call('front9', d, torch.from_numpy(obs).to(DEV), torch.from_numpy(onehot).to(DEV), rows, out, pad, pad, od=od) == 0
    torch.cuda.synchronize()
    chk()
    assert bool((out[rows:] == SENT).all())
    return out[:rows].cpu().numpy()


def _float64(obs, onehot, p, od):
    x = torch.from_numpy(obs[:, :243]).double().view(-1, 3, 9, 9)
    t = {k: torch.from_numpy(v).double() for k, v in p.items()}
    a = torch.relu(torch.nn.functional.conv2d(x, t['w1'].view(od, 3, 3, 3), t['b1']))
    a = torch.relu(torch.nn.functional.conv2d(a, t['w2'].view(od, od, 3, 3), t['b2']))
    v = torch.cat([torch.from_numpy(obs[:, 243:245]).double(), torch.from_numpy(onehot).double()], dim=1)
    return torch.cat([a.reshape(len(obs), -1), torch.relu(v @ t['mlp_w'].t() + t['mlp_b'])], dim=1).numpy()


@gpu
def test_front9_bits_of_the_build_before_the_pair_tiles():
    g = _golden()
    params = {k: g[k] for k in ('w1', 'b1', 'w2', 'b2', 'mlp_w', 'mlp_b')}
    got, want = _run_front9(g['obs'], g['onehot'], params, OD), g['out']
    assert want.shape == (33, PAD) and got.shape == want.shape
    assert float((want[:, :600] > 0).mean()) > 0.25          # the record is not a field of zeros
    differ = got.view(np.uint32) != want.view(np.uint32)
    both_zero = (got == 0) & (want == 0)
    bad = np.argwhere(differ & ~both_zero)
    print('elements with other bits: %d, of which zeros of the other sign: %d' % (int(differ.sum()), int((differ & both_zero).sum())))
    assert len(bad) == 0, ('%d elements differ, first at %s: got %r, recorded %r'
                           % (len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _rel_l2(got, ref):
    return float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref))


@gpu
def test_front9_od24_against_float64():
    from test_gpu_crnn_ops import GRAD_TOL
    g = _golden()
    params = {k: g[k] for k in ('w1', 'b1', 'w2', 'b2', 'mlp_w', 'mlp_b')}
    got = _run_front9(g['obs'], g['onehot'], params, OD)
    err = _rel_l2(got[:, :NF], _float64(g['obs'], g['onehot'], params, OD))
    print('od 24 rel_l2 %.2e' % err)
    assert err <= GRAD_TOL
    assert bool((got[:, NF:] == 0).all())


@gpu
def test_front9_od32_against_float64():
    """od 32 has no idle columns and no pair tiles: the untouched path, 33 rows (row block: 12)."""
    from test_gpu_crnn_ops import GRAD_TOL
    torch.manual_seed(32)
    conv1, conv2, mlp = torch.nn.Conv2d(3, 32, 3), torch.nn.Conv2d(32, 32, 3), torch.nn.Linear(2 + A, 10)
    params = {k: v.detach().numpy() for k, v in dict(w1=conv1.weight, b1=conv1.bias, w2=conv2.weight, b2=conv2.bias, mlp_w=mlp.weight,
                                                     mlp_b=mlp.bias).items()}
    g = _golden()
    got = _run_front9(g['obs'], g['onehot'], params, 32)
    err = _rel_l2(got[:, :810], _float64(g['obs'], g['onehot'], params, 32))
    print('od 32 rel_l2 %.2e' % err)
    assert err <= GRAD_TOL
    assert bool((got[:, 810:] == 0).all())
