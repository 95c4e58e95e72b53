"""The fov 11 / 13 front end (include/crnn_wide.h) on the GPU: the forward against float64 torch on the CPU (conv features, the
vector branch, the zero tail) and on integer cases where float32 is exact (tests/wide_front_cases.py: bit for bit, in a
sentinel-filled buffer between guard margins, both store paths); the backward against float64 autograd (relative L2 per tensor
within GRAD_TOL) and on the exact cases for every launch shape (n_part 1 .. 256, most partial ranges empty, NaN scratch).  Row
counts come from the kernels' own block rows (crnn_wide_forward_block_rows / crnn_wide_backward_block_rows)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import wide_front_cases as W
from front_kernel_cases import N_PARTS, guarded

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GRAD_TOL = 5e-6   # relative L2 of an fp32 gradient tensor against float64 autograd (tests/test_gpu_crnn_ops.py)
SENT = -777.25    # no exact case produces it: every value there is an integer
NAN = float('nan')
CASES = [(fov, od) for fov in W.FOVS for od in W.ODS]


def _lib():
    from marl_dmfb_amd import _lib
    return _lib.crnn_wide()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _rb(fov, od):
    rb = _lib().crnn_wide_forward_block_rows(fov, od)
    assert 0 < rb and 256 * rb + rb + 1 <= 4113
    return rb


def _fwd_rows(fov, od):
    """1, RB-1, RB, RB+1, 2 RB+3 and 256 RB + RB + 1: more blocks than any grid, a ragged block behind the wrap."""
    rb = _rb(fov, od)
    return [1, rb - 1, rb, rb + 1, 2 * rb + 3, 256 * rb + rb + 1]


def _net(fov, od, seed):
    from marl_dmfb_amd.network.base_net import CRNN
    a = types.SimpleNamespace(obs_shape=(3, fov, fov, 2, 3 * fov * fov + 2), hyper_hidden_dim=od, rnn_hidden_dim=128, n_actions=5, fov=fov)
    torch.manual_seed(seed)
    net = CRNN(a).cuda()
    assert net._hip_front() == fov and net._hip_geometry() is None
    return net


def _obs(fov, rows, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randint(-10, 11, (rows, 3 * fov * fov + 2), dtype=torch.int8, generator=g)
    onehot = torch.nn.functional.one_hot(torch.randint(0, 5, (rows,), generator=g), 5).to(torch.int8)
    onehot[::3] = 0   # first steps of episodes: no last action
    return obs, onehot


def _ref_pixels(net, obs, fov):
    x = obs[:, :3 * fov * fov].double().view(-1, 3, fov, fov)
    zs = []
    for conv in net.convs:
        z = torch.nn.functional.conv2d(x, conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu())
        zs.append(z)
        x = torch.relu(z)
    return x.reshape(obs.shape[0], -1), zs


@functools.lru_cache(maxsize=None)
def _real_forward_case(fov, od):
    """One network and the most rows of _fwd_rows with their float64 reference; the smaller row counts take a prefix."""
    rows = _fwd_rows(fov, od)[-1]
    net = _net(fov, od, fov * 100 + od)
    obs, onehot = _obs(fov, rows, fov + od)
    P = 3 * fov * fov
    ref, _ = _ref_pixels(net, obs, fov)
    mw, mb = net.mlp1.weight.detach().double().cpu(), net.mlp1.bias.detach().double().cpu()
    ref_vec = torch.relu(torch.cat([obs[:, P:].double(), onehot.double()], dim=1) @ mw.t() + mb)
    ref_vec0 = torch.relu(obs[:, P:].double() @ mw[:, :2].t() + mb)
    return net, obs, onehot, ref, ref_vec, ref_vec0


@pytest.mark.parametrize('which', range(6), ids=['one', 'RB-1', 'RB', 'RB+1', '2RB+3', 'wrap'])
@pytest.mark.parametrize('fov,od', CASES)
def test_front_forward_matches_float64(fov, od, which):
    rows = _fwd_rows(fov, od)[which]
    net, obs, onehot, ref, ref_vec, ref_vec0 = _real_forward_case(fov, od)
    obs, onehot, ref, ref_vec, ref_vec0 = (t[:rows] for t in (obs, onehot, ref, ref_vec, ref_vec0))
    nc, pad = W.n_conv(fov, od), W.padded_cols(fov, od)
    with torch.no_grad():
        pix = net._pixel_features_hip(obs.cuda()).cpu()
        padded = net._front_features_hip(obs.cuda(), onehot.cuda(), padded=True).cpu()
        plain = net._front_features_hip(obs.cuda(), None).cpu()
    assert pix.shape == (rows, nc) and padded.shape == (rows, pad) and plain.shape == (rows, nc + 10)
    assert net.padded_cols() == pad == _lib().crnn_wide_padded_cols(fov, od)
    np.testing.assert_allclose(pix.numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(padded[:, :nc].numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(padded[:, nc:nc + 10].numpy(), ref_vec.numpy(), rtol=1e-5, atol=1e-5)
    assert torch.all(padded[:, nc + 10:] == 0)
    np.testing.assert_allclose(plain[:, :nc].numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(plain[:, nc:].numpy(), ref_vec0.numpy(), rtol=1e-5, atol=1e-5)   # NULL one-hot = zeros


# ---- exact integer cases ------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = ~((got == want) | (got.isnan() & want.isnan()))
    idx = tuple(int(v) for v in bad.nonzero()[0])
    raise AssertionError('%s: %d of %d elements differ, first at %s: got %r, reference %r'
                         % (what, int(bad.sum()), bad.numel(), idx, float(got[idx]), float(want[idx])))


def _all(t, value, what):
    ok = t.isnan() if value != value else t == value
    assert bool(ok.all()), '%s: %d of %d elements are not %r' % (what, int((~ok).sum()), ok.numel(), value)


def _params(c):
    d = {}
    for k in ('w1', 'b1', 'w2', 'b2', 'mlp_w', 'mlp_b'):
        d[k], _ = guarded(tuple(getattr(c, k).shape), torch.float32, 0.0, DEV)
        d[k].copy_(getattr(c, k))
    return d


def _obs_dev(c, stride, nbytes):
    """int8 [rows][stride]: the first nbytes bytes of a row from the case, 127 in every byte behind them."""
    obs, check = guarded((c.rows, stride), torch.int8, 127, DEV)
    obs[:, :nbytes] = c.obs[:, :nbytes].to(DEV)
    return obs, check


def _forward(c, d, vec, out_stride, out_cols, offset=0):
    """One forward into a sentinel-filled, guarded [rows + 3][out_stride]; checks everything beside the features."""
    fov, od, R = c.fov, c.od, c.rows
    nb = W.n_pix(fov) + (2 if vec else 0)
    obs, chk_obs = _obs_dev(c, nb + 11, nb)
    out, chk_out = guarded((R + 3, out_stride), torch.float32, SENT, DEV, offset=offset)
    assert out.data_ptr() % 16 == 4 * offset
    rc = _lib().crnn_wide_front_forward(fov, _p(obs), obs.stride(0), _p(c.onehot.to(DEV)) if vec else None, c.n_actions, R, _p(d['w1']),
                                        _p(d['b1']), _p(d['w2']), _p(d['b2']), _p(d['mlp_w']) if vec else None,
                                        _p(d['mlp_b']) if vec else None, od, _p(out), out_stride, out_cols, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    n_feat = W.n_conv(fov, od) + (10 if vec else 0)
    n_out = max(out_cols, n_feat)
    chk_out()
    chk_obs()
    _all(out[:R, n_feat:n_out], 0.0, 'zero tail')
    _all(out[:R, n_out:], SENT, 'columns between out_cols and out_stride')
    _all(out[R:], SENT, 'rows behind `rows`')
    return out, n_feat


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'out+1'])
@pytest.mark.parametrize('vec', [True, False], ids=['vec', 'novec'])
@pytest.mark.parametrize('fov,od', CASES)
def test_forward_exact_integer_cases(fov, od, vec, offset):
    """2 RB + 3 rows (two full blocks and a ragged one), out_stride = out_cols + 8, once 16-byte aligned (16-byte stores) and once
    offset by one float (4-byte stores): features equal to float64 bit for bit, the tail exactly zero, nothing written outside
    [0, out_cols) of a row, behind the last row or in the guard margins."""
    c = W.make_case(fov, od, 2 * _rb(fov, od) + 3)
    ref = W.conditions(c, backward=False)
    assert ref.bound < 2.0 ** 22 and min(ref.zeros) > 0
    pad = W.padded_cols(fov, od)
    out, n_feat = _forward(c, _params(c), vec, pad + 8, pad, offset=offset)
    _same(out[:c.rows, :n_feat], ref.out[:, :n_feat], 'fov %d od %d vec %s offset %d' % (fov, od, vec, offset))


@pytest.mark.parametrize('fov,od', CASES)
def test_forward_exact_unpadded_rows_stay_inside(fov, od):
    """out_cols = 0 with the vector branch: od P2 + 10 columns (1186 / 1578 / 1954 / 2602, no multiple of 4, so always the 4-byte
    store path) into a guarded, sentinel-filled buffer whose stride is 5 floats wider: features exact, every column from n_feat on,
    the rows behind the last and the margins untouched."""
    c = W.make_case(fov, od, 2 * _rb(fov, od) + 3)
    ref = W.conditions(c, backward=False)
    n_feat = W.n_conv(fov, od) + 10
    assert n_feat % 4 != 0
    out, got = _forward(c, _params(c), True, n_feat + 5, 0)
    assert got == n_feat
    _same(out[:c.rows, :n_feat], ref.out, 'fov %d od %d out_cols 0' % (fov, od))


def _backward(c, d, y, n_part, odd):
    """One backward launch: strides wider than needed, NaN behind the conv columns of the gradient (and of d_out when `odd`),
    127 behind the pixels, d_part NaN and sized for exactly n_part vectors, d_grads sentinel-filled."""
    fov, od, R = c.fov, c.od, c.rows
    nc, npx = W.n_conv(fov, od), W.n_pix(fov)
    obs, chk_obs = _obs_dev(c, npx + 2 + 9, npx)
    dout, chk_dout = guarded((R, W.padded_cols(fov, od) + 4), torch.float32, NAN, DEV)
    dout[:, :nc] = y[:, :nc]
    if not odd:
        dout[:, nc:y.shape[1]] = y[:, nc:]
    g, chk_g = guarded((R, nc + (13 if odd else 22)), torch.float32, NAN, DEV)
    g[:, :nc] = c.g[:, :nc].to(DEV)
    n = _lib().crnn_wide_backward_parts(fov, od)
    assert n == W.n_grads(od)
    part, chk_part = guarded((n_part * n,), torch.float32, NAN, DEV)
    grads, chk_grads = guarded((n,), torch.float32, SENT, DEV)
    rc = _lib().crnn_wide_backward(fov, _p(obs), obs.stride(0), R, _p(dout), dout.stride(0), _p(g), g.stride(0), _p(d['w1']), _p(d['b1']),
                                   _p(d['w2']), od, _p(part), n_part, _p(grads), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for chk in (chk_obs, chk_dout, chk_g, chk_part, chk_grads):
        chk()
    assert not bool((grads == SENT).any()), 'an element of d_grads was left unwritten'
    return grads


@pytest.mark.parametrize('fov,od', CASES)
def test_backward_exact_for_every_grid(fov, od):
    """37 rows with n_part 1, 2, 3, 7 and 256: one workgroup walking every block, a last workgroup with a ragged block, hundreds of
    partial ranges that stay empty.  d_out is the forward kernel's own output (shown equal to the reference first).  Gradients
    bit-equal to float64 for every n_part, and a second run gives the same bits."""
    c = W.make_case(fov, od, 37)
    ref = W.conditions(c)
    assert ref.bound < 2.0 ** 22 and min(ref.zeros) > 0
    d = _params(c)
    pad, nc = W.padded_cols(fov, od), W.n_conv(fov, od)
    y, _ = _forward(c, d, True, pad, pad)
    y = y[:c.rows]
    _same(y[:, :nc + 10], ref.out, 'forward fov %d od %d' % (fov, od))
    for k, n_part in enumerate(N_PARTS):
        a = _backward(c, d, y, n_part, odd=k % 2 == 1)
        b = _backward(c, d, y, n_part, odd=k % 2 == 0)
        assert torch.equal(a, b), 'two runs differ at n_part %d' % n_part
        o = 0
        for name, t in zip(ref.names, ref.tensors):
            _same(a[o:o + t.numel()].view(t.shape), t, 'fov %d od %d n_part %d %s' % (fov, od, n_part, name))
            o += t.numel()
        assert o == a.numel()


# ---- backward on real-valued data ---------------------------------------------------------------------------------------------
def _rel_l2(g, r):
    return float(np.linalg.norm(g.astype(np.float64) - r) / max(np.linalg.norm(r), 1e-30))


@pytest.mark.parametrize('many', [False, True], ids=['11rows', '2x7xRB+5rows'])
@pytest.mark.parametrize('fov,od', CASES)
def test_front_backward_matches_float64_autograd(fov, od, many):
    """Gradients of every CRNN front-end parameter through the HIP forward + backward (_FrontWideTrain) against float64 autograd.
    Rows with a pre-activation within 2e-5 of zero get a zero upstream gradient (their fp32 ReLU mask may differ from float64's):
    what is compared is summation error only."""
    from marl_dmfb_amd.network.base_net import _FrontWideTrain
    rbb = _lib().crnn_wide_backward_block_rows(fov, od)
    assert rbb > 0
    rows = 2 * 7 * rbb + 5 if many else 11
    net = _net(fov, od, fov * 7 + od + rows)
    obs, onehot = _obs(fov, rows, rows + 1)
    _, zs = _ref_pixels(net, obs, fov)
    safe = torch.ones(rows, dtype=torch.bool)
    for z in zs:
        safe &= z.abs().reshape(rows, -1).min(dim=1).values > 2e-5
    assert safe.float().mean() > 0.5
    cols, nc = net.padded_cols(), W.n_conv(fov, od)
    gen = torch.Generator().manual_seed(rows)
    gout = torch.randn(rows, cols, generator=gen, dtype=torch.float64) * safe[:, None]
    c1, c2 = net.convs
    params = [net.mlp1.weight, net.mlp1.bias, c1.weight, c1.bias, c2.weight, c2.bias]
    x = _FrontWideTrain.apply(obs.cuda(), onehot.cuda(), fov, net.mlp1.weight, net.mlp1.bias, cols, *params[2:])
    (x * gout.float().cuda()).sum().backward()
    got = [p.grad.detach().cpu().double().numpy() for p in params]
    ref_params = [p.detach().cpu().double().requires_grad_(True) for p in params]
    P = 3 * fov * fov
    h = obs[:, :P].double().view(rows, 3, fov, fov)
    for k in range(2):
        h = torch.relu(torch.nn.functional.conv2d(h, ref_params[2 + 2 * k], ref_params[3 + 2 * k]))
    vec = torch.cat([obs[:, P:].double(), onehot.double()], dim=1)
    v = torch.relu(vec @ ref_params[0].t() + ref_params[1])
    (h.reshape(rows, -1) * gout[:, :nc]).sum().add_((v * gout[:, nc:nc + 10]).sum()).backward()
    errs = {}
    for name, g, r in zip(['mlp_w', 'mlp_b', 'w1', 'b1', 'w2', 'b2'], got, ref_params):
        errs[name] = _rel_l2(g, r.grad.numpy())
        print('fov %d od %d rows %d %s rel_l2 %.2e' % (fov, od, rows, name, errs[name]))
    for name, err in errs.items():
        assert err <= GRAD_TOL, (name, err)
