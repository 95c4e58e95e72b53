"""The kernels of the CRNN front end one by one, through the C ABI (include/crnn_ops.h, include/crnn_fov.h), on cases where float32
is EXACT (tests/front_kernel_cases.py): small integers and sparse weights, so the kernel and the float64 reference must agree bit
for bit -- `torch.equal`, no tolerance, no excluded rows, ReLUs at exactly zero included.  A mismatch is reported with the
element and both values.  Every case asserts its exactness conditions (from the reference alone) before it touches the GPU.

Every output is sentinel-filled and sits between guard margins; what a kernel must not read is poisoned: observation bytes behind
the ones it needs are 127, gradient columns behind the conv features NaN, scratch NaN.  Row counts come from the row-block
constants of the sources as they stand (front_kernel_cases.FWD_RB / BWD_RB, where they are re-derived); the launch shapes of the
backwards run from one workgroup that walks every block to hundreds of idle ones (n_part 1, 2, 3, 7, 256).

The only tests with a tolerance are test_backward_real_valued: default-initialised weights and randn gradients at n_part 1 and
7, under the rule (_safe_rows) and the bound (GRAD_TOL) of tests/test_gpu_crnn_ops.py.

No test here launches with a bad argument: each such call must be refused on the host, and the buffers are full-sized anyway."""
import ctypes as C

import numpy as np
import pytest
import torch

import front_kernel_cases as K

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENT = -777.25          # no exact case produces it: every value there is an integer
NAN = float('nan')
OK, BAD_ARG, UNSUPPORTED = 0, -1, -6
ODS = (24, 32)


def _ops():
    from marl_dmfb_amd import _lib
    return _lib.crnn_ops()


def _fovlib():
    from marl_dmfb_amd import _lib
    return _lib.crnn_fov()


def _sync():
    torch.cuda.synchronize()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _same(got, want, what):
    """Bit-for-bit equality of a float32 result with the float64 reference; the first differing element is named."""
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
    """The case's parameters on the device, each in a guarded buffer of its own."""
    d = {}
    for k in ('w1', 'b1', 'w2', 'b2', 'mlp_w', 'mlp_b'):
        t = getattr(c, k)
        if t is None:
            d[k] = None
            continue
        d[k], _ = K.guarded(tuple(t.shape), torch.float32, 0.0, DEV)
        d[k].copy_(t)
    return d


def _obs(c, stride, nbytes):
    """int8 [rows][stride] with the first nbytes bytes of a row from the case and 127 in every byte behind them."""
    obs, check = K.guarded((c.rows, stride), torch.int8, 127, DEV)
    obs[:, :nbytes] = c.obs[:, :nbytes].to(DEV)
    return obs, check


# ------------------------------------------------------------------------------------------------------------------------------
# forwards
# ------------------------------------------------------------------------------------------------------------------------------
# (entry, fov, vector branch)
FORWARDS = [('conv9', 9, False), ('front9', 9, True), ('front19', 19, True), ('front19', 19, False), ('fov', 5, True), ('fov', 5, False),
            ('fov', 7, True), ('fov', 7, False)]
FWD_IDS = ['conv9', 'front9', 'front19', 'front19-novec', 'fov5', 'fov5-novec', 'fov7', 'fov7-novec']


def _call_forward(entry, c, d, vec, obs, onehot, n_actions, rows, out, out_stride, out_cols, live=None):
    mw, mb = (d['mlp_w'], d['mlp_b']) if vec else (None, None)
    if entry == 'conv9':
        return _ops().crnn_conv9_forward(_p(obs), obs.stride(0), rows, _p(d['w1']), _p(d['b1']), _p(d['w2']), _p(d['b2']), c.od,
                                         _p(out), out_stride, None)
    tail = (_p(obs), obs.stride(0), _p(onehot), n_actions, rows, _p(d['w1']), _p(d['b1']), _p(d['w2']), _p(d['b2']), _p(mw), _p(mb),
            c.od, _p(out), out_stride, out_cols)
    if entry == 'front9':
        return _ops().crnn_front9_forward(*tail, None)
    if entry == 'front9_live':
        chips, n_live, rpc = live
        return _ops().crnn_front9_forward_live(*tail, _p(chips), _p(n_live), rpc, None)
    if entry == 'front19':
        return _ops().crnn_front19_forward(*tail, None)
    return _fovlib().crnn_fov_front_forward(c.fov, *tail, None)


def _forward(entry, c, vec, out_stride, out_cols, offset=0, onehot='case', extra_obs=11, d=None):
    """Runs one forward on case `c` into a sentinel-filled, guarded [rows + 3][out_stride] and checks everything beside the
    features: zero tail, the columns up to out_stride, the rows behind `rows`, the guard margins.  -> (out, n_feat)."""
    fov, od, R = c.fov, c.od, c.rows
    d = d or _params(c)
    nb = K.n_pix(fov) + (2 if vec else 0)
    obs, chk_obs = _obs(c, nb + extra_obs, nb)
    oh = c.onehot.to(DEV) if (vec and onehot == 'case') else None
    out, chk_out = K.guarded((R + 3, out_stride), torch.float32, SENT, DEV, offset=offset)
    rc = _call_forward(entry, c, d, vec, obs, oh, c.n_actions, R, out, out_stride, out_cols)
    assert rc == OK, rc
    _sync()
    n_feat = K.n_conv(fov, od) + (10 if vec else 0)
    n_out = max(out_cols, n_feat)
    chk_out()
    chk_obs()
    _all(out[:R, n_feat:n_out], 0.0, 'zero tail')
    _all(out[:R, n_out:], SENT, 'columns between out_cols and out_stride')
    _all(out[R:], SENT, 'rows behind `rows`')
    return out, n_feat


@pytest.mark.parametrize('od', ODS)
@pytest.mark.parametrize('which', range(5), ids=['one', 'RB-1', 'RB', 'RB+1', 'wrap'])
@pytest.mark.parametrize('entry,fov,vec', FORWARDS, ids=FWD_IDS)
def test_forward_rows_exact(entry, fov, vec, which, od):
    """Row counts 1, RB-1, RB, RB+1 and one at which the persistent loop wraps with a ragged last block (front_kernel_cases.fwd_rows:
    RB 16 / 12 for fov 9, 8 for fov 19, 16 for fov 5 / 7; grid 256 x workgroups per CU), rows padded out to the GEMM width."""
    c = K.make_case(fov, od, K.fwd_rows(fov, od)[which])
    ref = K.conditions(c, backward=False)
    pad = K.padded_cols(fov, od)
    out, n_feat = _forward(entry, c, vec, pad + 8, 0 if entry == 'conv9' else pad)
    _same(out[:c.rows, :n_feat], ref.out[:, :n_feat], '%s fov %d od %d rows %d' % (entry, fov, od, c.rows))


# store path -> (out_stride - padded, offset of `out` in floats).  fov 9 / 19 pick 16-byte, 8-byte or scalar stores from the
# stride, the alignment of `out` and the columns written; fov 5 / 7 16-byte or scalar.
STORE_PATHS = {'aligned': (8, 0), 'stride%4=2': (6, 0), 'odd-stride': (7, 0), 'out+1': (8, 1), 'out+2': (8, 2), 'out+3': (8, 3)}


# crnn_conv9_forward has no out_cols: one column count, od*25
STORE_CASES = [(e, f, v, p) for (e, f, v) in FORWARDS for p in (True, False) if p or e != 'conv9']
STORE_IDS = ['%s-%s' % (i, 'cols-padded' if p else 'cols-0') for (e, f, v), i in zip(FORWARDS, FWD_IDS) for p in (True, False) if p or e != 'conv9']


@pytest.mark.parametrize('od', ODS)
@pytest.mark.parametrize('path', sorted(STORE_PATHS))
@pytest.mark.parametrize('entry,fov,vec,padded', STORE_CASES, ids=STORE_IDS)
def test_forward_store_paths_exact(entry, fov, vec, padded, path, od):
    """16-byte stores (aligned, padded columns), the fall-back to 8 bytes (out_cols = 0: 610 / 810 columns; a stride or an `out`
    that is a multiple of 8 bytes only) and scalar stores (odd stride, `out` 4-byte aligned only), each with and without the
    zero tail, at RB + 1 rows: features exact, tail exactly zero, nothing written beside them."""
    c = K.make_case(fov, od, K.FWD_RB[(fov, od)] + 1)
    ref = K.conditions(c, backward=False)
    pad = K.padded_cols(fov, od)
    extra, offset = STORE_PATHS[path]
    out, n_feat = _forward(entry, c, vec, pad + extra, pad if padded and entry != 'conv9' else 0, offset=offset)
    assert out.data_ptr() % 16 == 4 * offset
    _same(out[:c.rows, :n_feat], ref.out[:, :n_feat], '%s fov %d od %d %s' % (entry, fov, od, path))


@pytest.mark.parametrize('od', ODS)
@pytest.mark.parametrize('variant', ['A0', 'A1', 'A16', 'no-onehot'])
@pytest.mark.parametrize('entry,fov', [('front9', 9), ('front19', 19), ('fov', 5), ('fov', 7)], ids=['front9', 'front19', 'fov5', 'fov7'])
def test_forward_vector_branch_exact(entry, fov, variant, od):
    """relu(mlp1([dir_x, dir_y, one-hot])) with 0, 1 and 16 actions and with d_onehot = NULL (all zeros), obs_stride wider than
    the row with 127 in every byte behind dir_y."""
    A = {'A0': 0, 'A1': 1, 'A16': 16}.get(variant, 5)
    c = K.make_case(fov, od, K.FWD_RB[(fov, od)] + 1, n_actions=A)
    ref = K.conditions(c, backward=False)
    pad = K.padded_cols(fov, od)
    out, n_feat = _forward(entry, c, True, pad, pad, onehot='none' if variant == 'no-onehot' else 'case')
    nc = K.n_conv(fov, od)
    _same(out[:c.rows, :nc], ref.conv, 'conv features')
    want = ref.vec
    if variant == 'no-onehot':
        dirs = c.obs[:, K.n_pix(fov):K.n_pix(fov) + 2].double()
        want = torch.relu(dirs @ c.mlp_w[:, :2].double().t() + c.mlp_b.double())
        assert not torch.equal(want, ref.vec)        # the one-hot matters in this case
    _same(out[:c.rows, nc:n_feat], want, 'vector features (%s)' % variant)


@pytest.mark.parametrize('od', ODS)
@pytest.mark.parametrize('rpc', [1, 7, 64])
def test_front9_live_rows_exact(od, rpc):
    """crnn_front9_forward_live: *d_n_live = 0 writes nothing; 1, some and all chips give, bit for bit, what the plain kernel gives
    on the gathered rows (and the reference); every row from n_live * rows_per_chip on keeps the sentinel."""
    chips = 5
    c = K.make_case(9, od, chips * rpc)
    ref = K.conditions(c, backward=False)
    d = _params(c)
    pad, n_feat = K.padded_cols(9, od), od * 25 + 10
    obs, chk_obs = _obs(c, 245 + 3, 245)
    oh = c.onehot.to(DEV)
    for live in ([], [3], [0, 2, 4], [0, 1, 2, 3, 4]):
        ids, chk_ids = K.guarded((chips,), torch.int32, 0, DEV)       # entries behind n_live: chip 0, valid if ever read
        ids[:len(live)] = torch.tensor(live, dtype=torch.int32, device=DEV)
        n_live, chk_n = K.guarded((1,), torch.int32, len(live), DEV)
        out, chk_out = K.guarded((c.rows + 3, pad + 4), torch.float32, SENT, DEV)
        rc = _call_forward('front9_live', c, d, True, obs, oh, c.n_actions, c.rows, out, pad + 4, pad, live=(ids, n_live, rpc))
        assert rc == OK
        _sync()
        for chk in (chk_ids, chk_n, chk_out, chk_obs):
            chk()
        n = len(live) * rpc
        _all(out[n:], SENT, 'rows behind the live ones (n_live %d)' % len(live))
        if not live:
            continue
        src = (torch.tensor(live).view(-1, 1) * rpc + torch.arange(rpc).view(1, -1)).reshape(-1)
        _same(out[:n, :n_feat], ref.out[src], 'live rows, od %d rows_per_chip %d live %s' % (od, rpc, live))
        _all(out[:n, n_feat:pad], 0.0, 'zero tail')
        _all(out[:n, pad:], SENT, 'columns behind out_cols')
        plain, _ = K.guarded((n, pad + 4), torch.float32, SENT, DEV)
        g_obs, g_oh = obs[src.to(DEV)].contiguous(), oh[src.to(DEV)].contiguous()
        assert _call_forward('front9', c, d, True, g_obs, g_oh, c.n_actions, n, plain, pad + 4, pad) == OK
        _sync()
        assert torch.equal(out[:n, :pad], plain[:, :pad])


# ------------------------------------------------------------------------------------------------------------------------------
# backwards
# ------------------------------------------------------------------------------------------------------------------------------
def _parts(fov, od):
    if fov == 9:
        return _ops().crnn_conv9_backward_parts(od)
    if fov == 19:
        return _ops().crnn_conv19_backward_parts(od)
    return _fovlib().crnn_fov_backward_parts(fov, od)


def _call_backward(fov, od, d, obs, rows, dout, g, part, n_part, grads):
    head = (_p(obs), obs.stride(0), rows, _p(dout), dout.stride(0), _p(g), g.stride(0), _p(d['w1']), _p(d['b1']))
    tail = (od, _p(part), n_part, _p(grads), None)
    if fov == 9:
        return _ops().crnn_conv9_backward(*head, _p(d['w2']), *tail)
    if fov == 19:
        return _ops().crnn_conv19_backward(*head, _p(d['w2']), _p(d['b2']), *tail)
    return _fovlib().crnn_fov_backward(fov, *head, _p(d['w2']), *tail)


def _backward(c, d, y, g_rows, n_part, strides, nan_tail):
    """One backward launch.  y = the forward's rows [rows][>= n_conv + 10]; strides = (obs, out, grad), each wider than needed.
    d_out carries the forward's vector features and zero tail behind the conv features, or NaN there (nan_tail); the gradient
    columns behind the conv features are NaN, the observation bytes behind the pixels 127, d_part NaN and sized for exactly
    n_part vectors, d_grads sentinel-filled.  -> d_grads (every element written, nothing beside it)."""
    fov, od, R = c.fov, c.od, c.rows
    nc, npx = K.n_conv(fov, od), K.n_pix(fov)
    s_obs, s_out, s_grad = strides
    obs, chk_obs = _obs(c, s_obs, npx)
    dout, chk_dout = K.guarded((R, s_out), torch.float32, NAN, DEV)
    dout[:, :nc] = y[:, :nc]
    if not nan_tail:
        w = min(s_out, y.shape[1])
        dout[:, nc:w] = y[:, nc:w]
    g, chk_g = K.guarded((R, s_grad), torch.float32, NAN, DEV)
    g[:, :nc] = g_rows[:, :nc]
    part, chk_part = K.guarded((n_part * _parts(fov, od),), torch.float32, NAN, DEV)
    grads, chk_grads = K.guarded((K.n_grads(fov, od),), torch.float32, SENT, DEV)
    rc = _call_backward(fov, od, d, obs, R, dout, g, part, n_part, grads)
    assert rc == OK, rc
    _sync()
    for chk in (chk_obs, chk_dout, chk_g, chk_part, chk_grads):
        chk()
    assert not bool((grads == SENT).any()), 'an element of d_grads was left unwritten'
    return grads


def _named(ref, flat, what):
    """Compares a flat gradient with the reference tensor by tensor, so that a mismatch names dW2 / db2 / dW1 / db1 and the index."""
    o = 0
    for name, t in zip(ref.names, ref.tensors):
        _same(flat[o:o + t.numel()].view(t.shape), t, '%s %s' % (what, name))
        o += t.numel()
    assert o == flat.numel()


def _strides(fov, od, odd_grad):
    nc, npx = K.n_conv(fov, od), K.n_pix(fov)
    return (npx + 2 + 9, K.padded_cols(fov, od) + 4, nc + (13 if odd_grad else 22))


BWD_CASES = [(fov, od, rows) for fov in (9, 19, 7, 5) for od in ODS for rows in K.bwd_rows(fov, od)]


@pytest.mark.parametrize('fov,od,rows', BWD_CASES)
def test_backward_exact_for_every_grid(fov, od, rows):
    """crnn_conv9_backward / crnn_conv19_backward / crnn_fov_backward at 1, RBB-1, RBB+1, 3 RBB+2 and 10 RBB+3 rows (RBB 10 / 6, 4 / 2,
    8 for fov 7, 32 for fov 5) with n_part 1, 2, 3, 7 and 256: one workgroup walking every block (the prefetch across blocks), a
    last workgroup without a block, hundreds of idle workgroups whose vectors must still count as zeros.  d_out is the forward
    kernel's own output (shown equal to the reference first).  Three different strides, each wider than needed; even n_part
    indices use an even gradient stride and the forward's real columns behind the conv features, odd ones an odd gradient stride
    and NaN there.  Exact for every n_part, hence identical across n_part; the vector branch's gradient (crnn_mlp_backward)
    from the same rows is exact too."""
    c = K.make_case(fov, od, rows)
    ref = K.conditions(c)
    d = _params(c)
    pad, nc = K.padded_cols(fov, od), K.n_conv(fov, od)
    y, _ = _forward({9: 'front9', 19: 'front19'}.get(fov, 'fov'), c, True, pad, pad, d=d)
    y = y[:rows]
    _same(y[:, :nc + 10], ref.out, 'forward fov %d od %d rows %d' % (fov, od, rows))
    g_rows = c.g.to(DEV)
    for k, n_part in enumerate(K.N_PARTS):
        grads = _backward(c, d, y, g_rows, n_part, _strides(fov, od, odd_grad=k % 2 == 1), nan_tail=k % 2 == 1)
        _named(ref, grads, 'fov %d od %d rows %d n_part %d' % (fov, od, rows, n_part))
    # the vector branch of the same rows
    obs, chk_obs = _obs(c, K.n_pix(fov) + 2 + 5, K.n_pix(fov) + 2)
    g, _ = K.guarded((rows, nc + 10 + 3), torch.float32, NAN, DEV)
    g[:, nc:nc + 10] = g_rows[:, nc:]
    dw, db = _mlp_backward(obs, K.n_pix(fov), c.onehot.to(DEV), y, g, nc)
    _same(dw, ref.mlp_dw, 'mlp dW')
    _same(db, ref.mlp_db, 'mlp db')
    chk_obs()


@pytest.mark.parametrize('fov,od', [(9, 24), (9, 32), (19, 24), (19, 32)])
def test_backward_twice_gives_identical_bits(fov, od):
    """Two launches on the same inputs, real-valued so that the order of the additions shows: the same bits, at n_part 7 and 256."""
    rows = 10 * K.BWD_RB[(fov, od)] + 3
    d, c, y, g = _real_case(fov, od, rows)
    for n_part in (7, 256):
        a = _backward(c, d, y, g, n_part, _strides(fov, od, False), nan_tail=False)
        b = _backward(c, d, y, g, n_part, _strides(fov, od, True), nan_tail=True)
        assert torch.equal(a, b), 'fov %d od %d n_part %d' % (fov, od, n_part)


def _mlp_backward(obs, dir_off, onehot, x, g, col0):
    A = onehot.shape[1]
    part, chk_part = K.guarded((_ops().crnn_mlp_backward_parts(),), torch.float32, NAN, DEV)
    dw, chk_dw = K.guarded((10, 2 + A), torch.float32, SENT, DEV)
    db, chk_db = K.guarded((10,), torch.float32, SENT, DEV)
    rc = _ops().crnn_mlp_backward(_p(obs), obs.stride(0), dir_off, _p(onehot), A, obs.shape[0], _p(x), x.stride(0), _p(g), g.stride(0),
                                  col0, _p(part), _p(dw), _p(db), None)
    assert rc == OK, rc
    _sync()
    for chk in (chk_part, chk_dw, chk_db):
        chk()
    assert not bool((dw == SENT).any()) and not bool((db == SENT).any())
    return dw, db


def _mlp_inputs(m, dir_off, col0, width):
    obs, _ = K.guarded((m.rows, dir_off + 2 + 3), torch.int8, 127, DEV)
    obs[:, dir_off:dir_off + 2] = m.dirs.to(DEV)
    x, _ = K.guarded((m.rows, width), torch.float32, NAN, DEV)
    x[:, col0:col0 + 10] = m.x.to(DEV)
    g, _ = K.guarded((m.rows, width + 1), torch.float32, NAN, DEV)
    g[:, col0:col0 + 10] = m.g.to(DEV)
    return obs, m.onehot.to(DEV), x, g


@pytest.mark.parametrize('rows,A', [(1, 5), (255, 1), (256, 16), (257, 5), (513, 2), (70001, 16)])
def test_mlp_backward_exact(rows, A):
    """One workgroup per 256 rows, at most 256: 1, 255, 256, 257, 513 and 70001 rows (274 blocks on 256 workgroups: the grid-stride
    loop wraps).  Everything the kernel must not read is NaN / 127, the scratch NaN."""
    m = K.mlp_case(rows, A, seed=rows + A)
    assert m.bound < K.BOUND_LIMIT and bool((m.dw != 0).any()) and bool((m.db != 0).any())
    obs, oh, x, g = _mlp_inputs(m, dir_off=7, col0=3, width=15)
    dw, db = _mlp_backward(obs, 7, oh, x, g, 3)
    _same(dw, m.dw, 'mlp dW rows %d' % rows)
    _same(db, m.db, 'mlp db rows %d' % rows)


def test_mlp_backward_back_to_back_on_one_stream():
    """Three calls without a synchronisation between them, on 1, 2 and 256 workgroups: the hand-off word must be back at zero
    after every call, or a later call adds its partial vectors too early or never."""
    lib = _ops()
    runs = []
    for rows in (200, 300, 70001, 257, 1):
        m = K.mlp_case(rows, 5, seed=rows)
        obs, oh, x, g = _mlp_inputs(m, dir_off=2, col0=0, width=12)
        part, _ = K.guarded((lib.crnn_mlp_backward_parts(),), torch.float32, NAN, DEV)
        dw, chk_dw = K.guarded((10, 7), torch.float32, SENT, DEV)
        db, chk_db = K.guarded((10,), torch.float32, SENT, DEV)
        runs.append((m, obs, oh, x, g, part, dw, db, chk_dw, chk_db))
    for m, obs, oh, x, g, part, dw, db, _, _ in runs:
        assert lib.crnn_mlp_backward(_p(obs), obs.stride(0), 2, _p(oh), 5, m.rows, _p(x), x.stride(0), _p(g), g.stride(0), 0, _p(part),
                                     _p(dw), _p(db), None) == OK
    _sync()
    for m, _, _, _, _, _, dw, db, chk_dw, chk_db in runs:
        _same(dw, m.dw, 'mlp dW rows %d' % m.rows)
        _same(db, m.db, 'mlp db rows %d' % m.rows)
        chk_dw()
        chk_db()


# ------------------------------------------------------------------------------------------------------------------------------
# real-valued cases: the only ones with a tolerance
# ------------------------------------------------------------------------------------------------------------------------------
def _rel_l2(g, r):
    return float(np.linalg.norm(g.astype(np.float64) - r) / max(np.linalg.norm(r), 1e-30))


def _real_case(fov, od, rows):
    """Default-initialised conv layers (torch.nn.Conv2d), pixels in [-10, 10] as the tests of test_gpu_crnn_ops.py draw them, a
    randn gradient that is zero on every row with a pre-activation within 2e-5 of zero (their _safe_rows rule).
    -> (device parameters, case, forward kernel's rows, gradient rows), the float64 gradients in case.ref."""
    torch.manual_seed(100 * fov + od)
    conv1 = torch.nn.Conv2d(3, od, 3, stride=2 if fov == 19 else 1)
    conv2 = torch.nn.Conv2d(od, od, 3) if fov != 5 else None
    mlp = torch.nn.Linear(2 + K.N_ACTIONS, 10)
    c = K.make_case(fov, od, rows)
    c.obs = torch.randint(-10, 11, c.obs.shape, dtype=torch.int8)
    c.w1, c.b1 = conv1.weight.detach(), conv1.bias.detach()
    c.w2, c.b2 = (conv2.weight.detach(), conv2.bias.detach()) if conv2 is not None else (None, None)
    c.mlp_w, c.mlp_b = mlp.weight.detach(), mlp.bias.detach()
    c.g = torch.randn(c.g.shape)
    p64 = [None if t is None else t.double().requires_grad_(True) for t in (c.w1, c.b1, c.w2, c.b2)]
    x = c.obs[:, :K.n_pix(fov)].double().view(rows, 3, fov, fov)
    zs, acts = K._stack(fov, x, p64[0], p64[1], p64[2], p64[3], torch.relu)
    safe = torch.ones(rows, dtype=torch.bool)
    for z in zs:
        safe &= z.detach().abs().reshape(rows, -1).min(dim=1).values > 2e-5
    assert int(safe.sum()) >= rows - rows // 4
    c.g[~safe] = 0.0
    nc = K.n_conv(fov, od)
    (acts[-1].reshape(rows, -1) * c.g[:, :nc].double()).sum().backward()
    tensors = ([p64[2].grad, p64[3].grad] if conv2 is not None else []) + [p64[0].grad, p64[1].grad]
    names = ((('dW3', 'db3') if fov == 19 else ('dW2', 'db2')) if conv2 is not None else ()) + ('dW1', 'db1')
    c.ref = names, [t.detach() for t in tensors]
    d = _params(c)
    pad = K.padded_cols(fov, od)
    y, _ = _forward({9: 'front9', 19: 'front19'}.get(fov, 'fov'), c, True, pad, pad, d=d)
    return d, c, y[:rows], c.g.to(DEV)


@pytest.mark.parametrize('fov,od', [(9, 24), (9, 32), (19, 24), (19, 32), (7, 24), (7, 32), (5, 24), (5, 32)])
def test_backward_real_valued(fov, od):
    """The small grids on data that is not sparse integers: default-initialised weights, randn gradients, 10 RBB + 3 rows, n_part 1
    and 7, against float64 autograd; relative L2 per tensor within GRAD_TOL = 5e-6 of tests/test_gpu_crnn_ops.py (their rule for
    knife-edge rows)."""
    from test_gpu_crnn_ops import GRAD_TOL
    rows = 10 * K.BWD_RB[(fov, od)] + 3
    d, c, y, g = _real_case(fov, od, rows)
    names, tensors = c.ref
    for n_part in (1, 7):
        grads = _backward(c, d, y, g, n_part, _strides(fov, od, n_part == 7), nan_tail=n_part == 7)
        assert bool(torch.isfinite(grads).all())
        o = 0
        for name, t in zip(names, tensors):
            err = _rel_l2(grads[o:o + t.numel()].cpu().numpy(), t.reshape(-1).numpy())
            print('real-valued fov=%d od=%d rows=%d n_part=%d %s rel_l2=%.2e' % (fov, od, rows, n_part, name, err))
            assert err <= GRAD_TOL, (name, n_part, err)
            o += t.numel()
        assert o == grads.numel()


# ------------------------------------------------------------------------------------------------------------------------------
# the argument contract: every bad call is refused on the host, nothing is launched, no output changes
# ------------------------------------------------------------------------------------------------------------------------------
class _Args:
    """Ordered, named arguments of one entry point, all valid, over full-sized buffers; call(**changes) replaces some."""

    def __init__(self, fn, items, outputs):
        self.fn, self.items, self.outputs = fn, items, outputs

    def call(self, **changes):
        assert set(changes) <= {k for k, _ in self.items}, changes
        vals = [changes.get(k, v) for k, v in self.items]
        return self.fn(*[_p(v) if torch.is_tensor(v) else v for v in vals])

    def pointers(self):
        return [k for k, v in self.items if torch.is_tensor(v)]

    def untouched(self):
        _sync()
        for t, fill, chk in self.outputs:
            _all(t, fill, 'an output after refused calls')
            chk()


ROWS_ARG = 4


def _forward_args(entry, fov, od, vec=True):
    c = K.make_case(fov, od, ROWS_ARG)
    d = _params(c)
    pad = K.padded_cols(fov, od)
    obs, _ = _obs(c, K.n_pix(fov) + 2, K.n_pix(fov) + 2)
    out, chk = K.guarded((ROWS_ARG + 2, pad + 8), torch.float32, SENT, DEV)
    lib = _fovlib() if entry == 'fov' else _ops()
    if entry == 'conv9':
        items = [('obs', obs), ('obs_stride', obs.stride(0)), ('rows', ROWS_ARG), ('w1', d['w1']), ('b1', d['b1']), ('w2', d['w2']),
                 ('b2', d['b2']), ('od', od), ('out', out), ('out_stride', pad + 8), ('stream', None)]
        return _Args(lib.crnn_conv9_forward, items, [(out, SENT, chk)])
    items = [('obs', obs), ('obs_stride', obs.stride(0)), ('onehot', c.onehot.to(DEV)), ('n_actions', c.n_actions), ('rows', ROWS_ARG),
             ('w1', d['w1']), ('b1', d['b1']), ('w2', d['w2']), ('b2', d['b2']), ('mlp_w', d['mlp_w'] if vec else None),
             ('mlp_b', d['mlp_b'] if vec else None), ('od', od), ('out', out), ('out_stride', pad + 8), ('out_cols', pad)]
    if entry == 'front9_live':
        ids = torch.arange(ROWS_ARG, dtype=torch.int32, device=DEV)
        n_live = torch.full((1,), ROWS_ARG, dtype=torch.int32, device=DEV)
        items += [('live_chips', ids), ('n_live', n_live), ('rows_per_chip', 1)]
    items.append(('stream', None))
    if entry == 'fov':
        items.insert(0, ('fov', fov))
    fn = getattr(lib, {'front9': 'crnn_front9_forward', 'front9_live': 'crnn_front9_forward_live', 'front19': 'crnn_front19_forward',
                       'fov': 'crnn_fov_front_forward'}[entry])
    return _Args(fn, items, [(out, SENT, chk)])


@pytest.mark.parametrize('entry,fov', [('conv9', 9), ('front9', 9), ('front9_live', 9), ('front19', 19), ('fov', 5), ('fov', 7)],
                         ids=['conv9', 'front9', 'front9_live', 'front19', 'fov5', 'fov7'])
def test_forward_argument_contract(entry, fov):
    od = 24
    a = _forward_args(entry, fov, od)
    npx, nc, pad = K.n_pix(fov), K.n_conv(fov, od), K.padded_cols(fov, od)
    vec = entry != 'conv9'
    n_feat = nc + (10 if vec else 0)
    optional = {'onehot'} | ({'mlp_w'} if entry in ('front19', 'fov') else set()) | ({'w2', 'b2'} if fov == 5 else set())
    for name in a.pointers():
        if name not in optional:
            assert a.call(**{name: None}) == BAD_ARG, name
    assert a.call(rows=-1) == BAD_ARG
    assert a.call(rows=0) == OK
    assert a.call(od=16) == UNSUPPORTED
    assert a.call(obs_stride=npx + (1 if vec else -1)) == BAD_ARG
    assert a.call(out_stride=n_feat - 1, **({'out_cols': 0} if vec else {})) == BAD_ARG
    if vec:
        assert a.call(n_actions=17) == BAD_ARG and a.call(n_actions=-1) == BAD_ARG
        assert a.call(out_cols=n_feat - 1) == BAD_ARG
        assert a.call(out_cols=pad + 1) == BAD_ARG
        assert a.call(out_cols=n_feat + 4, out_stride=n_feat + 2) == BAD_ARG
    if entry in ('front19', 'fov'):        # without the vector branch: the pixel bytes alone, od*25 / od*9 columns
        assert a.call(mlp_w=None, mlp_b=None, obs_stride=npx - 1, out_cols=0) == BAD_ARG
        assert a.call(mlp_w=None, mlp_b=None, out_stride=nc - 1, out_cols=0) == BAD_ARG
        assert a.call(mlp_w=None, mlp_b=None, out_cols=nc - 1) == BAD_ARG
    if entry == 'fov':
        assert a.call(fov=9) == UNSUPPORTED and a.call(fov=19) == UNSUPPORTED and a.call(fov=6) == UNSUPPORTED
    if entry == 'front9_live':
        assert a.call(rows=ROWS_ARG, rows_per_chip=3) == BAD_ARG          # rows % rows_per_chip != 0
        assert a.call(rows_per_chip=0) == BAD_ARG
        assert a.call(rows=65, rows_per_chip=65) == BAD_ARG
        assert a.call(rows=1 << 25) == BAD_ARG                            # refused before any launch: no such buffer exists
    a.untouched()


def _backward_args(fov, od):
    c = K.make_case(fov, od, ROWS_ARG)
    d = _params(c)
    nc, npx = K.n_conv(fov, od), K.n_pix(fov)
    obs, _ = _obs(c, npx + 2, npx)
    y = K.reference(c).out.float().to(DEV)
    dout, _ = K.guarded((ROWS_ARG + 2, nc + 10), torch.float32, 0.0, DEV)
    dout[:ROWS_ARG] = y
    g, _ = K.guarded((ROWS_ARG + 2, nc + 10), torch.float32, 0.0, DEV)
    g[:ROWS_ARG] = c.g.to(DEV)
    part, chk_part = K.guarded((258 * _parts(fov, od),), torch.float32, NAN, DEV)
    grads, chk_grads = K.guarded((K.n_grads(fov, od),), torch.float32, SENT, DEV)
    items = [('obs', obs), ('obs_stride', obs.stride(0)), ('rows', ROWS_ARG), ('out', dout), ('out_stride', nc + 10), ('g', g),
             ('grad_stride', nc + 10), ('w1', d['w1']), ('b1', d['b1']), ('w2', d['w2'])]
    if fov == 19:
        items.append(('b2', d['b2']))
    items += [('od', od), ('part', part), ('n_part', 4), ('grads', grads), ('stream', None)]
    if fov in (5, 7):
        items.insert(0, ('fov', fov))
    fn = {9: _ops().crnn_conv9_backward, 19: _ops().crnn_conv19_backward}.get(fov) or _fovlib().crnn_fov_backward
    return _Args(fn, items, [(part, NAN, chk_part), (grads, SENT, chk_grads)])


@pytest.mark.parametrize('od', ODS)
@pytest.mark.parametrize('fov', [9, 19, 7, 5])
def test_backward_argument_contract(fov, od):
    """Also the contract crnn_conv9_backward did not check: a stride shorter than what a row is read for -- a gradient stride of 0,
    which an expanded gradient has, was launched and read as row 0 for every row."""
    a = _backward_args(fov, od)
    nc, npx = K.n_conv(fov, od), K.n_pix(fov)
    for name in a.pointers():
        if not (fov == 5 and name == 'w2'):
            assert a.call(**{name: None}) == BAD_ARG, name
    assert a.call(rows=0) == BAD_ARG and a.call(rows=-1) == BAD_ARG
    assert a.call(od=16) == UNSUPPORTED
    assert a.call(n_part=0) == BAD_ARG and a.call(n_part=257) == BAD_ARG
    assert a.call(obs_stride=npx - 1) == BAD_ARG
    assert a.call(out_stride=nc - 1) == BAD_ARG
    assert a.call(grad_stride=nc - 1) == BAD_ARG
    assert a.call(grad_stride=0) == BAD_ARG
    assert a.call(out_stride=0) == BAD_ARG and a.call(obs_stride=0) == BAD_ARG
    if fov in (5, 7):
        assert a.call(fov=9) == UNSUPPORTED and a.call(fov=19) == UNSUPPORTED
    a.untouched()


def test_mlp_backward_argument_contract():
    lib = _ops()
    m = K.mlp_case(ROWS_ARG, 5, seed=1)
    obs, oh, x, g = _mlp_inputs(m, dir_off=243, col0=600, width=610)
    part, chk_part = K.guarded((lib.crnn_mlp_backward_parts(),), torch.float32, NAN, DEV)
    dw, chk_dw = K.guarded((10, 18), torch.float32, SENT, DEV)
    db, chk_db = K.guarded((10,), torch.float32, SENT, DEV)
    items = [('obs', obs), ('obs_stride', obs.stride(0)), ('dir_offset', 243), ('onehot', oh), ('n_actions', 5), ('rows', ROWS_ARG), ('out', x),
             ('out_stride', x.stride(0)), ('g', g), ('grad_stride', g.stride(0)), ('col0', 600), ('part', part), ('grad_w', dw), ('grad_b', db),
             ('stream', None)]
    a = _Args(lib.crnn_mlp_backward, items, [(part, NAN, chk_part), (dw, SENT, chk_dw), (db, SENT, chk_db)])
    for name in a.pointers():
        assert a.call(**{name: None}) == BAD_ARG, name
    assert a.call(rows=0) == BAD_ARG and a.call(rows=-1) == BAD_ARG
    assert a.call(n_actions=17) == BAD_ARG and a.call(n_actions=-1) == BAD_ARG
    assert a.call(dir_offset=-1) == BAD_ARG and a.call(col0=-1) == BAD_ARG
    assert a.call(obs_stride=244) == BAD_ARG and a.call(obs_stride=0) == BAD_ARG
    assert a.call(out_stride=609) == BAD_ARG and a.call(out_stride=0) == BAD_ARG
    assert a.call(grad_stride=609) == BAD_ARG and a.call(grad_stride=0) == BAD_ARG
    a.untouched()


def test_part_sizes_cover_the_gradient_layouts():
    for od in ODS:
        assert _ops().crnn_conv9_backward_parts(od) >= K.n_grads(9, od) and _ops().crnn_conv19_backward_parts(od) >= K.n_grads(19, od)
        assert _fovlib().crnn_fov_backward_parts(7, od) == K.n_grads(7, od) and _fovlib().crnn_fov_backward_parts(5, od) == K.n_grads(5, od)
        assert _ops().crnn_front_padded_cols(od) == K.padded_cols(9, od) and _fovlib().crnn_fov_padded_cols(7, od) == K.padded_cols(7, od)
    assert _ops().crnn_conv9_backward_parts(16) == UNSUPPORTED and _ops().crnn_front_padded_cols(16) == UNSUPPORTED
