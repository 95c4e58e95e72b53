"""The TD block of the VDN learn (marl_dmfb_amd/csrc/vdn_ops.hip) through its C ABI, every output word against what the library gave
BEFORE its one-step and lambda kernels were folded into one row rule and one index-rule pair: mtd, mask, the (num, mask_sum) pair,
the lambda targets and grad_q must keep their bits.  The float64 tests hold the one-step mtd only within a tolerance and the sums
only within their roundings; the weights of a learn follow both.

tests/golden/td_block_bits.npz holds only the recorded outputs (tools/record_td_block_fixture.py, run on an MI355X with the library
of the commit before the change); the inputs are regenerated here, on the host, from the seeds below: episodes longest first, about
30 % of the steps padded as an episode tail, about 20 % terminated, one agent row in ten with no available action, *d_grad_num 0.37.

  one-step padded   vdn_td_forward_sums + vdn_td_backward: one slot; odd sizes; 333 slots (two workgroups, the second partial);
                    16 510 slots (65 workgroups: the last one's lane-strided walk over the partials takes a second trip); A = 127
  one-step packed   vdn_td_forward_packed_sums + vdn_td_backward_packed_pad on the valid units of the same draws, step-major, and on
                    an unsorted unit list with repeats; grad_q with rows_pad = U*n and U*n rounded up to 64 (the zero tail)
  lambda            vdn_td_lambda_forward_sums and ..._packed_sums at lambda 0.5 and 0.8: one slot; two workgroups with idle waves;
                    65 steps (a lane takes a second step); VDN_LAMBDA_MAX_T
  bad actions       one case per family, three actions outside [0, A) placed by seed: the NaN positions, the bits everywhere else
                    and the counter"""
import ctypes as C
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

DEV = 'cuda'
GAMMA = 0.99
GRAD_NUM = 0.37
# (B, T, t_limit, n, A)
STEP_SHAPES = [(1, 1, 1, 1, 2), (5, 7, 9, 3, 5), (37, 9, 12, 2, 7), (130, 127, 130, 1, 3), (3, 5, 8, 4, 127)]
LOOSE = (3, 5, 700)                       # (n, A, U): an unsorted unit list with repeats over the slots of LOOSE_REPLAY
LOOSE_REPLAY = (37, 12)                   # (B, t_limit)
LAMBDA_SHAPES = [(1, 1, 1, 1, 2), (5, 7, 40, 4, 5), (3, 65, 70, 2, 5), (2, 512, 512, 1, 3)]
LAMBDAS = [0.5, 0.8]
BAD_STEP_SHAPE, BAD_LAMBDA_SHAPE, BAD_LAMBDA = (5, 7, 9, 3, 5), (5, 7, 40, 4, 5), 0.8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'td_block_bits.npz')
_ID = lambda s: 'x'.join(map(str, s))   # noqa: E731


def _p(t):
    return C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def case(shape, bad=False):
    """Host inputs of one shape in the layouts of include/vdn_ops.h.  bad: three actions outside [0, A) on valid steps."""
    B, T, Tl, n, A = shape
    g = np.random.default_rng(730000 + 1000 * B + 10 * T + A + (5 if bad else 0))
    c = SimpleNamespace(B=B, T=T, Tl=Tl, n=n, A=A)
    lens = g.integers((2 * T + 4) // 5, T + 1, B)           # 0.4 T .. T: about 30 % of the steps are an episode's padded tail
    lens[0] = T
    c.lens = np.sort(lens)[::-1].copy()
    c.padded = (np.arange(Tl)[None, :] >= c.lens[:, None]).astype(np.uint8)
    c.term = (g.random((B, Tl)) < 0.2).astype(np.uint8)
    c.r = g.standard_normal((B, Tl)).astype(np.float32)
    c.u = g.integers(0, A, (B, Tl, n)).astype(np.int8)
    c.avail = (g.random((B, Tl, n, A)) < 0.7).astype(np.int8)
    c.avail[g.random((B, Tl, n)) > 0.9] = 0
    c.qe = g.standard_normal((T, B, n, A)).astype(np.float32)
    c.qt = (g.standard_normal((T, B, n, A)) * 2).astype(np.float32)
    if bad:
        for v in (A, -1, 127):
            b = int(g.integers(0, B))
            c.u[b, int(g.integers(0, c.lens[b])), int(g.integers(0, n))] = v
    # the packed form: the valid units step after step, unit j with the Q rows of its (episode, step)
    c.counts = (c.lens[None, :] > np.arange(T)[:, None]).sum(1).astype(np.int32)
    bt = [(b, t) for t, k in enumerate(c.counts) for b in range(k)]
    c.units = np.array([b * Tl + t for b, t in bt], np.int32)
    rows = np.array([t * B + b for b, t in bt], np.int64)
    c.qe_packed, c.qt_packed = c.qe.reshape(T * B, n, A)[rows], c.qt.reshape(T * B, n, A)[rows]
    return c


@functools.lru_cache(maxsize=None)
def loose_case():
    n, A, U = LOOSE
    B, Tl = LOOSE_REPLAY
    g = np.random.default_rng(739000)
    c = SimpleNamespace(B=B, T=Tl, Tl=Tl, n=n, A=A)
    c.padded = (g.random((B, Tl)) < 0.3).astype(np.uint8)
    c.term = (g.random((B, Tl)) < 0.2).astype(np.uint8)
    c.r = g.standard_normal((B, Tl)).astype(np.float32)
    c.u = g.integers(0, A, (B, Tl, n)).astype(np.int8)
    c.avail = (g.random((B, Tl, n, A)) < 0.7).astype(np.int8)
    c.avail[g.random((B, Tl, n)) > 0.9] = 0
    c.units = g.integers(0, B * Tl, U).astype(np.int32)
    c.qe_packed = g.standard_normal((U, n, A)).astype(np.float32)
    c.qt_packed = (g.standard_normal((U, n, A)) * 2).astype(np.float32)
    return c


def _dev(c, *names):
    return SimpleNamespace(**{k: torch.from_numpy(np.ascontiguousarray(getattr(c, k))).to(DEV) for k in names})


def _outs(lib_parts, k):
    nan = float('nan')
    return SimpleNamespace(mtd=torch.full((k,), nan, device=DEV), mask=torch.full((k,), nan, device=DEV), tgt=torch.full((k,), nan, device=DEV),
                           sums=torch.full((2,), nan, device=DEV), part=torch.full((lib_parts,), nan, device=DEV),
                           cnt=torch.zeros(1, dtype=torch.int32, device=DEV), g=torch.tensor([GRAD_NUM], device=DEV))


def _record(o, **more):
    torch.cuda.synchronize()
    rec = dict(mtd=o.mtd, mask=o.mask, sums=o.sums, **more)
    rec = {k: v.cpu().numpy() for k, v in rec.items()}
    rec['bad'] = o.cnt.cpu().numpy()
    return rec


def run_step_padded(shape, bad=False):
    """-> mtd, mask [B*T], sums [2], grad_q [T*B*n*A], bad [1]"""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_tail()
    c = case(shape, bad)
    d = _dev(c, 'qe', 'qt', 'u', 'r', 'avail', 'term', 'padded')
    o = _outs(lib.vdn_td_sum_parts(c.B * c.T), c.B * c.T)
    gq = torch.full((c.T * c.B * c.n * c.A,), float('nan'), device=DEV)
    rc = lib.vdn_td_forward_sums(_p(d.qe), _p(d.qt), _p(d.u), _p(d.r), _p(d.avail), _p(d.term), _p(d.padded), c.B, c.T, c.Tl, c.n, c.A, GAMMA,
                                 _p(o.mtd), _p(o.mask), _p(o.cnt), _p(o.part), _p(o.sums), None)
    assert rc == 0, rc
    rc = _lib.vdn_ops().vdn_td_backward(_p(o.mtd), _p(o.mask), _p(d.u), _p(o.g), c.B, c.T, c.Tl, c.n, c.A, _p(gq), None)
    assert rc == 0, rc
    return _record(o, grad_q=gq)


def run_step_packed(shape, bad=False):
    """shape None: the unsorted list.  -> mtd, mask [U], sums [2], grad_q [rows_pad*A] at rows_pad = U*n rounded up to 64, bad [1];
    grad_q at rows_pad = U*n must be its first U*n rows (asserted here, so also when the record is made)."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_tail()
    c = loose_case() if shape is None else case(shape, bad)
    d = _dev(c, 'qe_packed', 'qt_packed', 'units', 'u', 'r', 'avail', 'term', 'padded')
    U = len(c.units)
    o = _outs(lib.vdn_td_sum_parts(U), U)
    rc = lib.vdn_td_forward_packed_sums(_p(d.qe_packed), _p(d.qt_packed), _p(d.units), U, _p(d.u), _p(d.r), _p(d.avail), _p(d.term), _p(d.padded),
                                        c.n, c.A, GAMMA, _p(o.mtd), _p(o.mask), _p(o.cnt), _p(o.part), _p(o.sums), None)
    assert rc == 0, rc
    rows = U * c.n
    rows_pad = (rows + 63) // 64 * 64
    gq = torch.full((rows_pad * c.A,), float('nan'), device=DEV)
    tight = torch.full((rows_pad * c.A,), float('nan'), device=DEV)
    for buf, rp in ((gq, rows_pad), (tight, rows)):
        rc = lib.vdn_td_backward_packed_pad(_p(o.mtd), _p(o.mask), _p(d.units), U, _p(d.u), _p(o.g), c.n, c.A, rp, _p(buf), None)
        assert rc == 0, rc
    rec = _record(o, grad_q=gq)
    tight = tight.cpu().numpy()
    assert np.isnan(tight[rows * c.A:]).all(), 'rows_pad = U*n wrote behind its last row'
    assert np.array_equal(tight[:rows * c.A].view(np.int32), rec['grad_q'][:rows * c.A].view(np.int32)), 'rows_pad changes the rows of the units'
    assert not rec['grad_q'][rows * c.A:].view(np.int32).any(), 'the tail behind the last unit is not +0'
    return rec


def run_lambda(shape, lam, packed, bad=False):
    """-> mtd, mask, targets [B*T] or [U], sums [2], bad [1]"""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_lambda()
    c = case(shape, bad)
    if packed:
        d = _dev(c, 'qe_packed', 'qt_packed', 'units', 'u', 'r', 'avail', 'term', 'padded')
        U = len(c.units)
        o = _outs(lib.vdn_td_lambda_sum_parts(int(c.counts[0])), U)
        rc = lib.vdn_td_lambda_forward_packed_sums(_p(d.qe_packed), _p(d.qt_packed), _p(d.units), U, _p(d.u), _p(d.r), _p(d.avail), _p(d.term),
                                                   _p(d.padded), c.n, c.A, GAMMA, _p(o.mtd), _p(o.mask), _p(o.cnt), _p(o.part), _p(o.sums), lam,
                                                   _p(o.tgt), len(c.counts), (C.c_int32 * len(c.counts))(*[int(k) for k in c.counts]), None)
    else:
        d = _dev(c, 'qe', 'qt', 'u', 'r', 'avail', 'term', 'padded')
        o = _outs(lib.vdn_td_lambda_sum_parts(c.B), c.B * c.T)
        rc = lib.vdn_td_lambda_forward_sums(_p(d.qe), _p(d.qt), _p(d.u), _p(d.r), _p(d.avail), _p(d.term), _p(d.padded), c.B, c.T, c.Tl, c.n, c.A,
                                            GAMMA, _p(o.mtd), _p(o.mask), _p(o.cnt), _p(o.part), _p(o.sums), lam, _p(o.tgt), None)
    assert rc == 0, rc
    return _record(o, targets=o.tgt)


def step_key(form, shape, bad=False):
    return 'step_%s_%s%s' % (form, 'loose' if shape is None else _ID(shape), '_bad' if bad else '')


def lambda_key(form, shape, lam, bad=False):
    return 'lambda_%s_%s_lam%g%s' % (form, _ID(shape), lam, '_bad' if bad else '')


def all_runs():
    """key -> a call that gives the case's outputs: every case of the record, the order of the file."""
    runs = {}
    for s in STEP_SHAPES:
        runs[step_key('padded', s)] = functools.partial(run_step_padded, s)
    for s in STEP_SHAPES + [None]:
        runs[step_key('packed', s)] = functools.partial(run_step_packed, s)
    for s in LAMBDA_SHAPES:
        for lam in LAMBDAS:
            for packed in (False, True):
                runs[lambda_key('packed' if packed else 'padded', s, lam)] = functools.partial(run_lambda, s, lam, packed)
    runs[step_key('padded', BAD_STEP_SHAPE, True)] = functools.partial(run_step_padded, BAD_STEP_SHAPE, True)
    runs[step_key('packed', BAD_STEP_SHAPE, True)] = functools.partial(run_step_packed, BAD_STEP_SHAPE, True)
    for packed in (False, True):
        runs[lambda_key('packed' if packed else 'padded', BAD_LAMBDA_SHAPE, BAD_LAMBDA, True)] = functools.partial(
            run_lambda, BAD_LAMBDA_SHAPE, BAD_LAMBDA, packed, True)
    return runs


def fields(key):
    return ('mtd', 'mask', 'sums', 'bad') + (('grad_q',) if key.startswith('step_') else ('targets',))


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _same_bits(key, got):
    """Every field of the case against the record: the same NaN positions (a bad-action case only) and the same bits elsewhere."""
    g = _golden()
    for f in fields(key):
        want, have = g[key + '.' + f], got[f]            # a key that the record lacks is a KeyError: a failure, never a skip
        assert have.dtype == want.dtype and have.shape == want.shape, (key, f, have.dtype, have.shape, want.dtype, want.shape)
        if f == 'bad':
            assert int(have[0]) == int(want[0]), (key, 'counter', int(have[0]), int(want[0]))
            continue
        nan_w, nan_h = np.isnan(want), np.isnan(have)
        assert key.endswith('_bad') or not nan_w.any(), 'the record of %s.%s holds NaN' % (key, f)
        assert np.array_equal(nan_h, nan_w), '%s.%s: NaN at other positions than recorded' % (key, f)
        wrong = np.flatnonzero((have.view(np.int32) != want.view(np.int32)) & ~nan_w)
        print('%s.%s: %d of %d words with other bits' % (key, f, len(wrong), have.size))
        if len(wrong):
            i = int(wrong[0])
            raise AssertionError('%s.%s: %d of %d words differ from the record, first at %d: got %r (0x%08x), recorded %r (0x%08x)' % (
                key, f, len(wrong), have.size, i, have[i], have.view(np.uint32)[i], want[i], want.view(np.uint32)[i]))


def test_the_record_holds_every_case():
    g = _golden()
    runs = all_runs()
    assert sorted(g) == sorted(k + '.' + f for k in runs for f in fields(k))
    for s in STEP_SHAPES:
        B, T, _, n, A = s
        U = int(case(s).lens.sum())
        assert g[step_key('padded', s) + '.mtd'].shape == (B * T,) and g[step_key('padded', s) + '.grad_q'].shape == (T * B * n * A,)
        assert g[step_key('packed', s) + '.mtd'].shape == (U,) and g[step_key('packed', s) + '.grad_q'].shape == ((U * n + 63) // 64 * 64 * A,)
    for k in runs:
        bad = int(g[k + '.bad'][0])
        assert (bad > 0) == k.endswith('_bad'), k
        assert np.isnan(g[k + '.sums'][0]) == k.endswith('_bad') and np.isnan(g[k + '.mtd']).sum() == bad, k
        assert float(g[k + '.sums'][1]) == float(g[k + '.mask'].sum()) > 0, k
    # 16 510 slots: about 30 % padded
    assert 0.2 < 1.0 - float(g[step_key('padded', STEP_SHAPES[3]) + '.mask'].mean()) < 0.4


@pytest.mark.gpu
@pytest.mark.parametrize('shape', STEP_SHAPES, ids=_ID)
def test_one_step_padded_bits_of_the_build_before(shape):
    _same_bits(step_key('padded', shape), run_step_padded(shape))


@pytest.mark.gpu
@pytest.mark.parametrize('shape', STEP_SHAPES + [None], ids=lambda s: 'loose' if s is None else _ID(s))
def test_one_step_packed_bits_of_the_build_before(shape):
    _same_bits(step_key('packed', shape), run_step_packed(shape))


@pytest.mark.gpu
@pytest.mark.parametrize('packed', [False, True], ids=['padded', 'packed'])
@pytest.mark.parametrize('lam', LAMBDAS)
@pytest.mark.parametrize('shape', LAMBDA_SHAPES, ids=_ID)
def test_lambda_bits_of_the_build_before(shape, lam, packed):
    _same_bits(lambda_key('packed' if packed else 'padded', shape, lam), run_lambda(shape, lam, packed))


@pytest.mark.gpu
def test_bad_action_bits_of_the_build_before():
    """One case per family: NaN where it was recorded and nowhere else, every other word and the counter as recorded."""
    for key, run in all_runs().items():
        if key.endswith('_bad'):
            _same_bits(key, run())
