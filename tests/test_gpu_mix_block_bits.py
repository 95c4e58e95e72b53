"""The mixing + TD block of the QMIX learn (marl_dmfb_amd/csrc/qmix_ops.hip) through its C ABI, every output word against what the
library gave BEFORE its entry points were folded into one launch path and its selector and the shared pieces of its lambda walk
moved into the header it shares with vdn_ops.hip (csrc/td_rules.h; the per-agent pick stays in the kernel): mtd, mask, the two
q_tot arrays, targets, picks, the bad-action counter, and grad_q, grad_p, Z and X of the backward must keep their bits.  The float64
tests hold these values only within a tolerance; the weights of a learn follow every bit.

tests/golden/mix_block_bits.npz holds only the recorded outputs (tools/record_mix_block_fixture.py, run on an MI355X with the library
of the commit before the change); the inputs are regenerated here, on the host, from the seeds of tests/qmix_kernel_cases.py and of
the kernel tests whose case builders this module borrows.  An array above 16 kB is recorded as one 8-byte blake2b digest per output
row, so a mismatch still names the row.  NaN words are compared by position: every NaN is written as 0x7fc00000 before the compare.

  rows, padded    qmix_mix_td_forward + _backward: one row; 33 rows (a second workgroup with one row); n = 1 with A = 1, n = 16 with
                  A = 16, n = 3 with A = 5; both H; the sep and the ring P layout
  rows, packed    qmix_mix_td_forward_packed + _backward_packed on the valid units of the same draws, step-major, with d_p_target_row
                  given and NULL, and on an unsorted unit list with repeats; grad_q with rows_pad = U*n and U*n rounded up to 64
  lambda          qmix_mix_td_lambda_forward and _packed at lambda 0, 0.5 and 0.8: B 1 x T 1; B 5 (two workgroups, idle waves);
                  T 65 (a lane takes a second step); T 512 at B 2, n 1
  double-Q        qmix_mix_td_double_forward and _packed at lambda 0 and 0.8: d_sel_units NULL; given, with one unit outside
                  [0, n_sel_units) (its row falls back to its own target rows, its picks read -1); d_picks and d_targets NULL and given
  bad actions     one case per family, three actions outside [0, A) placed by seed: the NaN positions, the bits everywhere else and
                  the counter"""
import ctypes as C
import functools
import hashlib
import os
import re

import numpy as np
import pytest
import torch

import qmix_kernel_cases as K
import test_gpu_qmix_double_kernels as DK
import test_gpu_qmix_kernels as P
import test_gpu_qmix_lambda_kernels as LK
import test_gpu_qmix_packed_kernels as PK

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mix_block_bits.npz')
DIGEST_ABOVE = 16384                     # bytes
# (B, T, n, H, A, layout)
ROW_COMBOS = [(1, 1, 1, 24, 1, 'ring'), (3, 11, 16, 32, 16, 'sep'), (3, 11, 3, 24, 5, 'ring'), (33, 1, 3, 32, 5, 'sep')]
PACKED_HOW = [(0, 'rows'), (1, 'rows'), (1, 'gathered'), (2, 'rows'), (2, 'gathered'), (2, 'loose'), (3, 'rows')]   # (combo, how)
LOOSE_UNITS = 45                         # two workgroups of units drawn with repeats from all 33 rows of ROW_COMBOS[2]
LAMBDA_COMBOS = [(1, 1, 1, 24, 1, 'ring'), (5, 7, 4, 32, 5, 'ring'), (2, 65, 3, 24, 5, 'sep'), (2, 512, 1, 24, 3, 'sep')]
LAMBDAS = [0.0, 0.5, 0.8]
DOUBLE_COMBOS = [(5, 7, 4, 32, 5, 'ring'), (3, 11, 16, 24, 16, 'sep')]
DOUBLE_LAMBDAS = [0.0, 0.8]
DOUBLE_PADDED, DOUBLE_PACKED = ('full', 'bare'), ('null', 'outside', 'bare')
OUTSIDE_UNIT = 5                         # the unit whose d_sel_units entry is n_sel_units
BAD_ROWS, BAD_LAMBDA, BAD_DOUBLE = ROW_COMBOS[2], (LAMBDA_COMBOS[1], 0.8), (DOUBLE_COMBOS[0], 0.8, 0.0)
_ID = lambda s: 'x'.join(map(str, s))   # noqa: E731


def _poison(c, seed):
    """Three actions outside [0, A) in three valid rows of the case, placed by seed."""
    g = np.random.default_rng(seed)
    valid = np.argwhere(c.padded[:, :c.T, 0].numpy() == 0)
    for (b, t), v in zip(valid[g.choice(len(valid), 3, replace=False)], (c.A, -1, 127)):
        c.u[int(b), int(t), int(g.integers(0, c.n)), 0] = v
    return c


def _np(**arrays):
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}


def run_rows_padded(combo, bad=False):
    """-> mtd, mask [B*T], grad_q [T*B][n*A], grad_p [B*p_rows][F] (0 in the rows no step owns), Z, X [B*T][..], bad [1]"""
    c = K.make_case(*combo, 'real', seed=K.SEEDS.get((combo, 'real'), 0))
    if bad:
        _poison(c, 41)
    o = P._run(c)
    return _np(mtd=o.mtd, mask=o.mask, grad_q=o.grad_q.reshape(c.T * c.B, -1), grad_p=o.grad_p.reshape(c.B * c.pe_rows, -1), Z=o.Z, X=o.X,
               bad=np.array([o.bad], np.int32))


def run_rows_packed(combo, how, bad=False):
    """-> mtd, mask [U], grad_q [rows_pad][A] at rows_pad = U*n rounded up to 64, grad_p, Z, X [U][..], bad [1]; grad_q at
    rows_pad = U*n must be its first U*n rows and leave the rest alone (asserted here, so also when the record is made)."""
    c = K.make_case(*combo, 'real', seed=K.SEEDS.get((combo, 'real'), 0))
    if bad:
        _poison(c, 43)
    d = P._to_gpu(c)
    if how == 'loose':
        g = np.random.default_rng(47)
        bt = [(int(r // c.T), int(r % c.T)) for r in g.integers(0, c.R, LOOSE_UNITS)]
        assert len(set(bt)) < len(bt) and bt != sorted(bt)
    else:
        bt = PK._units(c)
    k = PK._pack(c, d, bt, 'gathered' if how == 'gathered' else 'rows')
    assert (k.trow is None) == (how == 'gathered')
    o = PK._run_packed(c, d, k)
    rows = k.U * c.n
    gq = torch.cat([o.grad_q.reshape(rows, c.A), o.tail.reshape(-1, c.A)])
    assert gq.shape == (k.rows_pad, c.A) and not o.tail.view(torch.int32).any(), 'the tail behind the last unit is not +0'
    # the same backward with rows_pad = U*n
    mtd, mask, gnum = P._put(o.mtd)[0], P._put(o.mask)[0], P._put(torch.tensor([c.g0]))[0]
    tight = P._out(d, (k.rows_pad, c.A))
    gp, Z, X = P._out(d, (k.U, K.f_cols(c.H))), P._out(d, (k.U, K.z_cols(c.n))), P._out(d, (k.U, K.x_cols(c.H)))
    p = P._p
    rc = P._lib().qmix_packed().qmix_mix_td_backward_packed(p(mtd), p(mask), p(k.q_e), p(k.units), k.U, p(d.u), c.n, c.A, rows, p(k.pe), c.H,
                                                            K.M, C.byref(d.mix_e), p(gnum), p(tight), p(gp), p(Z), p(X), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for chk in d.checks:
        chk()
    tight = tight.cpu()
    assert bool((tight[rows:] == P.SENT).all()), 'rows_pad = U*n wrote behind its last row'
    same = tight[:rows].view(torch.int32) == gq[:rows].view(torch.int32)
    assert bool((same | (tight[:rows].isnan() & gq[:rows].isnan())).all()), 'rows_pad changes the rows of the units'
    for name, t in (('grad_p', gp), ('Z', Z), ('X', X)):
        a, b = t.cpu(), getattr(o, name)
        assert bool(((a.view(torch.int32) == b.view(torch.int32)) | (a.isnan() & b.isnan())).all()), name
    return _np(mtd=o.mtd, mask=o.mask, grad_q=gq, grad_p=o.grad_p, Z=o.Z, X=o.X, bad=np.array([o.bad], np.int32))


def run_lambda(combo, lam, packed, bad=False):
    """-> mtd, mask, targets, tot_e, tot_t [B*T] or [U], bad [1]"""
    c = LK._case(combo, 'real')
    if bad:
        _poison(c, 53)
    d = P._to_gpu(c)
    o = LK._call_packed(c, d, PK._pack(c, d, PK._units(c)), lam) if packed else LK._call_padded(c, d, lam)
    assert o.rc == 0, o.rc
    return _np(mtd=o.mtd, mask=o.mask, targets=o.tgt, tot_e=o.tot_e, tot_t=o.tot_t, bad=o.cnt)


def run_double(combo, lam, form, bad=False):
    """form: 'padded_full' / 'padded_bare' / 'packed_null' / 'packed_outside' / 'packed_bare' (module docstring); an output that the
    call leaves alone (the q_tot at lambda 0, picks and targets where NULL) is recorded with its fill.
    -> mtd, mask, targets, tot_e, tot_t [rows], picks [rows][n], bad [1]"""
    c = DK._case(combo)
    if bad:
        _poison(c, 59)
    d = P._to_gpu(c)
    bare = form.endswith('_bare')
    over = dict(tgt=None) if bare else {}
    if form.startswith('padded'):
        o = DK._double_padded(c, d, lam, DK._put(d, c.q_sel), picks=not bare, **over)
    else:
        k = PK._pack(c, d, PK._units(c))
        psel, n_sel, sel_units, own = DK._packed_selector(c, d, PK._units(c))
        if form == 'packed_null':
            o = DK._double_packed(c, d, k, lam, DK._put(d, own.contiguous()), k.U, None)
        else:
            if form == 'packed_outside':
                units = sel_units.cpu().clone()
                units[OUTSIDE_UNIT] = n_sel
                sel_units = DK._put(d, units)
            o = DK._double_packed(c, d, k, lam, psel, n_sel, sel_units, picks=not bare, **over)
    assert o.rc == 0, o.rc
    return _np(mtd=o.mtd, mask=o.mask, targets=o.tgt, tot_e=o.tot_e, tot_t=o.tot_t, picks=o.picks, bad=o.cnt)


ROW_FIELDS = ('mtd', 'mask', 'grad_q', 'grad_p', 'Z', 'X', 'bad')
LAMBDA_FIELDS = ('mtd', 'mask', 'targets', 'tot_e', 'tot_t', 'bad')
DOUBLE_FIELDS = LAMBDA_FIELDS + ('picks',)


def fields(key):
    return ROW_FIELDS if key.startswith('rows_') else LAMBDA_FIELDS if key.startswith('lambda_') else DOUBLE_FIELDS


def rows_key(form, combo, bad=False):
    return 'rows_%s_%s%s' % (form, _ID(combo), '_bad' if bad else '')


def lambda_key(form, combo, lam, bad=False):
    return 'lambda_%s_%s_lam%g%s' % (form, _ID(combo), lam, '_bad' if bad else '')


def double_key(form, combo, lam, bad=False):
    return 'double_%s_%s_lam%g%s' % (form, _ID(combo), lam, '_bad' if bad else '')


def all_runs():
    """key -> a call that gives the case's outputs: every case of the record, the order of the file."""
    part = functools.partial
    runs = {}
    for c in ROW_COMBOS:
        runs[rows_key('padded', c)] = part(run_rows_padded, c)
    for i, how in PACKED_HOW:
        runs[rows_key('packed_' + how, ROW_COMBOS[i])] = part(run_rows_packed, ROW_COMBOS[i], how)
    for c in LAMBDA_COMBOS:
        for lam in LAMBDAS:
            for packed in (False, True):
                runs[lambda_key('packed' if packed else 'padded', c, lam)] = part(run_lambda, c, lam, packed)
    for c in DOUBLE_COMBOS:
        for lam in DOUBLE_LAMBDAS:
            for form in ['padded_' + v for v in DOUBLE_PADDED] + ['packed_' + v for v in DOUBLE_PACKED]:
                runs[double_key(form, c, lam)] = part(run_double, c, lam, form)
    runs[rows_key('padded', BAD_ROWS, True)] = part(run_rows_padded, BAD_ROWS, True)
    runs[rows_key('packed_rows', BAD_ROWS, True)] = part(run_rows_packed, BAD_ROWS, 'rows', True)
    for packed in (False, True):
        runs[lambda_key('packed' if packed else 'padded', *BAD_LAMBDA, True)] = part(run_lambda, *BAD_LAMBDA, packed, True)
    runs[double_key('padded_full', BAD_DOUBLE[0], BAD_DOUBLE[1], True)] = part(run_double, BAD_DOUBLE[0], BAD_DOUBLE[1], 'padded_full', True)
    runs[double_key('packed_null', BAD_DOUBLE[0], BAD_DOUBLE[2], True)] = part(run_double, BAD_DOUBLE[0], BAD_DOUBLE[2], 'packed_null', True)
    return runs


def expected_bad(key):
    """What the counter of a case must read."""
    return 3 if key.endswith('_bad') else 1 if '_outside_' in key else 0


def words(a):
    """The array as it is recorded and compared: every NaN as 0x7fc00000; above DIGEST_ABOVE bytes one digest per output row."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        a = np.where(np.isnan(a), np.float32(np.nan), a).view(np.uint32)
    if a.nbytes <= DIGEST_ABOVE:
        return a
    assert a.ndim == 2, a.shape
    return np.array([int.from_bytes(hashlib.blake2b(row.tobytes(), digest_size=8).digest(), 'little') for row in a], np.uint64)


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _same_bits(key, got):
    g = _golden()
    assert int(got['bad'][0]) == expected_bad(key), (key, 'counter', int(got['bad'][0]))
    for f in fields(key):
        want, have = g[key + '.' + f], words(got[f])      # a key that the record lacks is a KeyError: a failure, never a skip
        assert have.dtype == want.dtype and have.shape == want.shape, (key, f, have.dtype, have.shape, want.dtype, want.shape)
        wrong = np.flatnonzero((have != want).reshape(len(have), -1).any(1))
        print('%s.%s: %d of %d %s with other bits' % (key, f, len(wrong), len(have), 'row digests' if have.dtype == np.uint64 else 'rows'))
        if len(wrong):
            i = int(wrong[0])
            raise AssertionError('%s.%s: %d of %d rows differ from the record, first at row %d: got %r, recorded %r' % (
                key, f, len(wrong), len(have), i, have[i], want[i]))


def test_the_record_holds_every_case():
    g = _golden()
    runs = all_runs()
    assert sorted(g) == sorted(k + '.' + f for k in runs for f in fields(k))
    assert os.path.getsize(GOLDEN) < 400 * 1024
    nan = np.uint32(0x7fc00000)
    for k in runs:
        assert int(g[k + '.bad'][0]) == expected_bad(k), k
        assert g[k + '.mtd'].dtype == np.uint32 and int((g[k + '.mtd'] == nan).sum()) == expected_bad(k), k
        assert set(np.unique(g[k + '.mask'])) <= {0, 0x3f800000}, k
        if k.startswith('lambda_') or (k.startswith('double_') and float(re.search(r'_lam([0-9.]+)', k).group(1)) > 0):
            assert int((g[k + '.tot_e'] == nan).sum()) == expected_bad(k) and not (g[k + '.tot_t'] == nan).any(), k
    for c in ROW_COMBOS:
        B, T, n, H, A, _ = c
        assert g[rows_key('padded', c) + '.mtd'].shape == (B * T,)
        for f, width in (('grad_q', n * A), ('Z', K.z_cols(n)), ('X', K.x_cols(H))):
            a = g[rows_key('padded', c) + '.' + f]
            assert a.shape == ((B * T, width) if B * T * width * 4 <= DIGEST_ABOVE else (B * T,)), (c, f, a.shape)
    assert {g[k + '.Z'].dtype for k in runs if k.startswith('rows_')} == {np.dtype(np.uint32), np.dtype(np.uint64)}
    k = double_key('packed_outside', DOUBLE_COMBOS[0], 0.0)
    assert (g[k + '.picks'][OUTSIDE_UNIT] == -1).all() and int((g[k + '.picks'] == -1).sum()) == DOUBLE_COMBOS[0][2]
    k = double_key('packed_bare', DOUBLE_COMBOS[0], 0.0)
    assert (g[k + '.picks'] == DK.PICK_SENT).all() and (g[k + '.targets'].view(np.float32) == P.SENT).all()
    assert (g[k + '.tot_e'].view(np.float32) == P.SENT).all()          # the hand-off is not written at lambda 0


def _keys(prefix, bad=False):
    return [k for k in all_runs() if k.startswith(prefix) and k.endswith('_bad') == bad]


@pytest.mark.gpu
@pytest.mark.parametrize('key', _keys('rows_padded'))
def test_padded_rows_bits_of_the_build_before(key):
    _same_bits(key, all_runs()[key]())


@pytest.mark.gpu
@pytest.mark.parametrize('key', _keys('rows_packed'))
def test_packed_rows_bits_of_the_build_before(key):
    _same_bits(key, all_runs()[key]())


@pytest.mark.gpu
@pytest.mark.parametrize('key', _keys('lambda_'))
def test_lambda_bits_of_the_build_before(key):
    _same_bits(key, all_runs()[key]())


@pytest.mark.gpu
@pytest.mark.parametrize('key', _keys('double_'))
def test_double_q_bits_of_the_build_before(key):
    _same_bits(key, all_runs()[key]())


@pytest.mark.gpu
def test_bad_action_bits_of_the_build_before():
    """One case per family: NaN where it was recorded and nowhere else, every other word and the counter as recorded."""
    keys = _keys('', bad=True)
    assert len(keys) == 6
    for key in keys:
        _same_bits(key, all_runs()[key]())
