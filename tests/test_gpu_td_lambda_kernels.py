"""The TD block on lambda-returns through its C ABI (include/vdn_lambda.h: vdn_td_lambda_forward_sums and
vdn_td_lambda_forward_packed_sums), every output slot against the float32 numpy statement of the rule
(marl_dmfb_amd.policy.td_lambda.lambda_targets_reference) BIT FOR BIT: the kernels do the same float32 operations in the same order
(the library is built with -ffp-contract=off), so nothing is left to a tolerance but the two scalar sums.

Every case holds an episode of length 1, one of length T and lengths between (longest first, as the packed form wants them), one
episode whose last valid step is not terminated, one terminated in mid-episode with valid steps behind it, agent rows with a single
available action and rows with none; rewards, Q values and flags of the padded slots are random, so a padded slot that leaked into a
valid one would show."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from marl_dmfb_amd.policy.td_lambda import lambda_targets_reference

pytestmark = pytest.mark.gpu

GAMMA = 0.99
SENT = -777.25          # what every output buffer holds before a call
GUARD = 16              # words behind every output
BAD_ARG = -1
U24 = 2.0 ** -24
# (B, T, t_limit, n, A): one slot; two steps; the default task; more episodes than one workgroup of four and a partial last one; the
# widest action set; the packed learn's step limit; VDN_LAMBDA_MAX_T (padded form only: a packed learn has at most 255 steps)
SHAPES = [(1, 1, 1, 1, 2), (3, 2, 5, 1, 5), (5, 7, 40, 4, 5), (70, 40, 40, 4, 5), (3, 5, 8, 4, 127), (9, 255, 255, 3, 9),
          (2, 512, 512, 2, 5)]
PACKED_MAX_T = 255
LAMBDAS = [0.0, 0.5, 0.8, 1.0]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _lens(B, T, rng):
    if B == 1:
        return np.array([T])
    if B == 2:
        return np.array([T, 1])
    mid = max(min(T, 2), (T + 1) // 2)            # one episode long enough to terminate in its middle (where T allows)
    lens = np.concatenate([[T, mid], rng.integers(1, T + 1, B - 3), [1]])
    return np.sort(lens)[::-1].copy()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """The inputs of one shape as numpy arrays in the layouts of include/vdn_ops.h, and what the rule needs of them: Q' and e per
    (episode, step), formed as k_td_forward forms them (agents added in index order, float32)."""
    B, T, Tl, n, A = shape
    rng = np.random.default_rng(1000 * B + T)
    c = SimpleNamespace(shape=shape, B=B, T=T, Tl=Tl, n=n, A=A)
    c.lens = _lens(B, T, rng)
    steps = np.arange(Tl)[None, :]
    c.padded = (steps >= c.lens[:, None]).astype(np.uint8)
    c.term = (rng.random((B, Tl)) < 0.5).astype(np.uint8)
    c.term[c.padded == 0] = 0
    c.term[np.arange(B), c.lens - 1] = 1                       # the last valid step terminates ...
    c.term[0, c.lens[0] - 1] = 0                               # ... but for the longest episode, which runs into the batch's end
    if B > 1 and c.lens[1] >= 3:
        c.term[1, c.lens[1] // 2 - 1] = 1                      # terminated in mid-episode, valid steps behind it
    c.r = rng.standard_normal((B, Tl)).astype(np.float32)
    c.u = rng.integers(0, A, (B, Tl, n)).astype(np.int8)
    c.avail = (rng.random((B, Tl, n, A)) < 0.7).astype(np.int8)
    kind = rng.random((B, Tl, n))
    single = kind < 0.15                                       # rows with one available action, rows with none
    c.avail[single] = 0
    c.avail[single, rng.integers(0, A, int(single.sum()))] = 1
    c.avail[kind > 0.9] = 0
    c.qe = rng.standard_normal((T, B, n, A)).astype(np.float32)
    c.qt = (rng.standard_normal((T, B, n, A)) * 2).astype(np.float32)
    qe_bt, qt_bt = c.qe.transpose(1, 0, 2, 3), c.qt.transpose(1, 0, 2, 3)                   # (B, T, n, A)
    taken = np.take_along_axis(qe_bt, c.u[:, :T, :, None].astype(np.int64), axis=3)[..., 0]
    best = np.where(c.avail[:, :T] == 0, np.float32(-9999999.0), qt_bt).max(axis=3)
    c.e, c.q_next = np.zeros((B, T), np.float32), np.zeros((B, T), np.float32)
    for i in range(n):
        c.e = c.e + taken[:, :, i]
        c.q_next = c.q_next + best[:, :, i]
    assert c.e.dtype == np.float32 and c.q_next.dtype == np.float32
    # the packed form of the same episodes: units step after step, the Q rows of unit j those of its (episode, step)
    c.counts = (c.lens[None, :] > np.arange(int(c.lens[0]))[:, None]).sum(1).astype(np.int32)
    c.unit_bt = [(b, t) for t, k in enumerate(c.counts) for b in range(k)]
    c.units = np.array([b * Tl + t for b, t in c.unit_bt], np.int32)
    assert c.lens[0] == T and c.counts.sum() == c.lens.sum()
    return c


def _reference(c, lam, u=None):
    """(mtd, mask, G) float32 (B, T) of the rule; u: the actions where they are not the case's (bad-action test)."""
    B, T = c.B, c.T
    G = lambda_targets_reference(c.q_next, c.r[:, :T], c.term[:, :T], c.padded[:, :T], GAMMA, lam, np.float32)
    mask = np.float32(1) - c.padded[:, :T].astype(np.float32)
    mtd = mask * (G - c.e)
    assert G.dtype == np.float32 and mtd.dtype == np.float32
    return mtd, mask, G


def _out(k, fill=SENT):
    return torch.full((k + GUARD,), fill, dtype=torch.float32, device='cuda')


def _gpu(c, u=None):
    d = SimpleNamespace()
    for k in ('qe', 'qt', 'r', 'avail', 'term', 'padded', 'units'):
        setattr(d, k, torch.as_tensor(getattr(c, k)).cuda().contiguous())
    d.u = torch.as_tensor(c.u if u is None else u).cuda().contiguous()
    rows = np.array([(t * c.B + b) for b, t in c.unit_bt], np.int64)
    d.qe_packed = torch.as_tensor(c.qe.reshape(c.T * c.B, c.n, c.A)[rows]).cuda().contiguous()
    d.qt_packed = torch.as_tensor(c.qt.reshape(c.T * c.B, c.n, c.A)[rows]).cuda().contiguous()
    return d


def _call_padded(lib, c, d, lam, with_sums=True, **over):
    """One call of the padded entry point on fresh sentinel-filled outputs -> (rc, mtd, mask, targets, sums, counter)."""
    slots = c.B * c.T
    o = SimpleNamespace(mtd=_out(slots), mask=_out(slots), tgt=_out(slots), sums=_out(2), cnt=torch.zeros(1 + GUARD, dtype=torch.int32, device='cuda'),
                        part=torch.full((lib.vdn_td_lambda_sum_parts(c.B),), float('nan'), device='cuda'))
    a = dict(qe=_p(d.qe), qt=_p(d.qt), u=_p(d.u), r=_p(d.r), avail=_p(d.avail), term=_p(d.term), padded=_p(d.padded), B=c.B, T=c.T, Tl=c.Tl,
             n=c.n, A=c.A, mtd=_p(o.mtd), mask=_p(o.mask), cnt=_p(o.cnt), part=_p(o.part) if with_sums else None,
             sums=_p(o.sums) if with_sums else None, lam=lam, tgt=_p(o.tgt))
    a.update(over)
    o.rc = lib.vdn_td_lambda_forward_sums(a['qe'], a['qt'], a['u'], a['r'], a['avail'], a['term'], a['padded'], a['B'], a['T'], a['Tl'], a['n'],
                                          a['A'], GAMMA, a['mtd'], a['mask'], a['cnt'], a['part'], a['sums'], a['lam'], a['tgt'], None)
    torch.cuda.synchronize()
    return o


def _call_packed(lib, c, d, lam, with_sums=True, **over):
    U = len(c.units)
    o = SimpleNamespace(mtd=_out(U), mask=_out(U), tgt=_out(U), sums=_out(2), cnt=torch.zeros(1 + GUARD, dtype=torch.int32, device='cuda'),
                        part=torch.full((lib.vdn_td_lambda_sum_parts(int(c.counts[0])),), float('nan'), device='cuda'))
    counts = over.pop('counts', c.counts)
    a = dict(qe=_p(d.qe_packed), qt=_p(d.qt_packed), units=_p(d.units), U=U, u=_p(d.u), r=_p(d.r), avail=_p(d.avail), term=_p(d.term),
             padded=_p(d.padded), n=c.n, A=c.A, mtd=_p(o.mtd), mask=_p(o.mask), cnt=_p(o.cnt), part=_p(o.part) if with_sums else None,
             sums=_p(o.sums) if with_sums else None, lam=lam, tgt=_p(o.tgt), n_steps=len(counts),
             counts=(C.c_int32 * max(1, len(counts)))(*[int(k) for k in counts]))
    a.update(over)
    o.rc = lib.vdn_td_lambda_forward_packed_sums(a['qe'], a['qt'], a['units'], a['U'], a['u'], a['r'], a['avail'], a['term'], a['padded'], a['n'],
                                                 a['A'], GAMMA, a['mtd'], a['mask'], a['cnt'], a['part'], a['sums'], a['lam'], a['tgt'],
                                                 a['n_steps'], a['counts'], None)
    torch.cuda.synchronize()
    return o


def _guards_untouched(o, k):
    for name, used in (('mtd', k), ('mask', k), ('tgt', k), ('sums', 2)):
        assert bool((getattr(o, name)[used:] == SENT).all()), name
    assert bool((o.cnt[1:] == 0).all())


def _all_untouched(o):
    for name in ('mtd', 'mask', 'tgt', 'sums'):
        assert bool((getattr(o, name) == SENT).all()), name
    assert bool((o.cnt == 0).all())


def _check_sums(o, k):
    """d_sums against the float64 sums of the returned mtd^2 and mask: within n_slots * 2^-24 * sum (tests/test_gpu_learn_tail.py)."""
    num64 = float((o.mtd[:k].double() ** 2).sum())
    mask64 = float(o.mask[:k].double().sum())
    num, msum = float(o.sums[0]), float(o.sums[1])
    print('sums over %d slots: num %.9g (float64 %.9g, err %.3g, bound %.3g), mask %.9g (float64 %.9g)' % (
        k, num, num64, abs(num - num64), k * U24 * num64, msum, mask64))
    assert abs(num - num64) <= k * U24 * num64 and abs(msum - mask64) <= k * U24 * mask64


@pytest.mark.parametrize('lam', LAMBDAS)
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_every_slot_equals_the_float32_rule_bit_for_bit(shape, lam):
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_lambda()
    c = _case(shape)
    d = _gpu(c)
    want_mtd, want_mask, want_G = _reference(c, lam)
    slots = c.B * c.T
    o = _call_padded(lib, c, d, lam)
    assert o.rc == 0 and int(o.cnt[0]) == 0
    _guards_untouched(o, slots)
    got = [x[:slots].cpu().numpy().reshape(c.B, c.T) for x in (o.mtd, o.mask, o.tgt)]
    for name, g_, w_ in zip(('mtd', 'mask', 'targets'), got, (want_mtd, want_mask, want_G)):
        assert np.array_equal(_bits(g_), _bits(w_)), (name, float(np.abs(g_ - w_).max()))
    _check_sums(o, slots)
    again = _call_padded(lib, c, d, lam)                                    # fixed order: two launches, identical bits
    assert torch.equal(again.sums, o.sums) and torch.equal(again.mtd, o.mtd) and torch.equal(again.tgt, o.tgt)
    no_sums = _call_padded(lib, c, d, lam, with_sums=False, tgt=None)       # d_sums and d_targets may be NULL
    assert no_sums.rc == 0 and torch.equal(no_sums.mtd, o.mtd) and bool((no_sums.sums == SENT).all()) and bool((no_sums.tgt == SENT).all())
    if lam == 0.0:                                                          # the one-step entry point, bit for bit
        tail = _lib.vdn_tail()
        mtd0, mask0 = _out(slots), _out(slots)
        part0, sums0 = torch.empty(tail.vdn_td_sum_parts(slots), device='cuda'), _out(2)
        assert tail.vdn_td_forward_sums(_p(d.qe), _p(d.qt), _p(d.u), _p(d.r), _p(d.avail), _p(d.term), _p(d.padded), c.B, c.T, c.Tl, c.n, c.A,
                                        GAMMA, _p(mtd0), _p(mask0), None, _p(part0), _p(sums0), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(mtd0.view(torch.int32), o.mtd.view(torch.int32)) and torch.equal(mask0, o.mask)
    if c.T > PACKED_MAX_T:
        return
    # ---- the packed form on the same episodes: slot for slot the padded result
    U = len(c.units)
    bs, ts = np.array([b for b, _ in c.unit_bt]), np.array([t for _, t in c.unit_bt])
    p = _call_packed(lib, c, d, lam)
    assert p.rc == 0 and int(p.cnt[0]) == 0
    _guards_untouched(p, U)
    for name, x, w_, padded_out in (('mtd', p.mtd, want_mtd, got[0]), ('mask', p.mask, want_mask, got[1]), ('targets', p.tgt, want_G, got[2])):
        x = x[:U].cpu().numpy()
        assert np.array_equal(_bits(x), _bits(w_[bs, ts])), name
        assert np.array_equal(_bits(x), _bits(padded_out[bs, ts])), name
    _check_sums(p, U)
    again = _call_packed(lib, c, d, lam)
    assert torch.equal(again.sums, p.sums) and torch.equal(again.mtd, p.mtd)
    if lam == 0.0:
        mtd0, mask0 = _out(U), _out(U)
        part0, sums0 = torch.empty(tail.vdn_td_sum_parts(U), device='cuda'), _out(2)
        assert tail.vdn_td_forward_packed_sums(_p(d.qe_packed), _p(d.qt_packed), _p(d.units), U, _p(d.u), _p(d.r), _p(d.avail), _p(d.term),
                                               _p(d.padded), c.n, c.A, GAMMA, _p(mtd0), _p(mask0), None, _p(part0), _p(sums0), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(mtd0.view(torch.int32), p.mtd.view(torch.int32)) and torch.equal(mask0, p.mask)


@pytest.mark.parametrize('shape', [(5, 7, 40, 4, 5), (70, 40, 40, 4, 5)], ids=['5x7', '70x40'])
def test_bad_actions_poison_their_slots_only_and_are_counted(shape):
    """Actions outside [0, A) in two slots of one episode and one slot of another: NaN exactly there, every other slot still the
    rule's (G does not read u), the counter reads 3 -- in both forms."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_lambda()
    c = _case(shape)
    lam = 0.8
    u = c.u.copy()
    hit = [(0, 0, 1), (0, c.T - 1, 0), (1, 1, c.n - 1)]            # (episode, step, agent): all valid steps (lens[0] = T, lens[1] >= 2)
    assert c.lens[1] >= 2
    u[hit[0]], u[hit[1]], u[hit[2]] = c.A, -1, 127
    d = _gpu(c, u)
    want_mtd, want_mask, want_G = _reference(c, lam)
    poisoned = np.zeros((c.B, c.T), bool)
    for b, t, _ in hit:
        poisoned[b, t] = True
    o = _call_padded(lib, c, d, lam)
    mtd = o.mtd[:c.B * c.T].cpu().numpy().reshape(c.B, c.T)
    assert o.rc == 0 and int(o.cnt[0]) == 3
    assert np.array_equal(np.isnan(mtd), poisoned) and np.array_equal(_bits(mtd[~poisoned]), _bits(want_mtd[~poisoned]))
    assert np.array_equal(_bits(o.tgt[:c.B * c.T].cpu().numpy().reshape(c.B, c.T)), _bits(want_G))
    assert np.isnan(float(o.sums[0])) and float(o.sums[1]) == float(want_mask.sum())
    bs, ts = np.array([b for b, _ in c.unit_bt]), np.array([t for _, t in c.unit_bt])
    p = _call_packed(lib, c, d, lam)
    pm = p.mtd[:len(c.units)].cpu().numpy()
    assert p.rc == 0 and int(p.cnt[0]) == 3
    assert np.array_equal(np.isnan(pm), poisoned[bs, ts]) and np.array_equal(_bits(pm[~poisoned[bs, ts]]), _bits(want_mtd[bs, ts][~poisoned[bs, ts]]))


def test_argument_errors_come_back_before_any_launch():
    """VDN_ERR_BAD_ARG with every sentinel-filled output untouched: lam outside [0, 1] or NaN, T / n_steps above VDN_LAMBDA_MAX_T,
    counts that grow, are negative or do not sum to n_units, NULL required pointers."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_lambda()
    c = _case((5, 7, 40, 4, 5))
    d = _gpu(c)
    for over in (dict(lam=-0.01), dict(lam=1.5), dict(lam=float('nan')), dict(T=513, Tl=513), dict(T=41), dict(qe=None), dict(padded=None),
                 dict(mtd=None), dict(mask=None), dict(part=None), dict(A=128), dict(n=0)):
        o = _call_padded(lib, c, d, over.pop('lam', 0.8), **over)
        assert o.rc == BAD_ARG, over
        _all_untouched(o)
    grow, neg, short = c.counts.copy(), c.counts.copy(), c.counts.copy()
    grow[1], grow[2] = grow[2] - 1, grow[1] + 1          # same total, but counts[2] > counts[1]
    assert grow.sum() == c.counts.sum() and grow[2] > grow[1]
    neg[-1] = -1
    short[0] += 1
    for over in (dict(lam=-0.01), dict(lam=1.5), dict(lam=float('nan')), dict(counts=np.ones(513, np.int32), U=513), dict(counts=grow),
                 dict(counts=neg), dict(counts=short), dict(counts=c.counts[:-1]), dict(units=None), dict(qt=None), dict(mtd=None),
                 dict(part=None)):
        o = _call_packed(lib, c, d, over.pop('lam', 0.8), **over)
        assert o.rc == BAD_ARG, over
        _all_untouched(o)
    o = _packed_with_null_counts(lib, c, d)
    assert o.rc == BAD_ARG
    _all_untouched(o)
    assert lib.vdn_td_lambda_sum_parts(0) == 2 and lib.vdn_td_lambda_sum_parts(4) == 2 and lib.vdn_td_lambda_sum_parts(5) == 4


def _packed_with_null_counts(lib, c, d):
    U = len(c.units)
    o = SimpleNamespace(mtd=_out(U), mask=_out(U), tgt=_out(U), sums=_out(2), cnt=torch.zeros(1 + GUARD, dtype=torch.int32, device='cuda'),
                        part=torch.empty(lib.vdn_td_lambda_sum_parts(int(c.counts[0])), device='cuda'))
    o.rc = lib.vdn_td_lambda_forward_packed_sums(_p(d.qe_packed), _p(d.qt_packed), _p(d.units), U, _p(d.u), _p(d.r), _p(d.avail), _p(d.term),
                                                 _p(d.padded), c.n, c.A, GAMMA, _p(o.mtd), _p(o.mask), _p(o.cnt), _p(o.part), _p(o.sums), 0.8,
                                                 _p(o.tgt), len(c.counts), None, None)
    torch.cuda.synchronize()
    return o
