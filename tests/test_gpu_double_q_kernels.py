"""The TD block with double-Q targets through its C ABI (include/vdn_double.h: vdn_td_double_forward_sums and
vdn_td_double_forward_packed_sums), every output slot against the float32 numpy statement of the rule
(marl_dmfb_amd.policy.double_q.double_pick_reference fed into marl_dmfb_amd.policy.td_lambda.lambda_targets_reference) BIT FOR BIT, in
the style of tests/test_gpu_td_lambda_kernels.py, whose case generator supplies the episodes (lengths 1 to T, a long episode whose last
valid step is not terminated, a mid-episode termination, rows with one available action and rows with none, random values in padded
slots).  The selector is random and independent of the target Q; about one agent row in ten has its two largest available selector
values equal (the first must win), about one in twenty all of them."""
import ctypes as C
import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_td_lambda_kernels as lk
from marl_dmfb_amd.policy.double_q import double_pick_reference, selector_units

pytestmark = pytest.mark.gpu

GAMMA, SENT, GUARD, BAD_ARG = lk.GAMMA, lk.SENT, lk.GUARD, lk.BAD_ARG
PICK_SENT = 85          # what the picks buffer holds before a call
SHAPES = list(lk.SHAPES)                    # the last one, VDN_LAMBDA_MAX_T steps: padded form with lam > 0 only
PACKED_MAX_T = lk.PACKED_MAX_T
LAMBDAS = [0.0, 0.5, 1.0]
_p, _bits, _out = lk._p, lk._bits, lk._out


@functools.lru_cache(maxsize=None)
def _case(shape):
    """The case of tests/test_gpu_td_lambda_kernels.py (left unchanged: a copy) with a selector, the rule's picks and Q'."""
    base = lk._case(shape)
    c = SimpleNamespace(**vars(base))
    B, T, Tl, n, A = shape
    rng = np.random.default_rng(77000 + 1000 * B + T)
    qs = (rng.standard_normal((T, B, n, A)) * 2).astype(np.float32)
    avail = c.avail[:, :T].transpose(1, 0, 2, 3)                                   # (T, B, n, A)
    kind = rng.random((T, B, n))
    order = np.argsort(np.where(avail == 0, -np.inf, qs), axis=-1, kind='stable')
    top, second = order[..., -1:], order[..., -2:-1]
    two = (kind < 0.1) & (avail.sum(-1) >= 2)                                      # the two largest available values equal
    tied = np.where(two[..., None], np.take_along_axis(qs, top, -1), np.take_along_axis(qs, second, -1))
    np.put_along_axis(qs, second, tied, -1)
    flat = kind > 0.95                                                             # all values equal
    qs[flat] = qs[flat][:, :1]
    c.qs = qs
    c.n_two, c.n_flat = int(two.sum()), int(flat.sum())
    c.picks, c.q_next = double_pick_reference(qs.transpose(1, 0, 2, 3), c.qt.transpose(1, 0, 2, 3), c.avail[:, :T], np.float32)
    assert c.picks.dtype == np.int8 and c.q_next.dtype == np.float32 and c.q_next.shape == (B, T)
    c.bs, c.ts = np.array([b for b, _ in c.unit_bt]), np.array([t for _, t in c.unit_bt])
    return c


def _gpu(c, u=None):
    d = lk._gpu(c, u)
    rows = np.array([(t * c.B + b) for b, t in c.unit_bt], np.int64)
    d.qs = torch.as_tensor(c.qs).cuda().contiguous()
    d.qs_packed = torch.as_tensor(c.qs.reshape(c.T * c.B, c.n, c.A)[rows]).cuda().contiguous()
    return d


def _reference(c, lam, q_next=None):
    """(mtd, mask, G) float32 (B, T): the rule's Q' through the lambda rule of tests/test_gpu_td_lambda_kernels.py."""
    r = SimpleNamespace(**vars(c))
    if q_next is not None:
        r.q_next = q_next
    return lk._reference(r, lam)


def _outputs(lib_parts, k, episodes, lam, n):
    parts = lib_parts(k, episodes, lam)
    return SimpleNamespace(mtd=_out(k), mask=_out(k), tgt=_out(k), sums=_out(2), cnt=torch.zeros(1 + GUARD, dtype=torch.int32, device='cuda'),
                           part=torch.full((parts,), float('nan'), device='cuda'),
                           picks=torch.full((k * n + GUARD,), PICK_SENT, dtype=torch.int8, device='cuda'))


def _parts(k, episodes, lam):
    """d_part's floats: the one-step rule's at lam == 0, the lambda walk's at lam > 0 (include/vdn_double.h)."""
    from marl_dmfb_amd import _lib
    return _lib.vdn_lambda().vdn_td_lambda_sum_parts(episodes) if lam else _lib.vdn_tail().vdn_td_sum_parts(k)


def _call_padded(lib, c, d, lam, with_sums=True, **over):
    slots = c.B * c.T
    o = _outputs(_parts, slots, c.B, lam, c.n)
    a = dict(qe=_p(d.qe), qt=_p(d.qt), u=_p(d.u), r=_p(d.r), avail=_p(d.avail), term=_p(d.term), padded=_p(d.padded), B=c.B, T=c.T, Tl=c.Tl,
             n=c.n, A=c.A, mtd=_p(o.mtd), mask=_p(o.mask), cnt=_p(o.cnt), part=_p(o.part) if with_sums else None,
             sums=_p(o.sums) if with_sums else None, lam=lam, tgt=_p(o.tgt), qs=_p(d.qs), picks=_p(o.picks))
    a.update(over)
    o.rc = lib.vdn_td_double_forward_sums(a['qe'], a['qt'], a['u'], a['r'], a['avail'], a['term'], a['padded'], a['B'], a['T'], a['Tl'], a['n'],
                                          a['A'], GAMMA, a['mtd'], a['mask'], a['cnt'], a['part'], a['sums'], a['lam'], a['tgt'], a['qs'],
                                          a['picks'], None)
    torch.cuda.synchronize()
    return o


def _call_packed(lib, c, d, lam, with_sums=True, **over):
    U = len(c.units)
    o = _outputs(_parts, U, int(c.counts[0]), lam, c.n)
    counts = over.pop('counts', c.counts)
    a = dict(qe=_p(d.qe_packed), qt=_p(d.qt_packed), units=_p(d.units), U=U, u=_p(d.u), r=_p(d.r), avail=_p(d.avail), term=_p(d.term),
             padded=_p(d.padded), n=c.n, A=c.A, mtd=_p(o.mtd), mask=_p(o.mask), cnt=_p(o.cnt), part=_p(o.part) if with_sums else None,
             sums=_p(o.sums) if with_sums else None, lam=lam, tgt=_p(o.tgt), n_steps=len(c.counts if counts is None else counts),
             counts=None if counts is None else (C.c_int32 * max(1, len(counts)))(*[int(k) for k in counts]), qs=_p(d.qs_packed), n_sel=U, sel_units=None,
             picks=_p(o.picks))
    a.update(over)
    o.rc = lib.vdn_td_double_forward_packed_sums(a['qe'], a['qt'], a['units'], a['U'], a['u'], a['r'], a['avail'], a['term'], a['padded'], a['n'],
                                                 a['A'], GAMMA, a['mtd'], a['mask'], a['cnt'], a['part'], a['sums'], a['lam'], a['tgt'],
                                                 a['n_steps'], a['counts'], a['qs'], a['n_sel'], a['sel_units'], a['picks'], None)
    torch.cuda.synchronize()
    return o


def _guards_untouched(o, k, n):
    lk._guards_untouched(o, k)
    assert bool((o.picks[k * n:] == PICK_SENT).all())


def _all_untouched(o):
    lk._all_untouched(o)
    assert bool((o.picks == PICK_SENT).all())


def _same(a, b, names=('mtd', 'mask', 'tgt', 'sums')):
    return all(torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32)) for k in names) and torch.equal(a.picks, b.picks)


def _cases():
    return [(s, lam) for s in SHAPES for lam in LAMBDAS if s[1] <= PACKED_MAX_T or lam > 0]


@pytest.mark.parametrize('shape,lam', _cases(), ids=['%s-lam%g' % ('x'.join(map(str, s)), lam) for s, lam in _cases()])
def test_every_slot_equals_the_float32_rule_bit_for_bit(shape, lam):
    from marl_dmfb_amd import _lib
    lib, tail, lamlib = _lib.vdn_double(), _lib.vdn_tail(), _lib.vdn_lambda()
    c = _case(shape)
    d = _gpu(c)
    want_mtd, want_mask, want_G = _reference(c, lam)
    slots = c.B * c.T
    print('\n%s: %d rows with their two largest selector values equal, %d with all equal' % (shape, c.n_two, c.n_flat))
    o = _call_padded(lib, c, d, lam)
    assert o.rc == 0 and int(o.cnt[0]) == 0
    _guards_untouched(o, slots, c.n)
    got = [x[:slots].cpu().numpy().reshape(c.B, c.T) for x in (o.mtd, o.mask, o.tgt)]
    for name, g_, w_ in zip(('mtd', 'mask', 'targets'), got, (want_mtd, want_mask, want_G)):
        assert np.array_equal(_bits(g_), _bits(w_)), (name, float(np.abs(g_ - w_).max()))
    got_picks = o.picks[:slots * c.n].cpu().numpy().reshape(c.B, c.T, c.n)
    assert np.array_equal(got_picks, c.picks), int((got_picks != c.picks).sum())
    lk._check_sums(o, slots)
    assert _same(_call_padded(lib, c, d, lam), o)                                   # fixed order: two launches, identical bits
    bare = _call_padded(lib, c, d, lam, with_sums=False, tgt=None, picks=None)      # d_sums, d_targets and d_picks may be NULL
    assert bare.rc == 0 and torch.equal(bare.mtd, o.mtd) and torch.equal(bare.mask, o.mask)
    assert bool((bare.sums == SENT).all()) and bool((bare.tgt == SENT).all()) and bool((bare.picks == PICK_SENT).all())
    for which in (dict(tgt=None), dict(picks=None)):
        one = _call_padded(lib, c, d, lam, **which)
        assert one.rc == 0 and torch.equal(one.mtd, o.mtd) and torch.equal(one.sums, o.sums)
    # the selector equal to the target network: the entry points without a selector, bit for bit (mtd and sums)
    own = _call_padded(lib, c, d, lam, qs=_p(d.qt))
    if lam == 0.0:
        mtd0, mask0 = _out(slots), _out(slots)
        part0, sums0 = torch.empty(tail.vdn_td_sum_parts(slots), device='cuda'), _out(2)
        assert tail.vdn_td_forward_sums(_p(d.qe), _p(d.qt), _p(d.u), _p(d.r), _p(d.avail), _p(d.term), _p(d.padded), c.B, c.T, c.Tl, c.n, c.A,
                                        GAMMA, _p(mtd0), _p(mask0), None, _p(part0), _p(sums0), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(mtd0.view(torch.int32), own.mtd.view(torch.int32)) and torch.equal(sums0.view(torch.int32), own.sums.view(torch.int32))
    elif lam == 0.5:
        plain = lk._call_padded(lamlib, c, d, lam)
        assert plain.rc == 0 and torch.equal(plain.mtd.view(torch.int32), own.mtd.view(torch.int32))
        assert torch.equal(plain.sums.view(torch.int32), own.sums.view(torch.int32)) and torch.equal(plain.tgt, own.tgt)
    if c.T > PACKED_MAX_T:
        return
    # ---- the packed form on the same episodes: slot for slot the padded result
    U = len(c.units)
    p = _call_packed(lib, c, d, lam)
    assert p.rc == 0 and int(p.cnt[0]) == 0
    _guards_untouched(p, U, c.n)
    for name, x, w_, padded_out in (('mtd', p.mtd, want_mtd, got[0]), ('mask', p.mask, want_mask, got[1]), ('targets', p.tgt, want_G, got[2])):
        x = x[:U].cpu().numpy()
        assert np.array_equal(_bits(x), _bits(w_[c.bs, c.ts])), name
        assert np.array_equal(_bits(x), _bits(padded_out[c.bs, c.ts])), name
    pp = p.picks[:U * c.n].cpu().numpy().reshape(U, c.n)
    assert np.array_equal(pp, c.picks[c.bs, c.ts]) and np.array_equal(pp, got_picks[c.bs, c.ts])
    lk._check_sums(p, U)
    assert _same(_call_packed(lib, c, d, lam), p)
    bare = _call_packed(lib, c, d, lam, with_sums=False, tgt=None, picks=None)
    assert bare.rc == 0 and torch.equal(bare.mtd, p.mtd) and bool((bare.sums == SENT).all()) and bool((bare.picks == PICK_SENT).all())
    ident = torch.arange(U, dtype=torch.int32, device='cuda')                       # NULL = the identity list
    assert _same(_call_packed(lib, c, d, lam, sel_units=_p(ident)), p)
    own = _call_packed(lib, c, d, lam, qs=_p(d.qt_packed))
    if lam == 0.0:
        mtd0, mask0 = _out(U), _out(U)
        part0, sums0 = torch.empty(tail.vdn_td_sum_parts(U), device='cuda'), _out(2)
        assert tail.vdn_td_forward_packed_sums(_p(d.qe_packed), _p(d.qt_packed), _p(d.units), U, _p(d.u), _p(d.r), _p(d.avail), _p(d.term),
                                               _p(d.padded), c.n, c.A, GAMMA, _p(mtd0), _p(mask0), None, _p(part0), _p(sums0), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(mtd0.view(torch.int32), own.mtd.view(torch.int32)) and torch.equal(sums0.view(torch.int32), own.sums.view(torch.int32))
        no_counts = _call_packed(lib, c, d, lam, n_steps=0, counts=None)            # counts are read only when lam > 0
        assert no_counts.rc == 0 and _same(no_counts, p)
    elif lam == 0.5:
        plain = lk._call_packed(lamlib, c, d, lam)
        assert plain.rc == 0 and torch.equal(plain.mtd.view(torch.int32), own.mtd.view(torch.int32))
        assert torch.equal(plain.sums.view(torch.int32), own.sums.view(torch.int32))


def _learner_selector(c, rng):
    """The selector tensor as VDN.learn_packed lays it out: the U units of the eval network's Q, then one tail unit per episode; the
    selector of unit (b, t) is unit (b, t + 1), or the tail unit of b behind its last valid step.  Step-0 units select nothing."""
    U, B = len(c.units), c.B
    S = (rng.standard_normal((U + B, c.n, c.A)) * 2).astype(np.float32)
    for j, (b, t) in enumerate(c.unit_bt):
        if t >= 1:
            S[j] = c.qs[t - 1, b]
    for b in range(B):
        S[U + b] = c.qs[c.lens[b] - 1, b]
    return S


@pytest.mark.parametrize('lam', [0.0, 0.8])
@pytest.mark.parametrize('shape', [(5, 7, 40, 4, 5), (70, 40, 40, 4, 5)], ids=['5x7', '70x40'])
def test_the_learners_selector_mapping(shape, lam):
    """sel_units as policy/double_q.py: selector_units builds them, n_sel_units = U + B: the padded result, slot for slot."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_double()
    c = _case(shape)
    d = _gpu(c)
    U = len(c.units)
    sel, last = selector_units(c.counts)
    off = np.concatenate([[0], np.cumsum(c.counts)])
    assert [c.unit_bt[j] for j in last] == [(b, c.lens[b] - 1) for b in range(c.B)]
    for j, (b, t) in enumerate(c.unit_bt):
        assert sel[j] == (off[t + 1] + b if t + 1 < c.lens[b] else U + b)
    S = torch.as_tensor(_learner_selector(c, np.random.default_rng(5))).cuda()
    sel_d = torch.as_tensor(sel).cuda()
    p = _call_packed(lib, c, d, lam, qs=_p(S), n_sel=U + c.B, sel_units=_p(sel_d))
    want_mtd, want_mask, want_G = _reference(c, lam)
    assert p.rc == 0 and int(p.cnt[0]) == 0
    _guards_untouched(p, U, c.n)
    for name, x, w_ in (('mtd', p.mtd, want_mtd), ('mask', p.mask, want_mask), ('targets', p.tgt, want_G)):
        assert np.array_equal(_bits(x[:U].cpu().numpy()), _bits(w_[c.bs, c.ts])), name
    assert np.array_equal(p.picks[:U * c.n].cpu().numpy().reshape(U, c.n), c.picks[c.bs, c.ts])


@pytest.mark.parametrize('lam', [0.0, 0.8])
def test_selector_units_outside_the_tensor_poison_their_slots_only(lam):
    """Three entries of d_sel_units outside [0, n_sel_units): -1, n_sel_units and 2^30.  They are never used as an index: NaN exactly
    there, picks -1 there, the counter reads 3.  Such a slot's Q' is formed with its own target rows as the selector (include/
    vdn_double.h), so every other slot keeps the bits of the rule with that selector -- at lam == 0, and for the slots that no bad slot's
    return reaches, the bits of the rule with the selector as given."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_double()
    c = _case((70, 40, 40, 4, 5))
    d = _gpu(c)
    U = len(c.units)
    hit = [c.unit_bt.index((0, 0)), c.unit_bt.index((0, c.T - 1)), c.unit_bt.index((1, 1))]
    sel = np.arange(U, dtype=np.int32)
    sel[hit[0]], sel[hit[1]], sel[hit[2]] = -1, U, 2 ** 30
    qs_bt = c.qs.transpose(1, 0, 2, 3).copy()
    for j in hit:
        b, t = c.unit_bt[j]
        qs_bt[b, t] = c.qt[t, b]
    _, q_next = double_pick_reference(qs_bt, c.qt.transpose(1, 0, 2, 3), c.avail[:, :c.T], np.float32)
    want_mtd, want_mask, want_G = _reference(c, lam, q_next)
    as_given = _reference(c, lam)[0]
    poisoned = np.zeros(U, bool)
    poisoned[hit] = True
    sel_d = torch.as_tensor(sel).cuda()
    p = _call_packed(lib, c, d, lam, sel_units=_p(sel_d))
    assert p.rc == 0 and int(p.cnt[0]) == 3
    _guards_untouched(p, U, c.n)
    pm = p.mtd[:U].cpu().numpy()
    assert np.array_equal(np.isnan(pm), poisoned)
    assert np.array_equal(_bits(pm[~poisoned]), _bits(want_mtd[c.bs, c.ts][~poisoned]))
    assert np.array_equal(_bits(p.tgt[:U].cpu().numpy()), _bits(want_G[c.bs, c.ts]))
    untouched = ~poisoned & ~np.isin(c.bs, [0, 1]) if lam else ~poisoned
    assert np.array_equal(_bits(pm[untouched]), _bits(as_given[c.bs, c.ts][untouched]))
    picks = p.picks[:U * c.n].cpu().numpy().reshape(U, c.n)
    assert bool((picks[poisoned] == -1).all()) and np.array_equal(picks[~poisoned], c.picks[c.bs, c.ts][~poisoned])
    assert np.isnan(float(p.sums[0])) and float(p.sums[1]) == float(want_mask[c.bs, c.ts].sum())


@pytest.mark.parametrize('shape', [(5, 7, 40, 4, 5), (70, 40, 40, 4, 5)], ids=['5x7', '70x40'])
def test_bad_actions_poison_their_slots_only_and_are_counted(shape):
    """Actions outside [0, A) in two slots of one episode and one slot of another: NaN exactly there, every other slot still the
    rule's (neither G nor the picks read u), the counter reads 3 -- in both forms."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_double()
    c = _case(shape)
    lam = 0.5
    u = c.u.copy()
    hit = [(0, 0, 1), (0, c.T - 1, 0), (1, 1, c.n - 1)]
    assert c.lens[1] >= 2
    u[hit[0]], u[hit[1]], u[hit[2]] = c.A, -1, 127
    d = _gpu(c, u)
    want_mtd, want_mask, want_G = _reference(c, lam)
    poisoned = np.zeros((c.B, c.T), bool)
    for b, t, _ in hit:
        poisoned[b, t] = True
    slots = c.B * c.T
    o = _call_padded(lib, c, d, lam)
    mtd = o.mtd[:slots].cpu().numpy().reshape(c.B, c.T)
    assert o.rc == 0 and int(o.cnt[0]) == 3
    assert np.array_equal(np.isnan(mtd), poisoned) and np.array_equal(_bits(mtd[~poisoned]), _bits(want_mtd[~poisoned]))
    assert np.array_equal(_bits(o.tgt[:slots].cpu().numpy().reshape(c.B, c.T)), _bits(want_G))
    assert np.array_equal(o.picks[:slots * c.n].cpu().numpy().reshape(c.B, c.T, c.n), c.picks)
    assert np.isnan(float(o.sums[0])) and float(o.sums[1]) == float(want_mask.sum())
    U = len(c.units)
    for lam_p in (0.0, lam):
        want = _reference(c, lam_p)[0]
        p = _call_packed(lib, c, d, lam_p)
        pm = p.mtd[:U].cpu().numpy()
        assert p.rc == 0 and int(p.cnt[0]) == 3
        assert np.array_equal(np.isnan(pm), poisoned[c.bs, c.ts])
        assert np.array_equal(_bits(pm[~poisoned[c.bs, c.ts]]), _bits(want[c.bs, c.ts][~poisoned[c.bs, c.ts]]))
        assert np.array_equal(p.picks[:U * c.n].cpu().numpy().reshape(U, c.n), c.picks[c.bs, c.ts])


def test_argument_errors_come_back_before_any_launch():
    """VDN_ERR_BAD_ARG with every sentinel-filled output untouched: what the lambda entry points refuse (at lam == 0 too, but for the
    counts, which are read only when lam > 0), d_q_sel == NULL, n_sel_units < 1, no list and fewer selector units than units."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_double()
    c = _case((5, 7, 40, 4, 5))
    d = _gpu(c)
    U = len(c.units)
    for lam0 in (0.0, 0.8):
        for over in (dict(lam=-0.01), dict(lam=1.5), dict(lam=float('nan')), dict(T=513, Tl=513), dict(T=41), dict(qe=None), dict(padded=None),
                     dict(mtd=None), dict(mask=None), dict(part=None), dict(A=128), dict(n=0), dict(qs=None)):
            o = _call_padded(lib, c, d, over.pop('lam', lam0), **over)
            assert o.rc == BAD_ARG, over
            _all_untouched(o)
    grow, neg, short = c.counts.copy(), c.counts.copy(), c.counts.copy()
    grow[1], grow[2] = grow[2] - 1, grow[1] + 1
    assert grow.sum() == c.counts.sum() and grow[2] > grow[1]
    neg[-1] = -1
    short[0] += 1
    ident = torch.arange(U, dtype=torch.int32, device='cuda')
    both = (dict(lam=-0.01), dict(lam=1.5), dict(lam=float('nan')), dict(units=None), dict(qt=None), dict(mtd=None), dict(part=None),
            dict(qs=None), dict(n_sel=0), dict(n_sel=-3, sel_units=_p(ident)), dict(n_sel=U - 1), dict(n_steps=513), dict(n_steps=-1),
            dict(A=128))
    walk_only = (dict(counts=np.ones(513, np.int32), U=513), dict(counts=grow), dict(counts=neg), dict(counts=short), dict(counts=c.counts[:-1]),
                 dict(counts=None))
    for lam0, overs in ((0.0, both), (0.8, both + walk_only)):
        for over in overs:
            over = dict(over)
            o = _call_packed(lib, c, d, over.pop('lam', lam0), **over)
            assert o.rc == BAD_ARG, over
            _all_untouched(o)


def test_header_prototypes_match_the_binding_table():
    """include/vdn_double.h against _lib.SIGNATURES['vdn_double']: the same names, the same number of arguments."""
    from marl_dmfb_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'vdn_double.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    protos = {m.group(1): len(m.group(2).split(',')) for m in re.finditer(r'\bint\s+(vdn_\w+)\s*\(([^)]*)\)\s*;', text)}
    table = {fn: len(sig[0] if isinstance(sig, tuple) else sig) for fn, sig in _lib.SIGNATURES['vdn_double'].items()}
    assert protos == table and len(table) == 2
    assert _lib._FILE['vdn_double'] == 'vdn_ops'
    lib = _lib.vdn_double()
    for fn in table:
        getattr(lib, fn)
