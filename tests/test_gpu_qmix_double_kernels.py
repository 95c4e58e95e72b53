"""The mixing + TD block of the QMIX learn with double-Q targets through its C ABI (include/qmix_double.h: qmix_mix_td_double_forward and
qmix_mix_td_double_forward_packed; csrc/qmix_ops.hip: k_mix_forward<H, Index, kTotals, MixSel>).

The reference is the PARENT's kernels and exact float32 comparisons only.  picks_ref = double_pick_reference(q_sel, q_target, avail,
float32)[0] is the rule in numpy (comparisons of float32 values: no rounding in it).  The existing entry points are then fed the same
inputs with avail' = one_hot(picks_ref) AND avail: their maximum over the target row is the value at the pick (-9999999 where the pick
is unavailable, an all-unavailable row stays all zeros), so d_mtd, d_mask, d_targets and the two q_tot of the existing one-step and
lambda entry points must equal the new entry points' BIT FOR BIT, padded and packed, at lambda 0, 0.5, 0.8 and 1.

  picks         d_picks == picks_ref in every output row, padded ones included
  packed        slot for slot the padded result on a length-sorted draw, with d_sel_units built by selector_units (n_sel_units = U + B,
                the unused selector units NaN) and with d_sel_units NULL;  a second launch gives the same bits
  q_sel == q_target   the bits of the existing entry points on the unchanged inputs
  data          asserted per case with A > 1: at least half of the picks differ from the target row's own first maximum, an exact tie
                in the selector, an agent with no available action, a selector maximum at an unavailable action, NaN at selector
                action 0 and at a later one
  shapes        (B, T) = (1, 1), (1, 2), (3, 11), (5, 7), (31, 1) with 32 and 33 rows beside it, (2, 65), and (2, 512) at
                lambda 0.8 only; both H, n in {1, 4, 16}, A in {1, 5, 16}; the ring, separate and wide P layouts
  a selector unit outside its tensor (low and high), alone and with a bad action; d_picks NULL; every QMIX_ERR_BAD_ARG and
  QMIX_ERR_UNSUPPORTED case of the header with NaN-filled outputs left untouched; the exports.

Every buffer sits between guard regions (front_kernel_cases.guarded)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import qmix_kernel_cases as K
import test_gpu_qmix_kernels as P
import test_gpu_qmix_lambda_kernels as LK
import test_gpu_qmix_packed_kernels as PK
from marl_dmfb_amd.policy.double_q import double_pick_reference, selector_units
from test_cabi_exports import _prototypes

pytestmark = pytest.mark.gpu

SENT = P.SENT
PICK_SENT = 99
BAD_ARG, UNSUPPORTED = -1, -6
LAMBDAS = LK.LAMBDAS
MAX_T = LK.MAX_T
# (B, T, n, H, A, layout) -> the lambdas it runs at
COMBOS = [((1, 1, 1, 24, 1, 'ring'), LAMBDAS), ((1, 2, 4, 32, 5, 'sep'), LAMBDAS), ((3, 11, 16, 24, 16, 'wide'), LAMBDAS),
          ((5, 7, 4, 32, 5, 'ring'), LAMBDAS), ((5, 7, 4, 32, 5, 'sep'), LAMBDAS), ((5, 7, 4, 32, 5, 'wide'), LAMBDAS),
          ((31, 1, 16, 32, 16, 'sep'), LAMBDAS), ((4, 8, 1, 24, 16, 'wide'), LAMBDAS), ((2, 65, 1, 24, 5, 'sep'), LAMBDAS),
          ((2, MAX_T, 4, 32, 5, 'ring'), [0.8])]
IDS = ['B%d_T%d_n%d_H%d_A%d_%s' % c for c, _ in COMBOS]
assert {c[0] * c[1] for c, _ in COMBOS} >= {31, 32, 33} and {c[3] for c, _ in COMBOS} == {24, 32}
assert {c[2] for c, _ in COMBOS} == {1, 4, 16} and {c[4] for c, _ in COMBOS} == {1, 5, 16} and {c[5] for c, _ in COMBOS} == {'ring', 'sep', 'wide'}
OUT = ('mtd', 'mask', 'tgt', 'tot_e', 'tot_t')


def _bits(x):
    return np.ascontiguousarray(torch.as_tensor(x).cpu().numpy(), np.float32).view(np.int32)


def _case(combo):
    """LK._case (its episodes: L = T, 1, 0, T-1, ...) with a selector c.q_sel (T, B, n, A) float32 of its own and, where A > 1, five
    (b, t, agent) slots written for the data conditions (c.slots); c.picks (B, T, n) is the rule's result in numpy."""
    c = LK._case(combo, 'real')
    B, T, n, A = c.B, c.T, c.n, c.A
    rng = np.random.default_rng(7 * B + 13 * T + n + A)
    sel = (rng.standard_normal((B, T, n, A)) * 2.0).astype(np.float32)
    avail = c.avail.numpy()                                     # shares the tensor's memory
    c.slots = {}
    if A > 1:
        flat = rng.permutation(B * T * n)[:5]
        names = ('tie', 'none', 'unavailable_max', 'nan_first', 'nan_later')
        for name, f in zip(names, flat):
            b, t, i = int(f // (T * n)), int(f // n % T), int(f % n)
            c.slots[name] = (b, t, i)
            if name == 'tie':
                avail[b, t, i, :] = 1
                sel[b, t, i, 1] = sel[b, t, i, A - 1] = 50.0
            elif name == 'none':
                avail[b, t, i, :] = 0
            elif name == 'unavailable_max':
                avail[b, t, i, :] = 1
                avail[b, t, i, 1] = 0
                sel[b, t, i, 1] = 100.0
            elif name == 'nan_first':
                avail[b, t, i, :] = 1
                sel[b, t, i, 0] = np.nan
            else:
                avail[b, t, i, :] = 1
                sel[b, t, i, A - 1] = np.nan
    q_t = c.q_t.permute(1, 0, 2, 3).numpy()
    c.picks = double_pick_reference(sel, q_t, avail[:, :T], np.float32)[0]
    c.q_sel = torch.as_tensor(sel).permute(1, 0, 2, 3).contiguous()
    c.sel_bt = sel
    return c


def _conditions(c):
    """The data conditions of the module docstring, from the arrays."""
    if c.A == 1:
        assert not c.picks.any()
        return
    T = c.T
    avail, q_t = c.avail.numpy()[:, :T], c.q_t.permute(1, 0, 2, 3).numpy()
    own = double_pick_reference(q_t, q_t, avail, np.float32)[0]            # the target row's own first maximum
    share = float((c.picks != own).mean())
    assert share >= 0.5, share
    s = c.slots
    row = lambda name: (c.sel_bt[s[name]], avail[s[name]], int(c.picks[s[name]]))
    v, a, p = row('tie')
    assert a.all() and v[1] == v[c.A - 1] == np.nanmax(v) and p == 1                       # the first maximum wins
    v, a, p = row('none')
    assert not a.any() and p == 0
    v, a, p = row('unavailable_max')
    assert int(np.nanargmax(v)) == 1 and a[1] == 0 and p != 1 and a[p] == 1
    v, a, p = row('nan_first')
    assert np.isnan(v[0]) and a[0] == 1 and p == 0                                       # nothing displaces a NaN
    v, a, p = row('nan_later')
    assert np.isnan(v[c.A - 1]) and a[c.A - 1] == 1 and p != c.A - 1                       # a NaN displaces nothing
    assert len(np.unique(c.picks)) >= min(c.A, 3)


def _one_hot_case(c):
    """The case with avail' = one_hot(picks) AND avail in the steps the call covers: what the existing entry points are fed."""
    c2 = copy.copy(c)
    T = c.T
    avail = c.avail.clone()
    hot = torch.zeros_like(avail[:, :T]).scatter_(3, torch.as_tensor(c.picks.astype(np.int64)).unsqueeze(3), 1)
    avail[:, :T] = avail[:, :T] * hot
    assert int(avail[:, :T].sum(3).max()) <= 1
    c2.avail = avail
    return c2


def _put(d, t):
    v, chk = P._put(t)
    d.checks.append(chk)
    return v


def _outputs(d, rows, n, fill):
    o = LK._outputs(d, rows, fill)
    o.picks = P._out(d, (rows, n), PICK_SENT, torch.int8)
    return o


def _finish(d, o, fill, lam, picks=True):
    torch.cuda.synchronize()
    for chk in d.checks:
        chk()
    if o.rc == 0 and fill == fill:            # (a NaN fill is for the calls that must write nothing: `_all_untouched`)
        for name in ('mtd', 'mask'):
            assert not bool((getattr(o, name) == fill).any()), (name, 'an output element was left unwritten')
        for name in ('tot_e', 'tot_t'):       # the hand-off of the two launches: written under lambda, not read or written without
            x = getattr(o, name)
            assert not bool((x == fill).any()) if lam > 0 else bool((x == fill).all()), name
        assert bool((o.picks != PICK_SENT).all()) if picks else bool((o.picks == PICK_SENT).all())
    return o


def _double_padded(c, d, lam0, sel0, fill=SENT, picks=True, **over):
    """One call of the padded entry point on fresh sentinel-filled outputs; `over` replaces arguments by their names in `a`."""
    o = _outputs(d, c.R, c.n, fill)
    a = LK._args_padded(c, d, o, lam0)
    a.update(sel=P._p(sel0), picks=P._p(o.picks) if picks else None)
    a.update(over)
    o.rc = P._lib().qmix_double().qmix_mix_td_double_forward(
        a['qe'], a['qt'], a['u'], a['r'], a['avail'], a['term'], a['padded'], a['B'], a['T'], a['Tl'], a['n'], a['A'], a['pe'], a['pe_rows'],
        a['pe_off'], a['pt'], a['pt_rows'], a['pt_off'], a['H'], a['M'], a['ev'], a['tg'], a['gamma'], a['mtd'], a['mask'], a['cnt'], a['lam'],
        a['tot_e'], a['tot_t'], a['tgt'], a['sel'], a['picks'], None)
    return _finish(d, o, fill, a['lam'], a['picks'] is not None)


def _double_packed(c, d, k, lam0, sel0, n_sel0, units0, fill=SENT, picks=True, **over):
    """One call of the packed entry point on the units `k` (PK._pack) on fresh sentinel-filled outputs; `over` as in `_double_padded`."""
    p = P._p
    o = _outputs(d, max(k.U, 1), c.n, fill)
    counts = over.pop('counts', LK._counts(c))
    a = dict(qe=p(k.q_e), qt=p(k.q_t), units=p(k.units), U=k.U, u=p(d.u), r=p(d.r), avail=p(d.avail), term=p(d.term), padded=p(d.padded),
             n=c.n, A=c.A, pe=p(k.pe), pt=p(k.pt), trow=p(k.trow), H=c.H, M=K.M, ev=C.byref(d.mix_e), tg=C.byref(d.mix_t), gamma=c.gamma,
             mtd=p(o.mtd), mask=p(o.mask), cnt=p(o.cnt), lam=lam0, tot_e=p(o.tot_e), tot_t=p(o.tot_t), tgt=p(o.tgt),
             n_steps=len(counts), counts=(C.c_int32 * max(1, len(counts)))(*[int(x) for x in counts]), sel=p(sel0), n_sel=n_sel0,
             sel_units=p(units0), picks=p(o.picks) if picks else None)
    a.update(over)
    o.rc = P._lib().qmix_double().qmix_mix_td_double_forward_packed(
        a['qe'], a['qt'], a['units'], a['U'], a['u'], a['r'], a['avail'], a['term'], a['padded'], a['n'], a['A'], a['pe'], a['pt'], a['trow'],
        a['H'], a['M'], a['ev'], a['tg'], a['gamma'], a['mtd'], a['mask'], a['cnt'], a['lam'], a['tot_e'], a['tot_t'], a['tgt'],
        a['n_steps'], a['counts'], a['sel'], a['n_sel'], a['sel_units'], a['picks'], None)
    return _finish(d, o, fill, a['lam'], a['picks'] is not None)


def _packed_selector(c, d, bt):
    """The selector of the units `bt` in the learner's layout: U + B' units (B' = the episodes with a valid step), the selector of
    unit j at unit selector_units(counts)[0][j], every unit that no list entry names NaN -> (tensor, n_sel_units, device list)."""
    b, t = torch.tensor([x[0] for x in bt]), torch.tensor([x[1] for x in bt])
    counts = LK._counts(c)
    sel_units = selector_units(counts)[0]
    U, E = len(bt), counts[0]
    full = torch.full((U + E, c.n, c.A), float('nan'))
    full[torch.as_tensor(sel_units.astype(np.int64))] = c.q_sel[t, b]
    assert int(torch.isnan(full).all(2).all(1).sum()) == E                # the units of step 0 select for nobody
    return _put(d, full), U + E, _put(d, torch.as_tensor(sel_units)), c.q_sel[t, b]


def _same(a, b, names, rows=None, what=''):
    for name in names:
        x, y = getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()
        if rows is not None:
            y = y[rows]
        assert np.array_equal(_bits(x), _bits(y)), (what, name)


@pytest.mark.parametrize('combo,lambdas', COMBOS, ids=IDS)
def test_equals_the_existing_kernels_on_the_one_hot_of_the_picks_bit_for_bit(combo, lambdas):
    c = _case(combo)
    _conditions(c)
    c2 = _one_hot_case(c)
    d, d2 = P._to_gpu(c), P._to_gpu(c2)
    sel = _put(d, c.q_sel)
    picks_ref = c.picks.reshape(c.R, c.n)
    bt = PK._units(c)
    assert len(bt) == int(c.lens.sum())
    rows = np.array([b * c.T + t for b, t in bt], np.int64)
    k, k2 = PK._pack(c, d, bt), PK._pack(c2, d2, bt)
    psel, n_sel, sel_units, own_sel = _packed_selector(c, d, bt)
    own_sel = _put(d, own_sel.contiguous())
    for lam in lambdas:
        names = OUT if lam > 0 else ('mtd', 'mask', 'tgt')
        o = _double_padded(c, d, lam, sel)
        assert o.rc == 0 and int(o.cnt[0]) == 0
        assert np.array_equal(o.picks.cpu().numpy(), picks_ref)
        ref = LK._call_padded(c2, d2, lam)                                      # the parent's lambda form (lam 0: its one-step bits)
        assert ref.rc == 0
        _same(o, ref, names, what=('padded', lam))
        if lam == 0.0:
            mtd0, mask0, bad0 = P._forward(c2, d2)                              # the parent's one-step entry point
            assert bad0 == 0 and np.array_equal(_bits(mtd0), _bits(o.mtd)) and np.array_equal(_bits(mask0), _bits(o.mask))
        again = _double_padded(c, d, lam, sel)                                  # a second launch: identical bits
        _same(again, o, names, what=('again', lam))
        assert torch.equal(again.picks, o.picks)
        bare = _double_padded(c, d, lam, sel, picks=False, tgt=None)            # d_picks and d_targets may be NULL
        assert bare.rc == 0 and bool((bare.tgt == SENT).all())
        _same(bare, o, ('mtd', 'mask'), what=('bare', lam))
        # ---- the packed form on the same episodes, longest first: slot for slot the padded result
        p = _double_packed(c, d, k, lam, psel, n_sel, sel_units)
        assert p.rc == 0 and int(p.cnt[0]) == 0
        _same(p, o, names, rows, what=('packed', lam))
        assert np.array_equal(p.picks.cpu().numpy(), picks_ref[rows])
        _same(p, LK._call_packed(c2, d2, k2, lam), names, what=('packed against the parent', lam))
        if lam == 0.0:
            one = PK._run_packed(c2, d2, k2)
            assert np.array_equal(_bits(one.mtd), _bits(p.mtd)) and np.array_equal(_bits(one.mask), _bits(p.mask))
        again = _double_packed(c, d, k, lam, psel, n_sel, sel_units)
        _same(again, p, names, what=('packed again', lam))
        assert torch.equal(again.picks, p.picks)
        own = _double_packed(c, d, k, lam, own_sel, k.U, None, picks=False)    # d_sel_units NULL: unit j selects for unit j
        assert own.rc == 0
        _same(own, p, names, what=('d_sel_units NULL', lam))


@pytest.mark.parametrize('combo', [COMBOS[3][0], COMBOS[2][0], COMBOS[0][0]], ids=[IDS[3], IDS[2], IDS[0]])
def test_selector_equal_to_the_target_gives_the_bits_of_the_existing_entry_points(combo):
    c = LK._case(combo, 'real')                                                 # finite Q values
    d = P._to_gpu(c)
    bt = PK._units(c)
    k = PK._pack(c, d, bt)
    rows = np.array([b * c.T + t for b, t in bt], np.int64)
    avail, q_t = c.avail.numpy()[:, :c.T], c.q_t.permute(1, 0, 2, 3).numpy()
    own = double_pick_reference(q_t, q_t, avail, np.float32)[0].reshape(c.R, c.n)
    for lam in LAMBDAS:
        names = OUT if lam > 0 else ('mtd', 'mask', 'tgt')
        o = _double_padded(c, d, lam, d.q_t)
        assert o.rc == 0
        _same(o, LK._call_padded(c, d, lam), names, what=('padded', lam))
        assert np.array_equal(o.picks.cpu().numpy(), own)
        p = _double_packed(c, d, k, lam, k.q_t, k.U, None)
        assert p.rc == 0
        _same(p, LK._call_packed(c, d, k, lam), names, what=('packed', lam))
        assert np.array_equal(p.picks.cpu().numpy(), own[rows])
        if lam == 0.0:
            mtd0, mask0, _ = P._forward(c, d)
            assert np.array_equal(_bits(mtd0), _bits(o.mtd)) and np.array_equal(_bits(mask0), _bits(o.mask))


@pytest.mark.parametrize('where', ['low', 'high'])
def test_a_selector_unit_outside_its_tensor_is_never_an_index(where):
    """One d_sel_units entry outside [0, n_sel_units): that row's picks are -1, its d_mtd NaN (under lambda its d_q_tot_eval too), the
    counter reads 1 -- also when the row's action is bad as well --, its target q_tot is the one its own target rows select (the value
    of the existing entry point), every other row keeps its bits at lambda 0, and the guards stay intact."""
    c = _case((5, 7, 4, 32, 5, 'ring'))
    d = P._to_gpu(c)
    bt = PK._units(c)
    k = PK._pack(c, d, bt)
    psel, n_sel, sel_units, _ = _packed_selector(c, d, bt)
    j = 5
    b, t = bt[j]
    assert not bool(c.padded[b, t, 0]) and 0 <= int(c.u[b, t, 0, 0]) < c.A
    units = sel_units.cpu().clone()
    units[j] = -1 if where == 'low' else n_sel
    bad_units = _put(d, units)
    keep = np.arange(k.U) != j
    base = _double_packed(c, d, k, 0.0, psel, n_sel, sel_units)
    o = _double_packed(c, d, k, 0.0, psel, n_sel, bad_units)
    assert o.rc == 0 and int(o.cnt[0]) == 1
    assert bool((o.picks[j] == -1).all()) and bool(torch.isnan(o.mtd[j]))
    for name in ('mtd', 'mask', 'tgt'):
        assert np.array_equal(_bits(getattr(o, name))[keep], _bits(getattr(base, name))[keep]), name
    assert torch.equal(o.picks.cpu()[keep], base.picks.cpu()[keep]) and float(o.mask[j]) == 1.0
    parent = LK._call_packed(c, d, k, 0.8)                                     # the row's own target rows select
    lam = _double_packed(c, d, k, 0.8, psel, n_sel, bad_units)
    assert lam.rc == 0 and int(lam.cnt[0]) == 1 and bool((lam.picks[j] == -1).all())
    assert bool(torch.isnan(lam.mtd[j])) and bool(torch.isnan(lam.tot_e[j]))
    assert np.array_equal(_bits(lam.tot_t[j:j + 1]), _bits(parent.tot_t[j:j + 1])) and bool(torch.isfinite(lam.tot_t).all())
    assert int(torch.isnan(lam.mtd).sum()) == 1 and int(torch.isnan(lam.tot_e).sum()) == 1
    null_counter = _double_packed(c, d, k, 0.0, psel, n_sel, bad_units, cnt=None)
    assert null_counter.rc == 0 and np.array_equal(_bits(null_counter.mtd), _bits(o.mtd))
    # a bad action in the same row: still counted once
    c.u[b, t, 0, 0] = c.A
    d = P._to_gpu(c)
    k = PK._pack(c, d, bt)
    psel, n_sel, sel_units, _ = _packed_selector(c, d, bt)
    both = _double_packed(c, d, k, 0.0, psel, n_sel, _put(d, units))
    assert both.rc == 0 and int(both.cnt[0]) == 1 and bool(torch.isnan(both.mtd[j])) and int(torch.isnan(both.mtd).sum()) == 1
    alone = _double_packed(c, d, k, 0.0, psel, n_sel, sel_units)               # the bad action alone: counted, picks still written
    assert alone.rc == 0 and int(alone.cnt[0]) == 1 and bool(torch.isnan(alone.mtd[j])) and bool((alone.picks[j] >= 0).all())


def _all_untouched(o):
    for name in OUT:
        assert bool(torch.isnan(getattr(o, name)).all()), name
    assert int(o.cnt[0]) == 0 and bool((o.picks == PICK_SENT).all())


def test_argument_errors_come_back_before_any_launch():
    """QMIX_ERR_BAD_ARG with every NaN-filled output untouched: what the entry point of the same form and lambda refuses, d_q_sel NULL,
    n_sel_units < 1, d_sel_units NULL with n_sel_units < n_units, lam outside [0, 1] or NaN; QMIX_ERR_UNSUPPORTED outside the build
    limits.  What only the lambda forms refuse is accepted at lam == 0."""
    nan = float('nan')
    c = _case((5, 7, 4, 32, 5, 'ring'))
    d = P._to_gpu(c)
    sel = _put(d, c.q_sel)
    big = MAX_T + 1
    one_step = [dict(qe=None), dict(qt=None), dict(u=None), dict(r=None), dict(avail=None), dict(term=None), dict(padded=None), dict(pe=None),
                dict(pt=None), dict(mtd=None), dict(mask=None), dict(ev=None), dict(tg=None), dict(B=0), dict(T=0), dict(n=0), dict(A=0),
                dict(Tl=c.T - 1), dict(pe_rows=c.T - 1), dict(pt_off=-1), dict(pe_off=2), dict(sel=None)]
    lam_only = [dict(T=big, Tl=big + 3, pe_rows=big + 1, pt_rows=big + 1), dict(tot_e=None), dict(tot_t=None)]
    for lam, cases in ((0.0, one_step), (0.8, one_step + lam_only)):
        for over in cases + [dict(lam=-0.01), dict(lam=1.5), dict(lam=nan), dict(lam=float('inf'))]:
            o = _double_padded(c, d, lam, sel, fill=nan, **dict(over))
            assert o.rc == BAD_ARG, (lam, over)
            _all_untouched(o)
        for over in (dict(H=16), dict(M=64), dict(n=17), dict(A=17)):
            o = _double_padded(c, d, lam, sel, fill=nan, **over)
            assert o.rc == UNSUPPORTED, (lam, over)
            _all_untouched(o)
    for over in lam_only[1:]:                                   # the hand-off is not read at lam == 0
        o = _double_padded(c, d, 0.0, sel, **over)
        assert o.rc == 0 and np.array_equal(o.picks.cpu().numpy(), c.picks.reshape(c.R, c.n)), over
    bt = PK._units(c)
    k = PK._pack(c, d, bt)
    psel, n_sel, sel_units, _ = _packed_selector(c, d, bt)
    counts = np.array(LK._counts(c))
    grow, neg, short = counts.copy(), counts.copy(), counts.copy()
    grow[1], grow[2] = grow[2] - 1, grow[1] + 1          # same total, but counts[2] > counts[1]
    assert grow.sum() == counts.sum() and grow[2] > grow[1]
    neg[-1] = -1
    short[0] += 1
    one_step = [dict(U=-1), dict(units=None), dict(qe=None), dict(qt=None), dict(u=None), dict(r=None), dict(avail=None), dict(term=None),
                dict(padded=None), dict(pe=None), dict(pt=None), dict(mtd=None), dict(mask=None), dict(ev=None), dict(tg=None), dict(n=0),
                dict(A=0), dict(sel=None), dict(n_sel=0), dict(n_sel=-3), dict(sel_units=None, n_sel=k.U - 1), dict(sel_units=None, n_sel=1)]
    lam_only = [dict(counts=np.ones(big, np.int32), U=big), dict(counts=grow), dict(counts=neg), dict(counts=short), dict(counts=counts[:-1]),
                dict(n_steps=-1), dict(tot_e=None), dict(tot_t=None)]
    for lam, cases in ((0.0, one_step), (0.8, one_step + lam_only)):
        for over in cases + [dict(lam=-0.01), dict(lam=1.5), dict(lam=nan)]:
            o = _double_packed(c, d, k, lam, psel, n_sel, sel_units, fill=nan, **dict(over))
            assert o.rc == BAD_ARG, (lam, over)
            _all_untouched(o)
        o = _double_packed(c, d, k, lam, psel, n_sel, sel_units, fill=nan, H=16)
        assert o.rc == UNSUPPORTED
        _all_untouched(o)
        o = _double_packed(c, d, k, lam, psel, n_sel, sel_units, fill=nan, U=0, counts=[])      # no units: accepted, nothing launched
        assert o.rc == 0
        _all_untouched(o)
    o = _null_counts_call(c, d, k, psel, n_sel, sel_units, 0.8, nan)
    assert o.rc == BAD_ARG
    _all_untouched(o)
    base = _double_packed(c, d, k, 0.0, psel, n_sel, sel_units)
    for over in (dict(counts=grow), dict(counts=neg), dict(n_steps=-1), dict(tot_e=None), dict(tot_t=None)):   # not read at lam == 0
        o = _double_packed(c, d, k, 0.0, psel, n_sel, sel_units, **over)
        assert o.rc == 0 and np.array_equal(_bits(o.mtd), _bits(base.mtd)), over
    o = _null_counts_call(c, d, k, psel, n_sel, sel_units, 0.0, SENT)
    assert o.rc == 0 and np.array_equal(_bits(o.mtd), _bits(base.mtd))


def _null_counts_call(c, d, k, sel, n_sel, sel_units, lam, fill):
    p = P._p
    o = _outputs(d, k.U, c.n, fill)
    o.rc = P._lib().qmix_double().qmix_mix_td_double_forward_packed(
        p(k.q_e), p(k.q_t), p(k.units), k.U, p(d.u), p(d.r), p(d.avail), p(d.term), p(d.padded), c.n, c.A, p(k.pe), p(k.pt), p(k.trow), c.H,
        K.M, C.byref(d.mix_e), C.byref(d.mix_t), c.gamma, p(o.mtd), p(o.mask), p(o.cnt), lam, p(o.tot_e), p(o.tot_t), p(o.tgt), len(LK._counts(c)),
        None, p(sel), n_sel, p(sel_units), p(o.picks), None)
    return _finish(d, o, fill, lam)


def test_every_declared_function_is_exported_with_its_arity():
    L = P._lib()
    declared = _prototypes('qmix_double.h')
    table = L.SIGNATURES['qmix_double']
    assert sorted(declared) == sorted(table) == ['qmix_mix_td_double_forward', 'qmix_mix_td_double_forward_packed']
    assert L._FILE['qmix_double'] == 'qmix_ops'
    raw = L.qmix_double()
    for name, n in declared.items():
        assert len(table[name]) == n and len(getattr(raw, name).argtypes) == n, name
