"""The mixing + TD block of the QMIX learn on lambda-returns through its C ABI (include/qmix_lambda.h: qmix_mix_td_lambda_forward and
qmix_mix_td_lambda_forward_packed; csrc/qmix_ops.hip: k_mix_forward<H, Index, true>, csrc/qmix_lambda_kernels.h: the walk).

  the walk      from the kernel's OWN d_q_tot_eval / d_q_tot_target the float32 numpy statement of the rule
                (marl_dmfb_amd.policy.td_lambda.lambda_targets_reference) and mask * (e - G) equal d_targets and d_mtd BIT FOR BIT
                in every slot, padded ones included, at lambda 0, 0.5, 0.8 and 1: the kernel does the same float32 operations in
                the same order (the library is built with -ffp-contract=off)
  the rows      the two q_tot outputs against the float64 mixer of tests/qmix_kernel_cases.py: value for value on the exact
                integer cases; on the real cases |q_tot - q_tot64| <= C_F x the row's value in the absolute run, the scale and the
                constant by which forward_ratio bounds mtd (C_F: four times the CPU yardstick; nothing is read off the kernels)
  lambda 0      mtd and mask have the bits of qmix_mix_td_forward / qmix_mix_td_forward_packed
  packed        slot for slot the padded result on a length-sorted draw;  a second launch gives the same bits
  shapes        (B, T) = (1, 1), (1, 2), (3, 11), (5, 7): idle waves and a second workgroup of the walk; (2, 65): the lane stride
                wraps; (2, 512): QMIX_LAMBDA_MAX_T; 31 / 32 / 33 rows for the rows launch; both H, n in {1, 4, 16}, A in {1, 5, 16}
  episodes      the tests write `padded` and `terminated` themselves: L = T, 1, 0, T-1 and between, the last valid step terminated
                or not, a step terminated in mid-episode, random flags and rewards in the padded slots
  bad actions, every QMIX_ERR_BAD_ARG case of the header with NaN-filled outputs left untouched, and the exports.

Every buffer sits between guard regions (front_kernel_cases.guarded)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import qmix_kernel_cases as K
import test_gpu_qmix_kernels as P
import test_gpu_qmix_packed_kernels as PK
from marl_dmfb_amd.policy.td_lambda import lambda_targets_reference
from test_cabi_exports import _prototypes

pytestmark = pytest.mark.gpu

SENT = P.SENT
BAD_ARG, UNSUPPORTED = -1, -6
LAMBDAS = [0.0, 0.5, 0.8, 1.0]
MAX_T = 512
# (B, T, n, H, A, layout); (n, H) are pairs of K.RECIPE
COMBOS = [(1, 1, 1, 24, 1, 'ring'), (1, 2, 4, 32, 5, 'sep'), (3, 11, 16, 24, 16, 'wide'), (5, 7, 4, 32, 5, 'ring'),
          (2, 65, 1, 24, 5, 'sep'), (2, MAX_T, 4, 32, 5, 'ring'), (31, 1, 16, 32, 16, 'sep'), (4, 8, 1, 24, 16, 'wide'),
          (3, 11, 4, 32, 1, 'ring')]
IDS = ['B%d_T%d_n%d_H%d_A%d_%s' % c for c in COMBOS]
assert {c[0] * c[1] for c in COMBOS} >= {31, 32, 33} and {c[3] for c in COMBOS} == {24, 32}
assert {c[2] for c in COMBOS} == {1, 4, 16} and {c[4] for c in COMBOS} == {1, 5, 16}


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _lens(B, T):
    """Leading valid steps per episode: T, 1, 0, T-1, T // 2, then random ones."""
    rng = np.random.default_rng(977 * B + T)
    return np.concatenate([[T, 1, 0, T - 1, T // 2], rng.integers(0, T + 1, max(0, B - 5))])[:B].astype(np.int64)


def _case(combo, kind):
    """K.make_case with `padded` and `terminated` written here.  The q_tot of a row do not depend on either, so K.reference (which
    rebuilds the case from its key) still holds their float64 values."""
    c = K.make_case(*combo, kind)
    B, T, Tl = c.B, c.T, c.Tl
    rng = np.random.default_rng(31 * B + T + (kind == 'exact'))
    lens = _lens(B, T)
    steps = np.arange(Tl)[None, :]
    padded = steps >= lens[:, None]
    term = rng.random((B, Tl)) < 0.1                          # here and there in mid-episode
    term[padded] = rng.random(int(padded.sum())) < 0.5        # anything in the padded slots
    for b in range(B):
        if lens[b] >= 1:
            term[b, lens[b] - 1] = b % 2 == 1                 # the last valid step: terminated in every other episode
    if T >= 3:
        term[0, T // 2 - 1] = True                            # the longest episode: terminated in its middle, valid steps behind
    c.lens = lens
    c.padded = torch.as_tensor(padded.astype(np.uint8)).unsqueeze(-1)
    c.term = torch.as_tensor(term.astype(np.uint8)).unsqueeze(-1)
    return c


def _args_padded(c, d, o, lam):
    p = P._p
    return dict(qe=p(d.q_e), qt=p(d.q_t), u=p(d.u), r=p(d.r), avail=p(d.avail), term=p(d.term), padded=p(d.padded), B=c.B, T=c.T, Tl=c.Tl,
                n=c.n, A=c.A, pe=p(d.pe), pe_rows=c.pe_rows, pe_off=c.pe_off, pt=p(d.pt), pt_rows=c.pt_rows, pt_off=c.pt_off, H=c.H, M=K.M,
                ev=C.byref(d.mix_e), tg=C.byref(d.mix_t), gamma=c.gamma, mtd=p(o.mtd), mask=p(o.mask), cnt=p(o.cnt), lam=lam,
                tot_e=p(o.tot_e), tot_t=p(o.tot_t), tgt=p(o.tgt))


def _outputs(d, rows, fill):
    o = types.SimpleNamespace(cnt=P._out(d, (1,), 0, torch.int32))
    for name in ('mtd', 'mask', 'tgt', 'tot_e', 'tot_t'):
        setattr(o, name, P._out(d, (rows,), fill))
    return o


def _finish(d, o, fill):
    torch.cuda.synchronize()
    for chk in d.checks:
        chk()
    if o.rc == 0:
        for name in ('mtd', 'mask', 'tot_e', 'tot_t'):
            assert not bool((getattr(o, name) == fill).any()), (name, 'an output element was left unwritten')
    return o


def _call_padded(c, d, lam, fill=SENT, **over):
    """One call of the padded entry point on fresh sentinel-filled outputs."""
    o = _outputs(d, c.R, fill)
    a = _args_padded(c, d, o, lam)
    a.update(over)
    o.rc = P._lib().qmix_lambda().qmix_mix_td_lambda_forward(
        a['qe'], a['qt'], a['u'], a['r'], a['avail'], a['term'], a['padded'], a['B'], a['T'], a['Tl'], a['n'], a['A'], a['pe'], a['pe_rows'],
        a['pe_off'], a['pt'], a['pt_rows'], a['pt_off'], a['H'], a['M'], a['ev'], a['tg'], a['gamma'], a['mtd'], a['mask'], a['cnt'], a['lam'],
        a['tot_e'], a['tot_t'], a['tgt'], None)
    return _finish(d, o, fill)


def _counts(c):
    return [int((c.lens > t).sum()) for t in range(int(c.lens.max()))]


def _call_packed(c, d, k, lam, fill=SENT, **over):
    """One call of the packed entry point on the units `k` (PK._pack) on fresh sentinel-filled outputs."""
    p = P._p
    o = _outputs(d, max(k.U, 1), fill)
    counts = over.pop('counts', _counts(c))
    a = dict(qe=p(k.q_e), qt=p(k.q_t), units=p(k.units), U=k.U, u=p(d.u), r=p(d.r), avail=p(d.avail), term=p(d.term), padded=p(d.padded),
             n=c.n, A=c.A, pe=p(k.pe), pt=p(k.pt), trow=p(k.trow), H=c.H, M=K.M, ev=C.byref(d.mix_e), tg=C.byref(d.mix_t), gamma=c.gamma,
             mtd=p(o.mtd), mask=p(o.mask), cnt=p(o.cnt), lam=lam, tot_e=p(o.tot_e), tot_t=p(o.tot_t), tgt=p(o.tgt),
             n_steps=len(counts), counts=(C.c_int32 * max(1, len(counts)))(*[int(x) for x in counts]))
    a.update(over)
    o.rc = P._lib().qmix_lambda().qmix_mix_td_lambda_forward_packed(
        a['qe'], a['qt'], a['units'], a['U'], a['u'], a['r'], a['avail'], a['term'], a['padded'], a['n'], a['A'], a['pe'], a['pt'], a['trow'],
        a['H'], a['M'], a['ev'], a['tg'], a['gamma'], a['mtd'], a['mask'], a['cnt'], a['lam'], a['tot_e'], a['tot_t'], a['tgt'],
        a['n_steps'], a['counts'], None)
    return _finish(d, o, fill)


def _rule(c, o, lam):
    """(mtd, mask, G) float32 (B, T) of the rule from the call's own q_tot outputs."""
    B, T = c.B, c.T
    e = o.tot_e.cpu().numpy().reshape(B, T)
    q = o.tot_t.cpu().numpy().reshape(B, T)
    pad, term = c.padded[:, :T, 0].numpy(), c.term[:, :T, 0].numpy()
    G = lambda_targets_reference(q, c.r[:, :T, 0].numpy(), term, pad, c.gamma, lam, np.float32)
    mask = np.float32(1) - pad.astype(np.float32)
    with np.errstate(invalid='ignore'):
        mtd = mask * (e - G)
    assert G.dtype == np.float32 and mtd.dtype == np.float32
    return mtd, mask, G


def _check_totals(c, o):
    """d_q_tot_eval / d_q_tot_target against the float64 mixer."""
    r, a = K.reference(c), K.reference(c, absolute=True)
    for name in ('tot_e', 'tot_t'):
        got, want, scale = getattr(o, name).cpu().double(), getattr(r, name), getattr(a, name)
        if c.kind == 'exact':
            assert torch.equal(got, want), (name, int((got != want).sum()))
        else:
            err = (got - want).abs()
            assert bool((err[scale == 0] == 0).all()), (name, 'a row of scale 0 is not exactly 0')
            ratio = float((err / scale.clamp_min(1e-300)).max())
            print('ratio %s %s %.3e (C_F %.3e)' % (c.key, name, ratio, K.C_F))
            assert ratio <= K.C_F, (name, ratio)


@pytest.mark.parametrize('kind', ['exact', 'real'])
@pytest.mark.parametrize('combo', COMBOS, ids=IDS)
def test_every_slot_equals_the_float32_rule_bit_for_bit(combo, kind):
    c = _case(combo, kind)
    d = P._to_gpu(c)
    bt = PK._units(c)
    assert len(bt) == int(c.lens.sum())
    k = PK._pack(c, d, bt) if bt else None
    rows = np.array([b * c.T + t for b, t in bt], np.int64)
    for lam in LAMBDAS:
        o = _call_padded(c, d, lam)
        assert o.rc == 0 and int(o.cnt[0]) == 0
        if lam == LAMBDAS[0]:
            _check_totals(c, o)
            first = o
        else:                                        # the rows launch does not depend on lambda
            assert torch.equal(o.tot_e.view(torch.int32), first.tot_e.view(torch.int32)) and torch.equal(o.tot_t, first.tot_t)
        want_mtd, want_mask, want_G = _rule(c, o, lam)
        got = {name: getattr(o, name).cpu().numpy().reshape(c.B, c.T) for name in ('mtd', 'mask', 'tgt')}
        for name, w_ in (('mtd', want_mtd), ('mask', want_mask), ('tgt', want_G)):
            assert np.array_equal(_bits(got[name]), _bits(w_)), (name, lam, float(np.nanmax(np.abs(got[name] - w_))))
        again = _call_padded(c, d, lam)                                        # two launches, identical bits
        for name in ('mtd', 'mask', 'tgt', 'tot_e', 'tot_t'):
            assert torch.equal(getattr(again, name).view(torch.int32), getattr(o, name).view(torch.int32)), name
        no_tgt = _call_padded(c, d, lam, tgt=None)                             # d_targets may be NULL
        assert no_tgt.rc == 0 and torch.equal(no_tgt.mtd.view(torch.int32), o.mtd.view(torch.int32)) and bool((no_tgt.tgt == SENT).all())
        if lam == 0.0:                                                         # the one-step entry point, bit for bit
            mtd0, mask0, bad0 = P._forward(c, d)
            assert bad0 == 0 and torch.equal(mtd0.view(torch.int32), o.mtd.view(torch.int32)) and torch.equal(mask0, o.mask)
        if k is None:
            continue
        # ---- the packed form on the same episodes, longest first: slot for slot the padded result
        p = _call_packed(c, d, k, lam)
        assert p.rc == 0 and int(p.cnt[0]) == 0
        for name in ('mtd', 'mask', 'tgt', 'tot_e', 'tot_t'):
            x, w_ = getattr(p, name).cpu().numpy(), getattr(o, name).cpu().numpy()[rows]
            assert np.array_equal(_bits(x), _bits(w_)), (name, lam)
        again = _call_packed(c, d, k, lam)
        for name in ('mtd', 'mask', 'tgt', 'tot_e', 'tot_t'):
            assert torch.equal(getattr(again, name).view(torch.int32), getattr(p, name).view(torch.int32)), name
        if lam == 0.0:
            one = PK._run_packed(c, d, k)
            assert torch.equal(one.mtd.view(torch.int32), p.mtd.cpu().view(torch.int32)) and torch.equal(one.mask, p.mask.cpu())


def test_case_patterns_hold_what_the_tests_claim():
    """The episode patterns written by `_case`: L = 0, 1, T-1 and T, a last valid step terminated and one that is not, a step
    terminated in mid-episode with valid steps behind it."""
    c = _case((5, 7, 4, 32, 5, 'ring'), 'real')
    assert c.lens.tolist()[:4] == [7, 1, 0, 6]
    term = c.term[:, :, 0].numpy()
    assert term[0, 2] == 1 and term[0, 6] == 0 and term[1, 0] == 1 and term[3, 5] == 1
    assert _counts(c)[0] == 4 and sum(_counts(c)) == int(c.lens.sum())
    assert _case((2, MAX_T, 4, 32, 5, 'ring'), 'real').lens.tolist() == [MAX_T, 1]


@pytest.mark.parametrize('combo', [COMBOS[3], COMBOS[2]], ids=[IDS[3], IDS[2]])
def test_bad_actions_poison_their_slots_only_and_are_counted(combo):
    """Actions outside [0, A) in two slots of one episode and one slot of another: NaN exactly there in d_mtd and d_q_tot_eval, every
    other slot and every target with the bits of the run without them (G does not read u), the counter reads 3; in both forms, and
    with a NULL counter."""
    c = _case(combo, 'real')
    lam = 0.8
    d = P._to_gpu(c)
    base = _call_padded(c, d, lam)
    hit = [(0, 0, c.n - 1), (0, c.T - 1, 0), (1, 0, c.n // 2)]           # (episode, step, agent): valid steps (lens = T, 1, ...)
    for (b, t, i), value in zip(hit, (c.A, -1, 127)):
        c.u[b, t, i, 0] = value
    poisoned = torch.zeros((c.B, c.T), dtype=torch.bool)
    for b, t, _ in hit:
        poisoned[b, t] = True
    poisoned = poisoned.reshape(-1)
    d = P._to_gpu(c)
    for counter in (True, False):
        o = _call_padded(c, d, lam, **({} if counter else {'cnt': None}))
        assert o.rc == 0 and int(o.cnt[0]) == (3 if counter else 0)
        for name in ('mtd', 'tot_e'):
            x = getattr(o, name).cpu()
            assert torch.equal(torch.isnan(x), poisoned), name
            assert torch.equal(x[~poisoned].view(torch.int32), getattr(base, name).cpu()[~poisoned].view(torch.int32)), name
        for name in ('mask', 'tgt', 'tot_t'):
            assert torch.equal(getattr(o, name).view(torch.int32), getattr(base, name).view(torch.int32)), name
    bt = PK._units(c)
    rows = torch.tensor([b * c.T + t for b, t in bt])
    k = PK._pack(c, d, bt)
    for counter in (True, False):
        p = _call_packed(c, d, k, lam, **({} if counter else {'cnt': None}))
        assert p.rc == 0 and int(p.cnt[0]) == (3 if counter else 0)
        for name in ('mtd', 'tot_e'):
            x = getattr(p, name).cpu()
            assert torch.equal(torch.isnan(x), poisoned[rows]), name
            keep = ~poisoned[rows]
            assert torch.equal(x[keep].view(torch.int32), getattr(base, name).cpu()[rows][keep].view(torch.int32)), name
        for name in ('mask', 'tgt', 'tot_t'):
            assert torch.equal(getattr(p, name).cpu().view(torch.int32), getattr(base, name).cpu()[rows].view(torch.int32)), name


def _all_untouched(o):
    for name in ('mtd', 'mask', 'tgt', 'tot_e', 'tot_t'):
        assert bool(torch.isnan(getattr(o, name)).all()), name
    assert int(o.cnt[0]) == 0


def test_argument_errors_come_back_before_any_launch():
    """QMIX_ERR_BAD_ARG with every NaN-filled output untouched: lam outside [0, 1] or NaN, T / n_steps above QMIX_LAMBDA_MAX_T, counts
    that grow, are negative or do not sum to n_units, NULL required pointers, and what the one-step entry points refuse (outside the
    build limits: QMIX_ERR_UNSUPPORTED, as there)."""
    nan = float('nan')
    c = _case((5, 7, 4, 32, 5, 'ring'), 'real')
    d = P._to_gpu(c)
    big = MAX_T + 1
    cases = [dict(lam=-0.01), dict(lam=1.5), dict(lam=nan), dict(lam=float('inf')),
             dict(T=big, Tl=big + 3, pe_rows=big + 1, pt_rows=big + 1), dict(tot_e=None), dict(tot_t=None), dict(qe=None), dict(qt=None),
             dict(u=None), dict(r=None), dict(avail=None), dict(term=None), dict(padded=None), dict(pe=None), dict(pt=None), dict(mtd=None),
             dict(mask=None), dict(ev=None), dict(tg=None), dict(B=0), dict(T=0), dict(n=0), dict(A=0), dict(Tl=c.T - 1),
             dict(pe_rows=c.T - 1), dict(pt_off=-1), dict(pe_off=2)]
    for over in cases:
        o = _call_padded(c, d, over.pop('lam', 0.8), fill=nan, **over)
        assert o.rc == BAD_ARG, over
        _all_untouched(o)
    for over in (dict(H=16), dict(M=64), dict(n=17), dict(A=17)):
        o = _call_padded(c, d, 0.8, fill=nan, **over)
        assert o.rc == UNSUPPORTED, over
        _all_untouched(o)
    bt = PK._units(c)
    k = PK._pack(c, d, bt)
    counts = np.array(_counts(c))
    grow, neg, short = counts.copy(), counts.copy(), counts.copy()
    grow[1], grow[2] = grow[2] - 1, grow[1] + 1          # same total, but counts[2] > counts[1]
    assert grow.sum() == counts.sum() and grow[2] > grow[1]
    neg[-1] = -1
    short[0] += 1
    cases = [dict(lam=-0.01), dict(lam=1.5), dict(lam=nan), dict(counts=np.ones(big, np.int32), U=big), dict(counts=grow), dict(counts=neg),
             dict(counts=short), dict(counts=counts[:-1]), dict(n_steps=-1), dict(U=-1),
             dict(units=None), dict(qe=None), dict(qt=None), dict(padded=None), dict(pe=None), dict(pt=None), dict(mtd=None), dict(mask=None),
             dict(tot_e=None), dict(tot_t=None), dict(ev=None), dict(n=0)]
    for over in cases:
        o = _call_packed(c, d, k, over.pop('lam', 0.8), fill=nan, **over)
        assert o.rc == BAD_ARG, over
        _all_untouched(o)
    o = _null_counts_call(c, d, k, len(counts), nan)
    assert o.rc == BAD_ARG
    _all_untouched(o)
    o = _call_packed(c, d, k, 0.8, fill=nan, H=16)
    assert o.rc == UNSUPPORTED
    _all_untouched(o)
    # no units: accepted, nothing launched
    o = _call_packed(c, d, k, 0.8, fill=nan, U=0, counts=[])
    assert o.rc == 0
    _all_untouched(o)


def _null_counts_call(c, d, k, n_steps, fill):
    p = P._p
    o = _outputs(d, k.U, fill)
    o.rc = P._lib().qmix_lambda().qmix_mix_td_lambda_forward_packed(
        p(k.q_e), p(k.q_t), p(k.units), k.U, p(d.u), p(d.r), p(d.avail), p(d.term), p(d.padded), c.n, c.A, p(k.pe), p(k.pt), p(k.trow), c.H,
        K.M, C.byref(d.mix_e), C.byref(d.mix_t), c.gamma, p(o.mtd), p(o.mask), p(o.cnt), 0.8, p(o.tot_e), p(o.tot_t), p(o.tgt), n_steps,
        None, None)
    return _finish(d, o, fill)


def test_every_declared_function_is_exported_with_its_arity():
    L = P._lib()
    declared = _prototypes('qmix_lambda.h')
    table = L.SIGNATURES['qmix_lambda']
    assert sorted(declared) == sorted(table) == ['qmix_mix_td_lambda_forward', 'qmix_mix_td_lambda_forward_packed']
    assert L._FILE['qmix_lambda'] == 'qmix_ops'
    raw = L.qmix_lambda()
    for name, n in declared.items():
        assert len(table[name]) == n and len(getattr(raw, name).argtypes) == n, name
