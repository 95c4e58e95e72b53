"""The QMIX mixing + TD kernels (csrc/qmix_ops.hip: k_mix_forward<24|32>, k_mix_backward<24|32>) through their C ABI
(include/qmix_ops.h), every output row by row against the float64 reference of tests/qmix_kernel_cases.py:

  exact cases   small integers on which float32 is exact: mtd, mask, grad_q, grad_p, Z and X equal the reference value for value,
                ties of relu, |.| and elu included, every element of a written area is written, a second launch gives the same bits
  real cases    |mtd - mtd64| <= C_F * scale_row per element; for grad_q, grad_p and Z the L2 error of every row that holds no near
                tie <= C_B * the L2 of that row's absolute-run values; X exact; the project's whole-tensor GRAD_TOL as well
  row counts    1, 31, 32, 33, 259 and 2049 rows (32 rows per workgroup), n from 1 to 16, A from 1 to 16, both H, three P layouts;
                rows of grad_p outside steps [0, T) keep their fill
  bad actions, d_bad_actions == NULL, *d_grad_num != 1, and QMIX._mix_td_fused with s / s_next as separate tensors.

The bounds C_F and C_B are four times what a float32 evaluation of the same formulas gives on the CPU
(tests/test_qmix_kernel_cases.py); nothing was read off the kernels.  Every buffer sits between guard regions
(front_kernel_cases.guarded: NaN around the float inputs, so a read outside one shows in the result)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import qmix_kernel_cases as K
from front_kernel_cases import guarded

pytestmark = pytest.mark.gpu

SENT = -777.125      # no multiple of 1/4: no output of an exact case can take this value
DEV = 'cuda'


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _lib():
    from marl_dmfb_amd import _lib
    return _lib


def _put(t):
    """A copy of CPU tensor `t` on the GPU inside guard regions -> (tensor, check)."""
    view, check = guarded(tuple(t.shape), t.dtype, 0, DEV)
    view.copy_(t)
    return view, check


def _to_gpu(c):
    """The inputs of case `c` on the GPU -> namespace with .checks (the guard checks of every buffer)."""
    d = types.SimpleNamespace(checks=[])

    def put(t):
        v, chk = _put(t)
        d.checks.append(chk)
        return v
    for k in ('q_e', 'q_t', 'u', 'r', 'avail', 'term', 'padded', 'pe'):
        setattr(d, k, put(getattr(c, k)))
    d.pt = d.pe if c.shared else put(c.pt)
    d.ev, d.tg = [put(t) for t in c.ev], [put(t) for t in c.tg]
    L = _lib()
    d.mix_e = L.QmixMixer(*[t.data_ptr() for t in d.ev])
    d.mix_t = L.QmixMixer(*[t.data_ptr() for t in d.tg])
    return d


def _out(d, shape, fill=SENT, dtype=torch.float32):
    v, chk = guarded(shape, dtype, fill, DEV)
    d.checks.append(chk)
    return v


def _forward(c, d, counter=True):
    lib = _lib().qmix_ops()
    mtd, mask = _out(d, (c.R,)), _out(d, (c.R,))
    cnt = _out(d, (1,), 0, torch.int32)
    rc = lib.qmix_mix_td_forward(_p(d.q_e), _p(d.q_t), _p(d.u), _p(d.r), _p(d.avail), _p(d.term), _p(d.padded), c.B, c.T, c.Tl, c.n, c.A,
                                 _p(d.pe), c.pe_rows, c.pe_off, _p(d.pt), c.pt_rows, c.pt_off, c.H, K.M, C.byref(d.mix_e),
                                 C.byref(d.mix_t), c.gamma, _p(mtd), _p(mask), _p(cnt) if counter else None, None)
    assert rc == 0
    torch.cuda.synchronize()
    for chk in d.checks:
        chk()
    assert not bool((mtd == SENT).any()) and not bool((mask == SENT).any()), 'an output element was left unwritten'
    return mtd, mask, int(cnt[0])


def _backward(c, d, mtd, mask, g0):
    lib = _lib().qmix_ops()
    o = types.SimpleNamespace()
    o.grad_q = _out(d, (c.T, c.B, c.n, c.A))
    o.grad_p = _out(d, (c.B, c.pe_rows, K.f_cols(c.H)))
    o.Z = _out(d, (c.R, K.z_cols(c.n)))
    o.X = _out(d, (c.R, K.x_cols(c.H)))
    gnum = _out(d, (1,), g0)
    rc = lib.qmix_mix_td_backward(_p(mtd), _p(mask), _p(d.q_e), _p(d.u), c.B, c.T, c.Tl, c.n, c.A, _p(d.pe), c.pe_rows, c.pe_off, c.H, K.M,
                                  C.byref(d.mix_e), _p(gnum), _p(o.grad_q), _p(o.grad_p), _p(o.Z), _p(o.X), None)
    assert rc == 0
    torch.cuda.synchronize()
    for chk in d.checks:
        chk()
    # every element of a written area is written; the rows of grad_p outside steps [0, T) keep their fill
    inside = torch.zeros(c.pe_rows, dtype=torch.bool, device=DEV)
    inside[c.pe_off:c.pe_off + c.T] = True
    assert bool((o.grad_p[:, ~inside] == SENT).all()), 'a row of grad_p outside steps [0, T) was written'
    for name, t in (('grad_q', o.grad_q), ('grad_p', o.grad_p[:, inside]), ('Z', o.Z), ('X', o.X)):
        assert not bool((t == SENT).any()), (name, 'an output element was left unwritten')
    return o


def _run(c, d=None, g0=None, counter=True):
    """Forward, then the backward on the forward's own mtd / mask, as _MixTD does -> CPU outputs."""
    d = _to_gpu(c) if d is None else d
    mtd, mask, bad = _forward(c, d, counter)
    o = _backward(c, d, mtd, mask, c.g0 if g0 is None else g0)
    out = types.SimpleNamespace(mtd=mtd.cpu(), mask=mask.cpu(), bad=bad)
    for name in ('grad_q', 'grad_p', 'Z', 'X'):
        setattr(out, name, getattr(o, name).cpu())
    out.grad_p = torch.where(out.grad_p == SENT, torch.zeros_like(out.grad_p), out.grad_p)    # untouched rows: no gradient
    return out


OUTPUTS = ('mtd', 'mask', 'grad_q', 'grad_p', 'Z', 'X')


def _same_bits(a, b, names=OUTPUTS):
    for name in names:
        assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name


@pytest.mark.parametrize('combo', K.COMBOS, ids=K.COMBO_IDS)
def test_exact_case_equals_float64(combo):
    c = K.case(combo, 'exact')
    r = K.reference(c)
    d = _to_gpu(c)
    out = _run(c, d)
    assert out.bad == 0
    for name in OUTPUTS:
        got, want = getattr(out, name).double(), getattr(r, name)
        diff = (got != want)
        assert not bool(diff.any()), (name, int(diff.sum()), 'first at', diff.nonzero()[0].tolist())
    _same_bits(out, _run(c, d))


@pytest.mark.parametrize('combo', K.COMBOS, ids=K.COMBO_IDS)
def test_real_case_row_by_row(combo):
    c = K.case(combo, 'real')
    _check_real(c, _run(c))


def _check_real(c, out, g0=None):
    r = K.reference(c, g0=g0)
    assert out.bad == 0
    assert torch.equal(out.mask.double(), r.mask)
    assert torch.equal(out.X.double(), r.X)                      # relu of the inputs and ones
    figures = {'mtd': K.forward_ratio(c, out.mtd, g0=g0)}
    keep = ~K.tie_rows(c)
    whole = {}
    for name in ('grad_q', 'grad_p', 'Z'):
        figures[name] = K.backward_ratio(c, name, getattr(out, name), g0=g0)
        got, want = K.row_view(c, name, getattr(out, name).double())[keep], K.row_view(c, name, getattr(r, name))[keep]
        whole[name] = float((got - want).norm() / (want.norm() + 1e-300))
    print('ratio %s g0=%s ties %.4f:' % (c.key, g0, float((~keep).double().mean())),
          ' '.join('%s %.3e' % kv for kv in figures.items()), '| whole', ' '.join('%s %.2e' % kv for kv in whole.items()))
    assert figures['mtd'] <= K.C_F, figures
    for name in ('grad_q', 'grad_p', 'Z'):
        assert figures[name] <= K.C_B, figures
        assert whole[name] < K.GRAD_TOL, whole


BAD_COMBO = (37, 7, 10, 32, 5, 'ring')


def test_bad_actions_poison_their_rows_only():
    """u = -128, -1, A and 127 in four rows, one of them in the last, ragged workgroup: those rows' mtd and every grad_q entry of
    them are NaN, the counter is 4, and every other row of every output has the bits of the same case without the bad actions."""
    c = K.case(BAD_COMBO, 'real')
    assert c.R == 259 and c.A == 5
    base = _run(c)
    rows = [0, 100, 200, 258]                                  # 258: the third row of the last group (rows 256..258)
    for k, (row, value) in enumerate(zip(rows, (-128, -1, c.A, 127))):
        c.u[row // c.T, row % c.T, (3 * k) % c.n, 0] = value
    d = _to_gpu(c)
    out = _run(c, d)
    assert out.bad == 4
    hit = torch.zeros(c.R, dtype=torch.bool)
    hit[rows] = True
    assert bool(torch.isnan(out.mtd[hit]).all()) and not bool(torch.isnan(out.mtd[~hit]).any())
    gq = K.row_view(c, 'grad_q', out.grad_q)
    assert bool(torch.isnan(gq[hit]).all()), 'a grad_q entry of a bad row is not NaN'
    assert torch.equal(out.mtd[~hit].view(torch.int32), base.mtd[~hit].view(torch.int32))
    assert torch.equal(out.mask.view(torch.int32), base.mask.view(torch.int32))
    for name in ('grad_q', 'grad_p', 'Z', 'X'):
        a, b = K.row_view(c, name, getattr(out, name))[~hit], K.row_view(c, name, getattr(base, name))[~hit]
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), name
    # without a counter: accepted, same mtd
    mtd, mask, cnt = _forward(c, d, counter=False)
    assert cnt == 0
    assert torch.equal(mtd.cpu().view(torch.int32), out.mtd.view(torch.int32))


def test_grad_num_scales_the_backward():
    """*d_grad_num = 1 / mask.sum(), what QMIX.learn passes: the same bounds."""
    c = K.case((37, 7, 4, 32, 9, 'wide'), 'real')
    g0 = float(np.float32(1.0) / np.float32(K.reference(c).mask.sum().item()))
    assert 0 < g0 < 0.02
    out = _run(c, g0=g0)
    _check_real(c, out, g0=g0)
    assert bool((out.grad_q != 0).any())


def test_wrapper_with_separate_and_shared_state_tensors():
    """QMIX._mix_td_fused with s and s_next as separate tensors (the (T, 0) layout of _state_rows, grad_p = empty_like) and as the
    two views of one tensor, at B * T = 33 * 7: both within the tolerances of tests/test_gpu_qmix_ops.py against its float64
    autograd."""
    from test_gpu_qmix_ops import GRAD_TOL, _case, _reference64, _rel
    from marl_dmfb_amd.policy.qmix import QMIX
    n, hh, B, T = 4, 24, 33, 7
    args, ev, tg, st, batch, q_e, q_t = _case(n, hh, B, T, seed=77)
    num64, gq64, g64 = _reference64(args, ev, tg, st, batch, q_e, q_t, T)
    pol = QMIX.__new__(QMIX)
    pol.args = types.SimpleNamespace(hyper_hidden_dim=hh, qmix_hidden_dim=32, gamma=0.99)
    pol.n_agents, pol.device = n, torch.device('cuda:0')
    pol.eval_qmix_net, pol.target_qmix_net = ev.to('cuda:0'), tg.to('cuda:0')
    stg = st.to('cuda:0')
    for mode in ('shared', 'separate'):
        b = {k: v.to('cuda:0') for k, v in batch.items()}
        if mode == 'shared':
            b['s'], b['s_next'] = stg[:, :-1], stg[:, 1:]
        else:
            b['s'], b['s_next'] = stg[:, :-1].contiguous(), stg[:, 1:].contiguous()
        b = {k: v[:, :T] for k, v in b.items()}
        (_, rows_e, off_e), (_, rows_t, off_t) = QMIX._state_rows(b['s'], b['s_next'], T)
        assert (rows_e, off_e, rows_t, off_t) == ((T + 1, 0, T + 1, 1) if mode == 'shared' else (T, 0, T, 0))
        for p in ev.parameters():
            p.grad = None
        pol._mix_bad = pol._td_bad = torch.zeros(1, dtype=torch.int32, device='cuda:0')
        qe = q_e.to('cuda:0').requires_grad_(True)
        num, mask_sum = pol._mix_td_fused(qe, q_t.to('cuda:0'), b, T)
        num.backward()
        assert abs(num.item() - num64.item()) <= 1e-5 * abs(num64.item())
        assert float(mask_sum) == float((~batch['padded'][:, :T]).sum())
        assert _rel(qe.grad.cpu(), gq64) < GRAD_TOL
        for k, p in ev.named_parameters():
            assert _rel(p.grad.cpu(), g64[k]) < GRAD_TOL, (mode, k, _rel(p.grad.cpu(), g64[k]))
        assert int(pol._mix_bad.item()) == 0
