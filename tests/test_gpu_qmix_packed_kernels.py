"""The packed QMIX kernels through their C ABI (include/qmix_packed.h; csrc/qmix_ops.hip: k_mix_forward / k_mix_backward with the
PackedIndex rule, k_gather_states).

Mixer: the cases of tests/qmix_kernel_cases.py, their valid (episode, step) units laid out as the packed learn lays them out
(length-sorted, step-major), the Q rows, the eval P rows and the target P rows picked for those units on the host.
  (a) every output row of a unit has the BITS of the row that the padded entry points (include/qmix_ops.h) give for its (b, t):
      both run the same per-row code;
  (b) exact cases equal the float64 reference value for value, real cases stay within C_F / C_B with the near-tie rule of
      qmix_kernel_cases (the rows that the packed run leaves out, the padded steps, are taken from the reference);
  (c) one bad action poisons its unit only;  (d) two launches give identical bits;
  (e) the rows of grad_q behind the units' (up to the row count rounded up to 64) are zeros.
Gather: float32 rows equal to states[rows].float() exactly for state lengths around the 16-byte paths, row lists with repeats in no
order, a source one byte past a 16-byte boundary, the full int8 range; an id outside the tensor gives a NaN row and leaves its
neighbours intact.  Every buffer sits between guard regions (front_kernel_cases.guarded)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import qmix_kernel_cases as K
import test_gpu_qmix_kernels as P
from front_kernel_cases import guarded

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENT = P.SENT
# (B, T) x two of K.SHAPES each: both H, n = 1 and n = 16 occur; the P layouts rotate
_PICK = {(1, 1): (0, 5), (31, 1): (1, 3), (4, 8): (4, 2), (3, 11): (0, 5), (37, 7): (3, 4), (683, 3): (1, 5)}
COMBOS = []
for _bt in K.ROW_COUNTS:
    for _k in _PICK[_bt]:
        COMBOS.append(_bt + K.SHAPES[_k] + (sorted(K.LAYOUTS)[len(COMBOS) % 3],))
IDS = ['B%d_T%d_n%d_H%d_A%d_%s' % c for c in COMBOS]
ROW_OUTPUTS = ('mtd', 'mask', 'grad_q', 'grad_p', 'Z', 'X')


def _case(combo, kind):
    return K.make_case(*combo, kind, seed=K.SEEDS.get((combo, kind), 0))


def _units(c, all_rows=False):
    """(b, t) of the units in packed order: episodes sorted by length (stable), step after step the episodes longer than it."""
    lens = (c.padded[:, :c.T, 0] == 0).sum(1).numpy()
    if all_rows:
        lens = np.full(c.B, c.T)
    order = np.argsort(-lens, kind='stable')
    return [(int(b), t) for t in range(c.T) for b in order if lens[b] > t]


def _pack(c, d, bt, target='rows'):
    """The packed inputs of case `c` for the units `bt` on the GPU.  target: 'rows' = the case's whole target P buffer and a
    row list, 'gathered' = the units' target rows gathered and d_p_target_row NULL."""
    def put(t):
        v, chk = P._put(t)
        d.checks.append(chk)
        return v
    b, t = torch.tensor([x[0] for x in bt]), torch.tensor([x[1] for x in bt])
    k = types.SimpleNamespace(U=len(bt), b=b, t=t, row=b * c.T + t)
    k.rows_pad = -(-k.U * c.n // 64) * 64

    def q(src):
        full = torch.full((k.rows_pad, c.A), float('nan'))
        full[:k.U * c.n] = src[t, b].reshape(k.U * c.n, c.A)
        return put(full)
    k.q_e, k.q_t = q(c.q_e), q(c.q_t)
    k.units = put((b * c.Tl + t).to(torch.int32))
    k.pe = put(c.pe[b, t + c.pe_off])
    if target == 'gathered':
        k.pt, k.trow = put(c.pt[b, t + c.pt_off]), None
    else:
        k.pt, k.trow = d.pt, put((b * c.pt_rows + t + c.pt_off).to(torch.int32))
    return k


def _run_packed(c, d, k, g0=None, counter=True):
    """Forward, then the backward on the forward's own mtd / mask, as _MixTDPacked does -> CPU outputs, one row per unit."""
    lib = P._lib().qmix_packed()
    p = P._p
    mtd, mask = P._out(d, (k.U,)), P._out(d, (k.U,))
    cnt = P._out(d, (1,), 0, torch.int32)
    rc = lib.qmix_mix_td_forward_packed(p(k.q_e), p(k.q_t), p(k.units), k.U, p(d.u), p(d.r), p(d.avail), p(d.term), p(d.padded), c.n, c.A,
                                        p(k.pe), p(k.pt), p(k.trow), c.H, K.M, C.byref(d.mix_e), C.byref(d.mix_t), c.gamma, p(mtd),
                                        p(mask), p(cnt) if counter else None, None)
    assert rc == 0
    gq = P._out(d, (k.rows_pad, c.A))
    gp = P._out(d, (k.U, K.f_cols(c.H)))
    Z = P._out(d, (k.U, K.z_cols(c.n)))
    X = P._out(d, (k.U, K.x_cols(c.H)))
    gnum = P._out(d, (1,), c.g0 if g0 is None else g0)
    rc = lib.qmix_mix_td_backward_packed(p(mtd), p(mask), p(k.q_e), p(k.units), k.U, p(d.u), c.n, c.A, k.rows_pad, p(k.pe), c.H, K.M,
                                         C.byref(d.mix_e), p(gnum), p(gq), p(gp), p(Z), p(X), None)
    assert rc == 0
    torch.cuda.synchronize()
    for chk in d.checks:
        chk()
    out = types.SimpleNamespace(bad=int(cnt[0]), mtd=mtd.cpu(), mask=mask.cpu(), grad_p=gp.cpu(), Z=Z.cpu(), X=X.cpu())
    gq = gq.cpu()
    for name in ('mtd', 'mask', 'grad_p', 'Z', 'X'):
        assert not bool((getattr(out, name) == SENT).any()), (name, 'an output element was left unwritten')
    assert not bool((gq == SENT).any()), 'an element of grad_q was left unwritten'
    out.grad_q = gq[:k.U * c.n].reshape(k.U, c.n * c.A)
    out.tail = gq[k.U * c.n:]
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_rows(c, k, out, padded):
    """(a): unit j of the packed outputs has the bits of row (b, t) of the padded entry points' outputs."""
    for name in ROW_OUTPUTS:
        want = K.row_view(c, name, getattr(padded, name))[k.row]
        got = getattr(out, name).reshape(k.U, -1)
        same = _bits(got) == _bits(want)
        assert bool(same.all()), (name, 'unit %d differs from its padded row' % int((~same).any(1).nonzero()[0]))


def _full(c, k, out):
    """The packed outputs in the padded entry points' layouts; the rows the packed run leaves out come from the reference."""
    r = K.reference(c)
    full = types.SimpleNamespace(bad=out.bad)
    for name in ROW_OUTPUTS:
        rows = K.row_view(c, name, getattr(r, name)).float().clone().reshape(c.R, -1)
        rows[k.row] = getattr(out, name).reshape(k.U, -1)
        if name == 'grad_q':
            rows = rows.reshape(c.B, c.T, c.n, c.A).permute(1, 0, 2, 3).contiguous()
        elif name == 'grad_p':
            gp = torch.zeros((c.B, c.pe_rows, K.f_cols(c.H)))
            gp[:, c.pe_off:c.pe_off + c.T] = rows.reshape(c.B, c.T, -1)
            rows = gp
        else:
            rows = rows.reshape(getattr(r, name).shape)
        setattr(full, name, rows)
    return full


@pytest.mark.parametrize('kind', ['exact', 'real'])
@pytest.mark.parametrize('combo', COMBOS, ids=IDS)
def test_units_have_the_bits_of_the_padded_rows(combo, kind):
    c = _case(combo, kind)
    d = P._to_gpu(c)
    padded = P._run(c, d)
    k = _pack(c, d, _units(c))
    assert k.U == int((c.padded[:, :c.T] == 0).sum()) and bool((padded.mask[k.row] == 1).all())
    out = _run_packed(c, d, k)
    assert out.bad == 0
    _same_rows(c, k, out, padded)                                          # (a)
    assert k.rows_pad % 64 == 0 and not bool((out.tail != 0).any())        # (e)
    assert _bits(out.tail).count_nonzero() == 0, 'a padding row of grad_q holds -0.0'
    full = _full(c, k, out)
    if kind == 'exact':                                                    # (b)
        r = K.reference(c)
        for name in ROW_OUTPUTS:
            diff = getattr(full, name).double() != getattr(r, name)
            assert not bool(diff.any()), (name, int(diff.sum()))
    else:
        P._check_real(c, full)
    again = _run_packed(c, d, k)                                           # (d)
    for name in ROW_OUTPUTS + ('tail',):
        assert torch.equal(_bits(getattr(again, name)), _bits(getattr(out, name))), name


@pytest.mark.parametrize('combo', [COMBOS[8], COMBOS[5]], ids=[IDS[8], IDS[5]])
def test_every_row_as_a_unit_and_gathered_target_rows(combo):
    """All B * T rows as units, the padded steps included, and the target rows gathered on the host with d_p_target_row NULL."""
    c = _case(combo, 'real')
    d = P._to_gpu(c)
    padded = P._run(c, d)
    bt = _units(c, all_rows=True)
    assert len(bt) == c.R
    k = _pack(c, d, bt, target='gathered')
    out = _run_packed(c, d, k)
    _same_rows(c, k, out, padded)
    assert bool((out.mask == 0).any()) and not bool((out.tail != 0).any())
    # the valid units alone, gathered target rows: the same bits again
    k2 = _pack(c, d, _units(c), target='gathered')
    _same_rows(c, k2, _run_packed(c, d, k2), padded)


def test_one_bad_action_poisons_its_unit_only():
    c = _case(COMBOS[8], 'real')
    assert (c.B, c.T) == (37, 7)
    bt = _units(c)
    d = P._to_gpu(c)
    k = _pack(c, d, bt)
    base = _run_packed(c, d, k)
    hit_j = len(bt) - 2                                       # a unit of the last, ragged workgroup
    b, t = bt[hit_j]
    c.u[b, t, c.n - 1, 0] = c.A
    d = P._to_gpu(c)
    k = _pack(c, d, bt)
    out = _run_packed(c, d, k)
    assert out.bad == 1
    hit = torch.zeros(k.U, dtype=torch.bool)
    hit[hit_j] = True
    assert bool(torch.isnan(out.mtd[hit]).all()) and not bool(torch.isnan(out.mtd[~hit]).any())
    assert bool(torch.isnan(out.grad_q[hit]).all()), 'a grad_q entry of the bad unit is not NaN'
    for name in ROW_OUTPUTS:
        a, w = getattr(out, name).reshape(k.U, -1)[~hit], getattr(base, name).reshape(k.U, -1)[~hit]
        assert torch.equal(_bits(a), _bits(w)), name
    assert not bool((out.tail != 0).any())
    again = _run_packed(c, d, k, counter=False)               # without a counter: accepted, same mtd
    assert again.bad == 0 and torch.equal(_bits(again.mtd), _bits(out.mtd))


# ------------------------------------------------------------------------------------------------------------------ the gather
def _gather(states, rows, n_state_rows=None):
    """qmix_gather_states of `rows` (int32, GPU) from `states` (int8 (n, S), GPU) into a guarded, sentinel-filled output."""
    n, S = states.shape
    out, check = guarded((rows.numel(), S), torch.float32, SENT, DEV)
    rc = P._lib().qmix_packed().qmix_gather_states(P._p(states), n if n_state_rows is None else n_state_rows, S, P._p(rows), rows.numel(),
                                                   P._p(out), None)
    assert rc == 0
    torch.cuda.synchronize()
    check()
    return out


def _states(n, S, offset, gen):
    """int8 (n, S) holding every value of the int8 range, its first byte `offset` bytes past a 256-byte boundary."""
    flat = torch.randint(-128, 128, (n * S + 512,), dtype=torch.int8, device=DEV, generator=gen)
    start = (-flat.data_ptr()) % 256 + offset
    st = flat[start:start + n * S].view(n, S)
    assert st.data_ptr() % 16 == offset
    if n * S >= 256:
        st.view(-1)[:256] = torch.arange(-128, 128, device=DEV).to(torch.int8)
    return st


@pytest.mark.parametrize('n_rows', [1, 63, 65, 1000])
@pytest.mark.parametrize('S', [1, 15, 16, 17, 300, 1800])
def test_gather_equals_indexing(S, n_rows):
    gen = torch.Generator(device=DEV).manual_seed(S * 1009 + n_rows)
    n = 257
    for offset in (0, 1):
        st = _states(n, S, offset, gen)
        rows = torch.randint(0, n, (n_rows,), device=DEV, generator=gen).to(torch.int32)     # repeats, no order
        if n_rows >= 63:
            rows[:4] = torch.tensor([n - 1, 0, n - 1, 5], dtype=torch.int32, device=DEV)
        out = _gather(st, rows)
        assert torch.equal(out, st[rows.long()].float()), (S, n_rows, offset)
        if S * n >= 256:
            first = _gather(st, torch.arange(0, -(-256 // S), device=DEV, dtype=torch.int32)).reshape(-1)[:256]
            assert torch.equal(first, torch.arange(-128, 128, device=DEV).float())             # the full int8 range


@pytest.mark.parametrize('S', [17, 300, 1800])
def test_gather_gives_nan_rows_for_ids_outside_the_tensor(S):
    gen = torch.Generator(device=DEV).manual_seed(S)
    n = 40
    st = _states(n + 2, S, 1, gen)[1:n + 1]                   # real bytes on either side of the tensor the call is told about
    rows = torch.randint(0, n, (70,), device=DEV, generator=gen).to(torch.int32)
    bad = {3: -1, 20: n, 21: 2 ** 31 - 1, 64: -2 ** 31, 69: n + 1}
    for i, v in bad.items():
        rows[i] = v
    out = _gather(st, rows)
    is_bad = torch.zeros(70, dtype=torch.bool, device=DEV)
    is_bad[list(bad)] = True
    assert bool(torch.isnan(out[is_bad]).all())
    assert torch.equal(out[~is_bad], st[rows[~is_bad].long()].float())
