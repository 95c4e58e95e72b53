"""What can be verified of tests/test_gpu_qmix_kernels.py without a GPU: every case it uses meets the conditions that make it
usable (tests/qmix_kernel_cases.py), the restated formulas of the float64 reference are QMixNet's and the TD rule of
policy/qmix.py, and a float32 evaluation of the same formulas on the CPU gives the yardstick from which the kernels' error
bounds are derived."""
import types

import pytest
import torch

import qmix_kernel_cases as K
from marl_dmfb_amd.network.qmix_net import QMixNet

REAL = [K.case(c, 'real') for c in K.COMBOS]


def test_the_combinations_cover_what_they_should():
    rows = {(B, T): B * T for B, T in K.ROW_COUNTS}
    assert sorted(rows.values()) == [1, 31, 32, 33, 259, 2049]
    for bt in K.ROW_COUNTS:                                  # every row count meets both H
        assert {c[3] for c in K.COMBOS if c[:2] == bt} == {24, 32}
    for shape in K.SHAPES:                                   # every (n, H, A) meets 33 and 259 rows
        assert {(3, 11), (37, 7)} <= {c[:2] for c in K.COMBOS if c[2:5] == shape}
    for H in (24, 32):                                       # every layout meets both H, on a ragged last workgroup
        assert {c[5] for c in K.COMBOS if c[3] == H and (c[0] * c[1]) % K.ROWS_PER_GROUP} == set(K.LAYOUTS)
    assert (16, 24, 16) in K.SHAPES and (1, 24, 1) in K.SHAPES


@pytest.mark.parametrize('combo', K.COMBOS, ids=K.COMBO_IDS)
def test_exact_cases_meet_the_exactness_conditions(combo):
    c = K.case(combo, 'exact')
    r = K.conditions(c)
    assert not bool(K.tie_rows(c).any())
    # multiples of 1/4 throughout: the float32 image of the reference is the reference
    for name in ('mtd', 'mask', 'grad_q', 'grad_p', 'Z', 'X'):
        t = getattr(r, name)
        assert torch.equal(4 * t, (4 * t).round()) and torch.equal(t.float().double(), t), name
    assert bool((r.mtd != 0).any()) and bool((r.grad_q != 0).any())


@pytest.mark.parametrize('combo', K.COMBOS, ids=K.COMBO_IDS)
def test_real_cases_meet_their_conditions(combo):
    c = K.case(combo, 'real')
    r = K.conditions(c)
    for name in ('mtd', 'grad_q', 'grad_p', 'Z', 'X'):
        assert bool(torch.isfinite(getattr(r, name)).all()), name
    # the absolute run bounds the real one element by element
    a = K.reference(c, absolute=True)
    for name in ('mtd', 'grad_q', 'grad_p', 'Z'):
        assert bool((getattr(r, name).abs() <= getattr(a, name).abs() * (1 + 1e-12)).all()), name


def _rel(a, b):
    return float((a.detach() - b.detach()).norm() / b.detach().norm())


@pytest.mark.parametrize('n,H,A,B,T,ring', [(3, 24, 5, 5, 7, False), (16, 32, 16, 3, 4, True), (1, 24, 1, 6, 2, True)])
def test_reference_is_qmixnet_and_the_td_rule(n, H, A, B, T, ring):
    """P = the first layers of a float64 QMixNet applied to the states: reference() must then give the mtd of QMixNet + the TD rule
    of policy/qmix.py:104-122 and, through Z^T X and dP^T s, every parameter gradient of the network."""
    S = 20
    args = types.SimpleNamespace(state_shape=S, hyper_hidden_dim=H, qmix_hidden_dim=K.M, n_agents=n, two_hyper_layers=True)
    torch.manual_seed(n * 100 + H)
    ev, tg = QMixNet(args).double(), QMixNet(args).double()
    with torch.no_grad():
        for p in list(ev.parameters()) + list(tg.parameters()):
            p.mul_(3.0)
    st = torch.randn((B, T + 1, S), dtype=torch.float64)
    c = K.make_case(B, T, n, H, A, 'ring' if ring else 'sep', 'real', seed=1)
    c.shared = False

    def first(net, rows):
        layers = net.first_layers()
        return torch.nn.functional.linear(rows, torch.cat([m.weight for m in layers]), torch.cat([m.bias for m in layers])).detach()
    s_e, s_t = (st, st) if ring else (st[:, :T], st[:, 1:])
    c.pe, c.pt = first(ev, s_e), first(tg, s_t)
    c.ev = [t.detach() for t in ev.second_layers()]
    c.tg = [t.detach() for t in tg.second_layers()]
    r = K.compute(c)

    qe = c.q_e.double().clone().requires_grad_(True)
    qg = torch.gather(qe.permute(1, 0, 2, 3), 3, c.u[:, :T].long()).squeeze(3)
    qm = c.q_t.double().permute(1, 0, 2, 3).masked_fill(c.avail[:, :T] == 0, -9999999).max(3)[0]
    tot_e, tot_t = ev(qg, st[:, :T]), tg(qm, st[:, 1:])
    targets = c.r[:, :T].double() + c.gamma * tot_t * (1 - c.term[:, :T].double())
    mask = 1 - c.padded[:, :T].double()
    mtd = mask * (tot_e - targets.detach())
    (mtd ** 2).sum().backward()
    assert _rel(r.mtd, mtd.reshape(-1)) <= 1e-12
    assert torch.equal(r.mask, mask.reshape(-1))
    assert _rel(r.grad_q, qe.grad) <= 1e-12
    want = [t.grad for t in ev.second_layers()]
    for k, (got, ref) in enumerate(zip(K.second_layer_grads(c, r), want)):
        assert _rel(got.reshape(ref.shape), ref) <= 1e-12, k
    dP = r.grad_p.reshape(-1, K.f_cols(H))
    dW, db = dP.t() @ s_e.reshape(-1, S), dP.sum(0)
    col = 0
    for m in ev.first_layers():
        rows = m.weight.shape[0]
        assert _rel(dW[col:col + rows], m.weight.grad) <= 1e-12 and _rel(db[col:col + rows], m.bias.grad) <= 1e-12
        col += rows
    assert col == K.f_cols(H)
    if ring:                                   # the extra state slot gets no gradient
        assert bool((r.grad_p[:, T] == 0).all())


def test_yardstick_ratios_are_the_recorded_ones():
    """The float32 evaluation of the same formulas on the CPU over the real cases: its worst ratios are the constants from which
    the kernels' bounds C_F and C_B are four times.  The sums are taken term by term in elementwise operations, so the figures do
    not depend on a BLAS; a tenth of slack either way is for the libm behind exp / expm1."""
    worst_f, worst_b = 0.0, 0.0
    for c in REAL:
        y = K.yardstick(c)
        worst_f = max(worst_f, K.forward_ratio(c, y.mtd))
        for name in ('grad_q', 'grad_p', 'Z'):
            worst_b = max(worst_b, K.backward_ratio(c, name, getattr(y, name)))
        r = K.reference(c)
        assert torch.equal(y.X.double(), r.X) and torch.equal(y.mask.double(), r.mask)
    print('yardstick: forward %.3e backward %.3e' % (worst_f, worst_b))
    assert 0.9 * K.YARD_F <= worst_f <= 1.1 * K.YARD_F, worst_f
    assert 0.9 * K.YARD_B <= worst_b <= 1.1 * K.YARD_B, worst_b
    assert K.C_F == 4 * K.YARD_F and K.C_B == 4 * K.YARD_B
    # the per-row bounds are far tighter than what the whole-tensor tolerance admits for a single row
    assert K.C_B < K.GRAD_TOL


def test_a_row_that_the_whole_tensor_bound_misses_fails_the_per_row_bound():
    """Dozens of rows of a case can have their whole grad_q row zeroed and stay under GRAD_TOL over the whole tensor; the per-row
    bound notices it in the row where that error is largest against the row's scale."""
    c = K.case((683, 3, 16, 32, 16, 'sep'), 'real')
    r, a = K.reference(c), K.reference(c, absolute=True)
    rows = K.row_view(c, 'grad_q', r.grad_q).norm(dim=1)
    scale = K.row_view(c, 'grad_q', a.grad_q).norm(dim=1)
    small = (rows > 0) & (rows < K.GRAD_TOL * r.grad_q.norm()) & ~K.tie_rows(c)
    assert int(small.sum()) >= 50
    k = int(torch.where(small, rows / scale.clamp_min(1e-300), torch.zeros_like(rows)).argmax())
    b, t = k // c.T, k % c.T
    broken = r.grad_q.clone()
    broken[t, b] = 0
    assert _rel(broken, r.grad_q) < K.GRAD_TOL
    assert K.backward_ratio(c, 'grad_q', broken) > 10 * K.C_B
