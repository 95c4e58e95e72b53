"""Shared by tests/test_qmix_kernel_cases.py (CPU) and tests/test_gpu_qmix_kernels.py (GPU): cases of the QMIX mixing + TD block
(include/qmix_ops.h) with every input of the two kernels spelled out, and their float64 reference ROW BY ROW.

`reference(case)` restates include/qmix_ops.h lines 8-13 in float64 torch autograd starting from P, the output of the
hypernetworks' first-layer GEMM (it does not go through QMixNet; tests/test_qmix_kernel_cases.py ties the two together):
  mtd, mask  [B*T], row b * T + t
  grad_q     [T][B][n][A]         d num / d q_eval, num = g0 * sum(mtd^2)
  grad_p     in the eval P's row layout [B][p_rows][F]  (zero in the rows of steps outside [0, T))
  X          [B*T][2H + M + 3]    [h1 | 1 | h2 | 1 | hb | 1]
  Z          [B*T][nM + M + 1]    [d num / d z1 | d num / d z2 | g], z1 / z2 the second-layer pre-activations (the arguments of
                                  |.|), g = d num / d q_tot_eval
`reference(case, absolute=True)` is the same computation with |.| of every input, no ReLU, no |.| and no ELU (every value is
>= 0 there, so |elu(pre)| = pre; the identity is used because autograd's subgradient of |.| at 0 is 0): differences become sums,
so each output of it bounds, row by row, the magnitude of every term that the real computation adds up for that output.  It is
the per-row SCALE of the error bounds of a real-valued case and the exactness bound of an integer case.

Two kinds of case (`make_case(..., kind=)`):
  'real'   randn inputs with a spread, so that both branches of relu, |.| and elu occur; the target of one unterminated,
           unpadded row has an agent without any available action (the -9999999 maximum).  float32 and float64 may pick
           different signs for a second-layer pre-activation z that is nearly 0: an entry is a NEAR TIE if |z| in float64 is below
           delta = 2 (H + 1) 2^-24 (sum |w| |h| + |b|), twice the worst-case float32 dot-product bound.  A row holding one is left
           out of the gradient comparisons (not of mtd's: |z| is continuous).  At most MAX_TIE_ROWS of a case's rows may be.
  'exact'  small integers throughout, q >= 0 and the b1 columns of P >= 0, so that pre >= 0 everywhere, elu(pre) = pre, and every
           product and partial sum is an integer (a multiple of 1/4 in the backward: gamma = 0.5, g0 = 0.25) far below 2^24 / 4 in
           any order, with or without FMA.  The float32 kernels must equal float64 bit for bit, ties included: several percent of
           the relu inputs, of z1, z2 and of pre are exactly 0.
`conditions(case)` asserts what makes a case usable, from the reference alone.
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

M = 32                                   # qmix_hidden_dim of the build
ROWS_PER_GROUP = 32                      # csrc/qmix_ops.hip: kBlock / kLanes rows per 256-thread workgroup
GAMMA = float(np.float32(0.99))          # the kernels take gamma as a float: the reference uses the same number
U24 = 2.0 ** -24
BOUND_LIMIT = 2.0 ** 22
MAX_TIE_ROWS = 0.05
MIN_ZEROS, MIN_POSITIVE, MIN_EACH_SIGN = 0.01, 0.25, 0.10
GRAD_TOL = 5e-6                          # the project's whole-tensor relative L2 (tests/test_gpu_qmix_ops.py)

# (B, T): 1, 31, 32, 33, 259 and 2049 rows -- one row, one short of a workgroup, exactly one, one over, nine with a ragged last
# one, many.
ROW_COUNTS = [(1, 1), (31, 1), (4, 8), (3, 11), (37, 7), (683, 3)]
# (n, H, A)
SHAPES = [(1, 24, 1), (2, 24, 5), (4, 32, 9), (10, 32, 5), (16, 24, 16), (16, 32, 16)]
# P layouts (include/qmix_ops.h): name -> (eval rows per episode - T, eval offset, target rows - T, target offset, one buffer)
LAYOUTS = {'sep': (0, 0, 0, 0, False),     # s and s_next as separate tensors
           'ring': (1, 0, 1, 1, True),     # the replay ring: both networks read one buffer of T + 1 slots per episode
           'wide': (3, 2, 2, 1, False)}    # more slots than steps on either side of the eval rows
# every row count meets both H, every (n, H, A) meets 33 and 259 rows; the layouts rotate
_MEET = {(1, 1): [0, 2], (31, 1): [1, 3], (4, 8): [4, 5], (3, 11): [0, 1, 2, 3, 4, 5], (37, 7): [0, 1, 2, 3, 4, 5], (683, 3): [1, 5]}
COMBOS = []
for _bt in ROW_COUNTS:
    for _k in _MEET[_bt]:
        COMBOS.append(_bt + SHAPES[_k] + (sorted(LAYOUTS)[len(COMBOS) % 3],))
COMBO_IDS = ['B%d_T%d_n%d_H%d_A%d_%s' % c for c in COMBOS]

# exact cases, (n, H) -> (density of the second-layer weights, share of zero q, share of zero b1 columns of P)
RECIPE = {(1, 24): (0.10, 0.5, 0.5), (2, 24): (0.10, 0.5, 0.5), (4, 32): (0.08, 0.5, 0.5), (10, 32): (0.06, 0.7, 0.5),
          (16, 24): (0.06, 0.8, 0.6), (16, 32): (0.05, 0.8, 0.6)}
# real cases: randn times these (P, the second-layer weights, q)
SPREAD_P, SPREAD_W, SPREAD_Q = 1.5, 0.5, 2.0
# seeds chosen on the CPU so that conditions() holds where seed 0 misses it (a single row leaves little to chance)
SEEDS = {((1, 1, 1, 24, 1, 'ring'), 'real'): 6,     # seed 0 terminates the only row
         ((1, 1, 4, 32, 9, 'sep'), 'exact'): 2}    # seed 0 has no pre == 0 among the row's 32

# ---- accuracy of the real-valued cases (profiles/qmix/NOTES.md, "Accuracy of the mixer kernels") -------------------------------
# YARD_*: the worst ratio, over the real cases of COMBOS, of a float32 evaluation of the SAME formulas on the CPU (`yardstick`)
# against the float64 reference: YARD_F = max |mtd32 - mtd64| / scale_row, YARD_B = max over grad_q / grad_p / Z and rows of
# ||row32 - row64|| / ||row of the absolute run||, near-tie rows excepted.  tests/test_qmix_kernel_cases.py recomputes them.
# The kernels' bounds are 4 x the yardstick: the margin is for another summation order, FMA contraction and the device's
# expm1f / expf.  Neither was read off the kernels; KERNEL_* is what the kernels gave on an MI355X, for the record only.
YARD_F = 9.18e-9
YARD_B = 2.58e-9
C_F, C_B = 4 * YARD_F, 4 * YARD_B
KERNEL_F = 8.51e-9       # B683_T3_n2_H24_A5_ring
KERNEL_B = 2.83e-9       # Z of the same case; grad_q 6.4e-10, grad_p 5.7e-10


def f_cols(H):
    return 2 * H + 2 * M


def x_cols(H):
    return 2 * H + M + 3


def z_cols(n):
    return n * M + M + 1


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g)


def _episode(g, B, T, Tl):
    """terminated / padded as tests/test_gpu_qmix_ops.py:_case draws them, uint8 [B][Tl][1]."""
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    t = torch.arange(Tl)[None, :]
    padded = (t >= lens[:, None]).unsqueeze(-1)
    term = (t >= lens[:, None] - 1).unsqueeze(-1) & (torch.rand((B, 1, 1), generator=g) < 0.7)
    term = term | padded
    return term.to(torch.uint8), padded.to(torch.uint8)


def make_case(B, T, n, H, A, layout, kind, seed=0):
    """All inputs of qmix_mix_td_forward / _backward as CPU tensors in the layouts of include/qmix_ops.h."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * B + 31 * T + 7 * n + H + 3 * A + (kind == 'exact'))
    Tl, Fc, R = T + 3, f_cols(H), B * T
    de, oe, dt, ot, shared = LAYOUTS[layout]
    c = types.SimpleNamespace(B=B, T=T, n=n, H=H, A=A, Tl=Tl, R=R, layout=layout, kind=kind, seed=seed, shared=shared,
                              pe_rows=T + de, pe_off=oe, pt_rows=T + dt, pt_off=ot)
    c.key = (B, T, n, H, A, layout, kind, seed)
    c.term, c.padded = _episode(g, B, T, Tl)
    if kind == 'real':
        c.gamma, c.g0 = GAMMA, 1.0

        def mixer():
            return (torch.randn((n * M, H), generator=g) * SPREAD_W, torch.randn((n * M,), generator=g), torch.randn((M, H), generator=g) * SPREAD_W,
                    torch.randn((M,), generator=g), torch.randn((1, M), generator=g), torch.randn((1,), generator=g))

        def first(rows):
            return torch.randn((B, rows, Fc), generator=g) * SPREAD_P
        c.q_e = torch.randn((T, B, n, A), generator=g) * SPREAD_Q
        c.q_t = torch.randn((T, B, n, A), generator=g) * SPREAD_Q
        c.u = torch.randint(0, A, (B, Tl, n, 1), generator=g, dtype=torch.int8)
        c.r = torch.randn((B, Tl, 1), generator=g)
        c.avail = (torch.rand((B, Tl, n, A), generator=g) < 0.8).to(torch.int8)
        live = ((c.term[:, :T, 0] == 0) & (c.padded[:, :T, 0] == 0)).nonzero()
        if len(live):                        # one agent without any available action in a row whose target counts
            c.avail[live[0, 0], live[0, 1], n - 1] = 0
    else:
        density, q_zero, b_zero = RECIPE[(n, H)]
        c.gamma, c.g0 = 0.5, 0.25

        def sparse(shape):
            return (_ints(g, shape, -1, 1) * (torch.rand(shape, generator=g) < density)).float()

        def mixer():
            return (sparse((n * M, H)), _ints(g, (n * M,), -1, 1).float(), sparse((M, H)), _ints(g, (M,), -1, 1).float(),
                    _ints(g, (1, M), -1, 1).float(), _ints(g, (1,), -1, 1).float())

        def first(rows):
            p = _ints(g, (B, rows, Fc), -2, 2).float()
            b1 = _ints(g, (B, rows, M), 1, 2).float() * (torch.rand((B, rows, M), generator=g) >= b_zero)
            p[:, :, 2 * H:2 * H + M] = b1
            return p

        def q():
            return (_ints(g, (T, B, n, A), 1, 2) * (torch.rand((T, B, n, A), generator=g) >= q_zero)).float()
        c.q_e, c.q_t = q(), q()
        c.u = torch.randint(0, A, (B, Tl, n, 1), generator=g, dtype=torch.int8)
        c.r = _ints(g, (B, Tl, 1), -2, 2).float()
        c.avail = (torch.rand((B, Tl, n, A), generator=g) < 0.8).to(torch.int8)
        c.avail.scatter_(3, torch.randint(0, A, (B, Tl, n, 1), generator=g), 1)     # every agent has an available action
    c.ev, c.tg = mixer(), mixer()
    c.pe = first(c.pe_rows)
    c.pt = c.pe if shared else first(c.pt_rows)
    return c


def case(combo, kind):
    """The case of one entry of COMBOS."""
    return make_case(*combo, kind, seed=SEEDS.get((combo, kind), 0))


def _dot(h, w, b, seq):
    """h [R][K] @ w[N][K]^T + b -> [R][N]; seq=True adds the K terms one after the other in elementwise operations, so that the
    float32 yardstick does not depend on the BLAS at hand."""
    if not seq:
        return h @ w.t() + b
    acc = torch.zeros((h.shape[0], w.shape[0]), dtype=h.dtype)
    for k in range(h.shape[1]):
        acc = acc + h[:, k:k + 1] * w[:, k]
    return acc + b


def _sum(terms, seq):
    """Sum over the last axis, one term after the other when seq."""
    if not seq:
        return terms.sum(-1)
    acc = terms[..., 0]
    for k in range(1, terms.shape[-1]):
        acc = acc + terms[..., k]
    return acc


def _mix(P, w, q, n, H, absolute, seq):
    """q_tot [R] of rows P [R][F] and agent values q [R][n] (include/qmix_ops.h lines 8-10) and the intermediates."""
    act = (lambda t: t) if absolute else torch.relu
    mag = (lambda t: t) if absolute else torch.abs
    w1, b1, w2, b2, wb, bb = w
    m = types.SimpleNamespace()
    m.h1, m.h2, m.hb = act(P[:, :H]), act(P[:, H:2 * H]), act(P[:, 2 * H + M:])
    m.z1 = _dot(m.h1, w1, b1, seq)                          # [R][n * M], entry i * M + j
    m.z2 = _dot(m.h2, w2, b2, seq)                          # [R][M]
    b2v = _dot(m.hb, wb, bb, seq)[:, 0]
    terms = q.unsqueeze(1) * mag(m.z1).view(-1, n, M).transpose(1, 2)      # [R][M][n]
    m.pre = _sum(terms, seq) + P[:, 2 * H:2 * H + M]
    m.hid = m.pre if absolute else F.elu(m.pre)
    m.prod = m.hid * mag(m.z2)
    m.tot = _sum(m.prod, seq) + b2v
    return m


def compute(c, absolute=False, dtype=torch.float64, seq=False, g0=None):
    """The block on case `c` (uncached).  The case's tensors may already be float64 (tests/test_qmix_kernel_cases.py)."""
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    B, T, n, H, A, R = c.B, c.T, c.n, c.H, c.A, c.R
    g0 = c.g0 if g0 is None else g0
    P = f(c.pe.to(dtype)).clone().requires_grad_(True)
    Pt = (P.detach() if c.shared else f(c.pt.to(dtype)))[:, c.pt_off:c.pt_off + T].reshape(R, -1)
    Pe = P[:, c.pe_off:c.pe_off + T].reshape(R, -1)
    ev = [f(t.to(dtype)) for t in c.ev]
    tg = [f(t.to(dtype)) for t in c.tg]
    qe = c.q_e.to(dtype).clone().requires_grad_(True)
    qev = f(qe).permute(1, 0, 2, 3)                                           # [B][T][n][A]
    qtv = c.q_t.to(dtype).permute(1, 0, 2, 3)
    taken = torch.gather(qev, 3, c.u[:, :T].long()).squeeze(3).reshape(R, n)
    tmax = f(qtv.masked_fill(c.avail[:, :T] == 0, -9999999.0).max(3)[0]).reshape(R, n)
    e = _mix(Pe, ev, taken, n, H, absolute, seq)
    t = _mix(Pt, tg, tmax.detach(), n, H, absolute, seq)
    for v in (e.z1, e.z2, e.tot, e.h1, e.h2):
        v.retain_grad()
    r = f(c.r[:, :T].to(dtype)).reshape(R)
    not_term = 1.0 - c.term[:, :T].to(dtype).reshape(R)
    mask = 1.0 - c.padded[:, :T].to(dtype).reshape(R)
    target = r + (c.gamma * t.tot.detach()) * not_term
    mtd = mask * (e.tot + target if absolute else e.tot - target)
    num = abs(g0) * (mtd * mtd).sum() if absolute else g0 * (mtd * mtd).sum()
    num.backward()
    out = types.SimpleNamespace(mtd=mtd.detach(), mask=mask, num=num.detach(), grad_q=qe.grad, grad_p=P.grad)
    one = torch.ones((R, 1), dtype=dtype)
    out.X = torch.cat([e.h1.detach(), one, e.h2.detach(), one, e.hb.detach(), one], dim=1)
    out.Z = torch.cat([e.z1.grad, e.z2.grad, e.tot.grad.unsqueeze(1)], dim=1)
    out.z1, out.z2, out.pre, out.pre_t = e.z1.detach(), e.z2.detach(), e.pre.detach(), t.pre.detach()
    out.dh1, out.dh2 = e.h1.grad, e.h2.grad
    out.tot_e, out.tot_t = e.tot.detach(), t.tot.detach()
    out.prod, out.prod_t = e.prod.detach(), t.prod.detach()
    return out


@functools.lru_cache(maxsize=None)
def _reference(key, absolute, g0):
    return compute(make_case(*key), absolute=absolute, g0=g0)


def reference(c, absolute=False, g0=None):
    """The float64 reference of case `c`, or its absolute run (cached; treat as read-only).  g0 replaces the case's own."""
    return _reference(c.key, absolute, g0)


def yardstick(c, g0=None):
    """float32 torch autograd of the same formulas from the same P on the CPU, the sums taken term by term."""
    return compute(c, dtype=torch.float32, seq=True, g0=g0)


def tie_rows(c):
    """bool [B*T]: rows holding a near-tie second-layer pre-activation (module docstring).  Always empty for an exact case."""
    if c.kind == 'exact':
        return torch.zeros(c.R, dtype=torch.bool)
    r, H = reference(c), c.H
    w1, b1, w2, b2 = (t.double().abs() for t in c.ev[:4])
    k = 2 * (H + 1) * U24
    d1 = k * (r.X[:, :H] @ w1.t() + b1)
    d2 = k * (r.X[:, H + 1:2 * H + 1] @ w2.t() + b2)
    return (r.z1.abs() < d1).any(1) | (r.z2.abs() < d2).any(1)


def row_view(c, name, t):
    """An output tensor as [B*T][row's elements] (grad_q: [T][B][n][A]; grad_p: the rows of steps t < T)."""
    if name == 'grad_q':
        return t.reshape(c.T, c.B, -1).permute(1, 0, 2).reshape(c.R, -1)
    if name == 'grad_p':
        return t.reshape(c.B, c.pe_rows, -1)[:, c.pe_off:c.pe_off + c.T].reshape(c.R, -1)
    return t.reshape(c.R, -1)


def forward_ratio(c, mtd, g0=None):
    """max over rows of |mtd - mtd64| / scale_row (0 / 0 counts as 0: a padded row's mtd is exactly 0)."""
    r, a = reference(c, g0=g0), reference(c, absolute=True, g0=g0)
    err = (mtd.double() - r.mtd).abs()
    assert bool((err[a.mtd == 0] == 0).all()), 'a row of scale 0 is not exactly 0'
    return float((err / a.mtd.clamp_min(1e-300)).max())


def backward_ratio(c, name, t, g0=None):
    """max over the rows that are no near tie of ||row - row64|| / ||row of the absolute run||."""
    r, a = reference(c, g0=g0), reference(c, absolute=True, g0=g0)
    keep = ~tie_rows(c)
    err = (row_view(c, name, t.double()) - row_view(c, name, getattr(r, name))).norm(dim=1)[keep]
    scale = row_view(c, name, getattr(a, name)).norm(dim=1)[keep]
    assert bool((err[scale == 0] == 0).all()), (name, 'a row of scale 0 is not exactly 0')
    return float((err / scale.clamp_min(1e-300)).max()) if err.numel() else 0.0


def second_layer_grads(c, r):
    """The six second-layer gradients as policy/qmix.py forms them from Z and X."""
    H, nM = c.H, c.n * M
    g1 = r.Z[:, :nM].t() @ r.X[:, :H + 1]
    g2 = r.Z[:, nM:nM + M].t() @ r.X[:, H + 1:2 * H + 2]
    g3 = r.Z[:, nM + M:].t() @ r.X[:, 2 * H + 2:]
    return [g1[:, :H], g1[:, H], g2[:, :H], g2[:, H], g3[:, :M], g3[:, M]]


def conditions(c):
    """Asserts what the module docstring requires of a case -> its reference."""
    r, a = reference(c), reference(c, absolute=True)
    tag = c.key
    T = c.T
    for k, g in enumerate(second_layer_grads(c, r)):
        assert bool((g != 0).any()), (tag, 'second-layer gradient %d is zero' % k)
    if c.kind == 'real':
        assert float((r.pre < 0).double().mean()) >= MIN_EACH_SIGN and float((r.pre > 0).double().mean()) >= MIN_EACH_SIGN, tag
        starved = (c.avail[:, :T] == 0).all(3).any(2) & (c.term[:, :T, 0] == 0) & (c.padded[:, :T, 0] == 0)
        assert bool(starved.any()), (tag, 'no starved agent in a row whose target counts')
        if c.B >= 2 and T >= 2:          # an episode has at least one step, so a single step is never padded
            for name in ('term', 'padded'):
                v = getattr(c, name)[:, :T]
                assert bool((v == 0).any()) and bool((v != 0).any()), (tag, name)
        assert float(tie_rows(c).double().mean()) <= MAX_TIE_ROWS, (tag, float(tie_rows(c).double().mean()))
        return r
    big = [a.z1, a.z2, a.pre, a.pre_t, a.prod, a.prod_t, a.tot_e, a.tot_t, a.mtd, a.Z, a.grad_p, a.grad_q, a.dh1, a.dh2]
    bound = max(float(t.abs().max()) for t in big)
    assert bound < BOUND_LIMIT, (tag, bound)
    relu_in = torch.cat([c.pe[:, :, :2 * c.H], c.pe[:, :, 2 * c.H + M:]], dim=2)
    for name, t in (('pre', r.pre), ('z1', r.z1), ('z2', r.z2), ('relu inputs', relu_in)):
        assert float((t == 0).double().mean()) >= MIN_ZEROS, (tag, name, float((t == 0).double().mean()))
    assert float((r.pre > 0).double().mean()) >= MIN_POSITIVE, tag
    assert bool((r.pre >= 0).all()) and bool((r.pre_t >= 0).all()), tag
    return r
