"""The kernels of the packed learn (`VDN.learn_packed`) one by one, through the C ABI, against float64 restatements on the CPU:
vdn_td_forward_packed / vdn_td_backward_packed (and the unpacked pair on the same memory), vdn_gather_units, vdn_clip_adam_step with
and without d_grad_div, and the edges of the packed GRU sequence kernels that the tests of tests/test_gpu_crnn_ops.py leave out.

Inputs are built so that every factor matters (padded and terminated steps anywhere, unsorted unit lists with repeats, agents without
an available action, non-zero initial states, rows that never run), and no bound was read off the kernels: each is derived from the
operation count and the float32 unit roundoff 2^-24 (the TD block), exact (gather, gradient scatter, masks), or the tolerance the
project already uses for that kernel (GRU: 2e-5 on h, relative L2 2e-4 on gradients; clip + Adam: those of
tests/test_gpu_td_fused.py).  Every output buffer is pre-filled with a sentinel and is followed by a guard region in the same
allocation: every element must be written and nothing beyond."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = -777.25      # no kernel output below can take this value
GUARD = 256         # elements after every output buffer that must keep their fill
U24 = 2.0 ** -24    # unit roundoff of float32
BAD_ARG, UNSUPPORTED = -1, -6


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _out(n, fill=SENT, dtype=torch.float32):
    """A flat output buffer of n elements filled with `fill`, with GUARD more elements behind it in the same allocation."""
    return torch.full((n + GUARD,), fill, dtype=dtype, device='cuda')


def _written_inside(buf, n, fill=SENT):
    """Every one of the first n elements was written, none of the elements behind them."""
    assert not bool((buf[:n] == fill).any()), 'an output element was left unwritten'
    assert bool((buf[n:] == fill).all()), 'written past the end of the output'


def _untouched(buf, fill=SENT):
    assert bool((buf == fill).all())


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the TD block
# ------------------------------------------------------------------------------------------------------------------------------
S, TL = 11, 7                            # ring slots, steps per slot
GAMMA = float(np.float32(0.99))          # the kernels take gamma as a float: the reference uses the same number
G_NUM = 0.37                             # upstream gradient *d_grad_num


def _td_inputs(n, A, U, seed, starve=False):
    """Replay tensors of an S x TL ring (flat over slot * TL + t), an unsorted random unit list and the Q tensors of U units with
    NaN rows up to the next multiple of 64 rows.  CPU tensors; starve=True leaves about a quarter of the agents without any
    available action, otherwise every agent has at least one."""
    g = torch.Generator().manual_seed(seed)
    N = S * TL
    d = types.SimpleNamespace(n=n, A=A, U=U)
    d.units = torch.randint(0, N, (U,), generator=g, dtype=torch.int32)
    d.u = torch.randint(0, A, (N, n), generator=g).to(torch.int8)
    d.r = torch.randn(N, generator=g)
    d.avail = (torch.rand(N, n, A, generator=g) < 0.7).to(torch.int8)
    if starve:
        d.avail[torch.rand(N, n, generator=g) < 0.25] = 0
    else:
        d.avail.scatter_(2, torch.randint(0, A, (N, n, 1), generator=g), 1)
    d.term = (torch.rand(N, generator=g) < 0.2).to(torch.uint8)
    d.padded = (torch.rand(N, generator=g) < 0.3).to(torch.uint8)
    rows = -(-U * n // 64) * 64
    d.q_e, d.q_t = torch.randn(rows, A, generator=g), torch.randn(rows, A, generator=g)
    d.q_e[U * n:] = float('nan')
    d.q_t[U * n:] = float('nan')
    return d


def _to_gpu(d):
    return types.SimpleNamespace(**{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in vars(d).items()})


def _td_reference(d, ep):
    """float64 restatement of include/vdn_ops.h for the units `ep` (flat slot * TL + t, one per group of n Q rows, in row order):
    masked TD error, mask, the derived per-element bound 4 (2n + 3) 2^-24 (|r| + sum_i |q_e taken| + gamma sum_i |max q_t|) and the
    float64 gradient of sum(mtd^2) * G_NUM w.r.t. q_e."""
    n, A, U = d.n, d.A, ep.numel()
    ep = ep.long()
    qe = d.q_e[:U * n].double().view(U, n, A)
    qt = d.q_t[:U * n].double().view(U, n, A)
    act = d.u[ep].long()                                                   # (U, n)
    taken = qe.gather(2, act.clamp(0, A - 1).unsqueeze(2)).squeeze(2)
    tmax = qt.masked_fill(d.avail[ep] == 0, -9999999.0).max(2).values      # (U, n)
    mask = 1.0 - d.padded[ep].double()
    target = d.r[ep].double() + GAMMA * tmax.sum(1) * (1.0 - d.term[ep].double())
    mtd = mask * (target - taken.sum(1))
    bound = 4 * (2 * n + 3) * U24 * (d.r[ep].double().abs() + taken.abs().sum(1) + GAMMA * tmax.abs().sum(1))
    g64 = float(np.float32(G_NUM))
    gq = torch.zeros(U, n, A, dtype=torch.float64)
    gq.scatter_(2, act.clamp(0, A - 1).unsqueeze(2), (-(2.0 * mtd * mask) * g64).view(U, 1, 1).expand(U, n, 1))
    return mtd, mask, bound, gq


def _packed_forward(lib, dg, counter=True):
    U = dg.U
    mtd, mask = _out(U), _out(U)
    cnt = torch.zeros(1 + GUARD, dtype=torch.int32, device='cuda')
    rc = lib.vdn_td_forward_packed(_p(dg.q_e), _p(dg.q_t), _p(dg.units), U, _p(dg.u), _p(dg.r), _p(dg.avail), _p(dg.term), _p(dg.padded),
                                   dg.n, dg.A, GAMMA, _p(mtd), _p(mask), _p(cnt) if counter else None, None)
    assert rc == 0
    torch.cuda.synchronize()
    _written_inside(mtd, U)
    _written_inside(mask, U)
    assert bool((cnt[1:] == 0).all())
    return mtd, mask, int(cnt[0])


def _packed_backward(lib, dg, mtd, mask):
    U, n, A = dg.U, dg.n, dg.A
    gq = _out(U * n * A)
    gnum = torch.full((1,), G_NUM, device='cuda')
    rc = lib.vdn_td_backward_packed(_p(mtd), _p(mask), _p(dg.units), U, _p(dg.u), _p(gnum), n, A, _p(gq), None)
    assert rc == 0
    torch.cuda.synchronize()
    _written_inside(gq, U * n * A)
    return gq, gnum


def _scatter_expected(dg, ep, mtd, mask, gnum):
    """What the backward must leave, from the kernel's OWN mtd in float32: products only, so bit-exact."""
    U, n, A = ep.numel(), dg.n, dg.A
    dval = (-((2.0 * mtd[:U]) * mask[:U])) * gnum[0]
    want = torch.zeros(U, n, A, device='cuda')
    want.scatter_(2, dg.u[ep.long()].long().unsqueeze(2), dval.view(U, 1, 1).expand(U, n, 1))
    return want


TD_CASES = [(1, 1, 1), (3, 5, 255), (10, 9, 256), (4, 127, 257), (3, 5, 700), (10, 9, 1), (4, 127, 700), (1, 1, 257)]


@pytest.mark.parametrize('n,A,U', TD_CASES)
@pytest.mark.parametrize('starve', [False, True], ids=['avail', 'starved'])
def test_td_packed_matches_float64(n, A, U, starve):
    """vdn_td_forward_packed / vdn_td_backward_packed on an unsorted unit list with repeats, padded ~30 %, terminated ~20 %,
    avail ~70 % (starved: a quarter of the agents with no available action, whose maximum is the -9999999 fill), NaN in the Q rows
    behind the last unit.  mask exact; mtd per element within the derived bound; the gradient bit-exact from the kernel's own mtd
    and within 2 |g| x that bound of float64."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_ops()
    d = _td_inputs(n, A, U, seed=1000 * n + 10 * A + U + (7 if starve else 0), starve=starve)
    if starve and U > 50:
        assert bool((d.avail[d.units.long()].sum(2) == 0).any())
    dg = _to_gpu(d)
    mtd_ref, mask_ref, bound, gq_ref = _td_reference(d, d.units)
    mtd, mask, bad = _packed_forward(lib, dg)
    assert bad == 0
    assert torch.equal(mask[:U].cpu().double(), mask_ref)
    if U > 50:
        assert 0 < int(mask_ref.sum()) < U and 0 < int(d.term[d.units.long()].sum()) < U      # both factors non-trivial
    err = (mtd[:U].cpu().double() - mtd_ref).abs()
    print('td packed n=%d A=%d U=%d starved=%s: max err / bound = %.3f' % (n, A, U, starve, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), float((err - bound).max())
    gq, gnum = _packed_backward(lib, dg, mtd, mask)
    got = gq[:U * n * A].view(U, n, A)
    assert torch.equal(got, _scatter_expected(dg, dg.units, mtd, mask, gnum))       # taken action: the product; every other: 0
    gerr = (got.cpu().double() - gq_ref).abs()
    assert bool((gerr <= (2 * G_NUM * bound).view(U, 1, 1)).all())


@pytest.mark.parametrize('n,A', [(3, 5), (4, 127)])
def test_td_packed_equals_unpacked_on_a_full_rectangle(n, A):
    """B = 9 full episodes of T = t_limit = 7 steps, units[t * B + b] = b * t_limit + t, the same Q memory: the packed kernels and
    vdn_td_forward / vdn_td_backward evaluate identical source expressions, so mtd (index transposed), mask and the gradient are
    bit-identical (the library is built with -ffp-contract=off, so neither side fuses a multiply-add the other does not).  The unpacked forward also gets the per-element float64 check that
    tests/test_gpu_td_fused.py lacks (it compares the scalar sum only)."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_ops()
    B, T = 9, TL
    U = B * T
    d = _td_inputs(n, A, U, seed=77 + A)
    tb = torch.arange(U)
    d.units = ((tb % B) * TL + tb // B).to(torch.int32)
    dg = _to_gpu(d)
    mtd_p, mask_p, bad = _packed_forward(lib, dg)
    gq_p, gnum = _packed_backward(lib, dg, mtd_p, mask_p)
    mtd_u, mask_u, gq_u = _out(U), _out(U), _out(U * n * A)
    cnt = torch.zeros(1, dtype=torch.int32, device='cuda')
    assert lib.vdn_td_forward(_p(dg.q_e), _p(dg.q_t), _p(dg.u), _p(dg.r), _p(dg.avail), _p(dg.term), _p(dg.padded), B, T, TL, n, A,
                              GAMMA, _p(mtd_u), _p(mask_u), _p(cnt), None) == 0
    assert lib.vdn_td_backward(_p(mtd_u), _p(mask_u), _p(dg.u), _p(gnum), B, T, TL, n, A, _p(gq_u), None) == 0
    torch.cuda.synchronize()
    for buf, k in ((mtd_u, U), (mask_u, U), (gq_u, U * n * A)):
        _written_inside(buf, k)
    assert bad == 0 and int(cnt[0]) == 0
    # unpacked index b * T + t -> packed index t * B + b
    assert torch.equal(mtd_u[:U].view(B, T).t().reshape(-1), mtd_p[:U])
    assert torch.equal(mask_u[:U].view(B, T).t().reshape(-1), mask_p[:U])
    assert torch.equal(gq_u[:U * n * A], gq_p[:U * n * A])          # both time-major
    mtd_ref, mask_ref, bound, gq_ref = _td_reference(d, d.units)
    got = mtd_u[:U].view(B, T).t().reshape(-1).cpu().double()
    assert bool(((got - mtd_ref).abs() <= bound).all())
    assert torch.equal(mask_u[:U].view(B, T).t().reshape(-1).cpu().double(), mask_ref)
    gerr = (gq_u[:U * n * A].view(U, n, A).cpu().double() - gq_ref).abs()
    assert bool((gerr <= (2 * G_NUM * bound).view(U, 1, 1)).all())


@pytest.mark.parametrize('n,A', [(3, 5), (4, 127)])
def test_td_packed_bad_actions_poison_and_are_counted(n, A):
    """u == A, u == -1 and (A = 127) u == -128 in three different (slot, step) units of the ring, each drawn several times by a
    300-unit list: the counter equals the number of drawn units that hold one, mtd is NaN exactly there, the gradient is NaN in the
    offending agent's whole row and at the taken action of the unit's other agents, everything else is finite; a NULL counter is
    accepted."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_ops()
    U = 300
    d = _td_inputs(n, A, U, seed=5 + A)
    eps = [12, 40, 63][:3 if A == 127 else 2]
    vals = [A, -1, -128]
    agents = [1, 0, n - 1]
    for e, v, i in zip(eps, vals, agents):
        d.u[e, i] = v
    d.units[[3, 256, 299][:len(eps)]] = torch.tensor(eps, dtype=torch.int32)      # each is drawn at least once, in two blocks
    d.padded[eps[0]] = 1                                                           # a padded unit is poisoned all the same
    dg = _to_gpu(d)
    is_bad = torch.isin(d.units.long(), torch.tensor(eps))
    mtd, mask, bad = _packed_forward(lib, dg)
    assert bad == int(is_bad.sum()) >= len(eps)
    assert torch.equal(torch.isnan(mtd[:U]).cpu(), is_bad)
    assert bool(torch.isfinite(mtd[:U].cpu()[~is_bad]).all())
    mtd2, mask2, _ = _packed_forward(lib, dg, counter=False)
    assert torch.equal(torch.isnan(mtd2[:U]), torch.isnan(mtd[:U])) and torch.equal(mtd2[:U].nan_to_num(0.0), mtd[:U].nan_to_num(0.0))
    assert torch.equal(mask2[:U], mask[:U])
    gq, _ = _packed_backward(lib, dg, mtd, mask)
    got = torch.isnan(gq[:U * n * A].view(U, n, A)).cpu()
    act = d.u[d.units.long()].long()                                               # (U, n)
    off = (act < 0) | (act >= A)
    taken = torch.zeros(U, n, A, dtype=torch.bool).scatter_(2, act.clamp(0, A - 1).unsqueeze(2), True) & ~off.unsqueeze(2)
    want = is_bad.view(U, 1, 1) & (off.unsqueeze(2) | taken)
    assert torch.equal(got, want)
    assert bool(torch.isfinite(gq[:U * n * A].view(U, n, A).cpu()[~want]).all())


# ------------------------------------------------------------------------------------------------------------------------------
# 2. vdn_gather_units
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('unit_bytes,src_off,dst_off', [(980, 0, 0), (20, 0, 0), (4, 0, 0), (735, 0, 0), (15, 0, 0), (1, 0, 0), (980, 1, 0), (980, 0, 2)])
def test_gather_units_is_an_exact_index_expression(unit_bytes, src_off, dst_off):
    """dst unit j = src unit units[j] + shift, zeros for j < zero_below, for the dword kernel (unit_bytes % 4 == 0, both pointers
    4-aligned) and the byte kernel (everything else, including a multiple of 4 at a misaligned source or destination).  The source
    units sit between two spare units of 0x7f, a byte no real unit holds: a lost or doubled shift shows up as 0x7f or as the wrong
    unit.  dst is pre-filled with 0x55 and lies inside a larger allocation that must keep that fill."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_ops()
    n_src = 40
    g = torch.Generator().manual_seed(unit_bytes + 3 * src_off + 5 * dst_off)
    real = torch.randint(-128, 127, (n_src, unit_bytes), generator=g).to(torch.int8).cuda()          # never 0x7f
    big = torch.full((src_off + (n_src + 2) * unit_bytes + 64,), 0x7f, dtype=torch.int8, device='cuda')
    big[src_off + unit_bytes: src_off + (n_src + 1) * unit_bytes] = real.view(-1)
    src_ptr = big.data_ptr() + src_off + unit_bytes
    assert big.data_ptr() % 256 == 0
    for U in (1, 257, 1000):
        for shift in (0, -1, 1):
            for zb in (0, 5, U, U + 3):
                units = torch.randint(1 if shift < 0 else 0, n_src - 1 if shift > 0 else n_src, (U,), generator=g, dtype=torch.int32)
                units[:zb] = 0                           # never read: with shift -1 they would point at the spare unit in front
                units = units.cuda()
                dst = torch.full((dst_off + U * unit_bytes + GUARD,), 0x55, dtype=torch.int8, device='cuda')
                assert dst.data_ptr() % 256 == 0
                rc = lib.vdn_gather_units(C.c_void_p(src_ptr), unit_bytes, _p(units), U, shift, zb, C.c_void_p(dst.data_ptr() + dst_off), None)
                assert rc == 0
                want = real[(units.long() + shift).clamp(0, n_src - 1)]
                want[:zb] = 0
                body = dst[dst_off: dst_off + U * unit_bytes]
                assert torch.equal(body.view(U, unit_bytes), want), (U, shift, zb)
                assert not bool((body == 0x7f).any())
                assert bool((dst[:dst_off] == 0x55).all()) and bool((dst[dst_off + U * unit_bytes:] == 0x55).all()), (U, shift, zb)
    dst = torch.full((64,), 0x55, dtype=torch.int8, device='cuda')
    units = torch.zeros(4, dtype=torch.int32, device='cuda')
    assert lib.vdn_gather_units(C.c_void_p(src_ptr), unit_bytes, _p(units), 0, 0, 0, _p(dst), None) == 0
    torch.cuda.synchronize()
    assert bool((dst == 0x55).all())


# ------------------------------------------------------------------------------------------------------------------------------
# 3. vdn_clip_adam_step
# ------------------------------------------------------------------------------------------------------------------------------
LR, BETA1, BETA2, EPS = 5e-4, 0.9, 0.99, 1e-8


def _network_numels():
    from marl_dmfb_amd.network.base_net import CRNN
    a = types.SimpleNamespace(obs_shape=(3, 9, 9, 2, 245), hyper_hidden_dim=24, rnn_hidden_dim=128, n_actions=5, fov=9)
    return [p.numel() for p in CRNN(a).parameters()]


def _many_tiny_numels():
    cyc = (1, 2, 3, 5, 255, 256, 257, 1023, 1024, 1025, 4097)
    return [cyc[k % len(cyc)] for k in range(32)]


class _AdamState:
    """Parameters, gradients and both moments as views at the head of sentinel-filled allocations, plus the C arrays of the call."""

    def __init__(self, numels, gen):
        self.numels = numels
        self.bufs = {k: [_out(m) for m in numels] for k in 'pgmv'}
        self.p, self.g, self.m, self.v = ([b[:m] for b, m in zip(self.bufs[k], numels)] for k in 'pgmv')
        for p, m, v in zip(self.p, self.m, self.v):
            p.copy_(torch.randn(p.shape, device='cuda', generator=gen) * 0.1)
            m.zero_()
            v.zero_()
        self.partials = _out(128)
        self.norm = _out(1)
        n = len(numels)
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        self.args = (arr(self.p), arr(self.g), arr(self.m), arr(self.v), (C.c_int64 * n)(*numels))

    def step(self, lib, k, clip, div):
        rc = lib.vdn_clip_adam_step(len(self.numels), *self.args, clip, LR, BETA1, BETA2, EPS, 1.0 - BETA1 ** k, 1.0 - BETA2 ** k,
                                    _p(self.partials), _p(self.norm), _p(div), None)
        torch.cuda.synchronize()
        return rc

    def guards_intact(self):
        for k in 'pgmv':
            for b, m in zip(self.bufs[k], self.numels):
                assert bool((b[m:] == SENT).all()), 'written past the end of a tensor'
        assert bool((self.partials[128:] == SENT).all()) and bool((self.norm[1:] == SENT).all())


def _same_class_and_close(got, want, tol, what):
    """NaN and non-finite masks equal torch's; the finite values within tol (a tensor)."""
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what
    assert torch.equal(torch.isfinite(got), torch.isfinite(want)), what
    f = torch.isfinite(want)
    d = (got - want).abs()
    assert bool((d[f] <= tol[f]).all()), (what, float((d[f] - tol[f]).max()))


def _clip_adam_against_torch(numels, clip, grad_div, seed, poison=None, steps=3):
    """`steps` steps, each from identical state, against _foreach_div_ + clip_grad_norm_ + Adam(fused=True) on the same device, with
    the tolerances of tests/test_gpu_td_fused.py::test_two_launch_clip_and_adam_equals_torch_clip_and_adam: norm rtol 1e-5, the
    parameter update within 2e-6 of its own size + one ulp of the parameter, both moments 1e-6 relative to their operands; the
    gradients left in memory rtol 1e-5 (they carry the norm's tolerance through the clip coefficient).  poison = (step, value): one
    gradient element of that step is NaN / inf; then the NaN and finite masks must equal torch's as well."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_ops()
    gen = torch.Generator(device='cuda').manual_seed(seed)
    st = _AdamState(numels, gen)
    refs = [torch.nn.Parameter(p.clone()) for p in st.p]
    opt = torch.optim.Adam(refs, lr=LR, betas=(BETA1, BETA2), eps=EPS, fused=True)
    div = None if grad_div is None else torch.full((1,), grad_div, device='cuda')
    for k in range(1, steps + 1):
        grads = []
        for p in st.p:
            mag = 10.0 ** torch.empty_like(p).uniform_(-12.0, 0.0, generator=gen)
            grads.append(mag * torch.sign(torch.randn(p.shape, device='cuda', generator=gen)))
        if poison is not None and poison[0] == k:
            t = len(numels) // 2
            grads[t][numels[t] // 3] = poison[1]
        for g, r, mine in zip(grads, refs, st.g):
            r.grad = g.clone()
            mine.copy_(g)
        before = [r.detach().clone() for r in refs]
        if div is not None:
            torch._foreach_div_([r.grad for r in refs], div.reshape(()))
        want_norm = torch.nn.utils.clip_grad_norm_(refs, clip)
        opt.step()
        assert st.step(lib, k, clip, div) == 0
        st.guards_intact()
        got_norm = st.norm[0]
        if bool(torch.isfinite(want_norm)):
            np.testing.assert_allclose(float(got_norm), float(want_norm), rtol=1e-5)
        else:
            assert bool(torch.isnan(got_norm)) == bool(torch.isnan(want_norm)) and bool(torch.isinf(got_norm)) == bool(torch.isinf(want_norm))
            assert poison is not None
        for t, (p, r, b) in enumerate(zip(st.p, refs, before)):
            rd, s = r.detach(), opt.state[r]
            what = (t, k)
            _same_class_and_close(st.g[t], r.grad, 1e-5 * r.grad.abs(), ('grad',) + what)
            _same_class_and_close(p, rd, 2e-6 * (rd - b).abs() + 1.2e-7 * rd.abs() + 1e-9, ('param',) + what)
            _same_class_and_close(st.m[t], s['exp_avg'], 1e-6 * (s['exp_avg'].abs() + 0.2 * r.grad.abs()).clamp_min(1e-37), ('m',) + what)
            _same_class_and_close(st.v[t], s['exp_avg_sq'], 1e-6 * s['exp_avg_sq'].abs().clamp_min(1e-37), ('v',) + what)
            if div is None and poison is None and float(want_norm) + 1e-6 < clip:
                assert torch.equal(st.g[t], grads[t]), what            # coefficient 1 and no divisor: p.grad is not rewritten
            # next step from identical state
            p.copy_(rd)
            st.m[t].copy_(s['exp_avg'])
            st.v[t].copy_(s['exp_avg_sq'])
    return st


@pytest.mark.parametrize('clip', [1.0e6, 0.05])
def test_clip_adam_with_grad_div_network_shapes(clip):
    """(a) the network's tensor list with d_grad_div = 37, the branch every shipped learn takes, with and without the clip biting."""
    _clip_adam_against_torch(_network_numels(), clip, 37.0, seed=11)


@pytest.mark.parametrize('clip,grad_div', [(1.0e6, None), (0.05, 37.0), (0.05, None)])
def test_clip_adam_single_one_element_tensor(clip, grad_div):
    """(b) one tensor of one element: one block, one thread with work."""
    _clip_adam_against_torch([1], clip, grad_div, seed=12)


@pytest.mark.parametrize('clip,grad_div', [(0.05, 37.0), (1.0e6, 37.0), (0.05, None)])
def test_clip_adam_walks_32_tiny_tensors(clip, grad_div):
    """(c) VDN_MAX_TENSORS tensors of 1 .. 4097 elements: tensor boundaries inside a thread's 256-stride and inside a block's chunk,
    several tensors within one stride (locate() advances more than one tensor at a time), a total that is a multiple of nothing."""
    numels = _many_tiny_numels()
    assert len(numels) == 32 and sum(numels) % 2 == 1
    _clip_adam_against_torch(numels, clip, grad_div, seed=13)


def test_clip_adam_leaves_the_gradient_alone_at_coefficient_one():
    """(d) no divisor and a norm below max_norm: p.grad is bit-unchanged (asserted inside the comparison)."""
    _clip_adam_against_torch(_many_tiny_numels()[:12], 1.0e6, None, seed=14)


@pytest.mark.parametrize('value', [float('nan'), float('inf')], ids=['nan', 'inf'])
@pytest.mark.parametrize('grad_div', [None, 37.0])
def test_clip_adam_nonfinite_norm_follows_torch(value, grad_div):
    """(e) one NaN gradient element: the norm and with it every gradient, moment and parameter is NaN, as clip_grad_norm_ makes them.
    One +inf: the norm is inf, the coefficient 0, the element itself inf * 0 = NaN and every other gradient 0.  The poisoned step is
    the second of three, so finite and non-finite state is carried into a further step."""
    _clip_adam_against_torch(_many_tiny_numels()[:12], 0.05, grad_div, seed=15, poison=(2, value))


def test_clip_adam_argument_checks_touch_nothing():
    """(f) n_tensors = 33, a zero numel, bias_correction2 = 0 and a NULL list: VDN_ERR_BAD_ARG, every buffer as it was."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_ops()
    gen = torch.Generator(device='cuda').manual_seed(16)
    numels = [5, 300, 7]
    st = _AdamState(numels, gen)
    for g in st.g:
        g.copy_(torch.randn(g.shape, device='cuda', generator=gen))
    div = torch.full((1,), 37.0, device='cuda')
    snap = {k: [b.clone() for b in st.bufs[k]] for k in 'pgmv'}
    n = len(numels)
    arr33 = lambda ts: (C.c_void_p * 33)(*[ts[k % n].data_ptr() for k in range(33)])
    common = (0.05, LR, BETA1, BETA2, EPS, 0.1, 0.01, _p(st.partials), _p(st.norm), _p(div), None)
    p_, g_, m_, v_, ne_ = st.args
    assert lib.vdn_clip_adam_step(33, arr33(st.p), arr33(st.g), arr33(st.m), arr33(st.v), (C.c_int64 * 33)(*[numels[k % n] for k in range(33)]),
                                  *common) == BAD_ARG
    assert lib.vdn_clip_adam_step(n, p_, g_, m_, v_, (C.c_int64 * n)(5, 0, 7), *common) == BAD_ARG
    assert lib.vdn_clip_adam_step(n, p_, g_, m_, v_, ne_, 0.05, LR, BETA1, BETA2, EPS, 0.1, 0.0, _p(st.partials), _p(st.norm), _p(div), None) == BAD_ARG
    for hole in range(5):
        a = [p_, g_, m_, v_, ne_]
        a[hole] = None
        assert lib.vdn_clip_adam_step(n, *a, *common) == BAD_ARG
    torch.cuda.synchronize()
    for k in 'pgmv':
        for b, s in zip(st.bufs[k], snap[k]):
            assert torch.equal(b, s)
    _untouched(st.partials)
    _untouched(st.norm)
    assert st.step(lib, 1, 0.05, div) == 0                       # the same state is accepted once the arguments are right
    assert bool(torch.isfinite(st.norm[0]))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the packed GRU sequence kernels
# ------------------------------------------------------------------------------------------------------------------------------
H = 128


def _steps(step_rows):
    return (C.c_int32 * len(step_rows))(*step_rows)


def _gru_inputs(R, step_rows, seed, scale=1.0):
    torch.manual_seed(seed)
    V = sum(step_rows)
    d = types.SimpleNamespace(R=R, step_rows=list(step_rows), T=len(step_rows), V=V)
    d.cells = [torch.nn.GRUCell(H, H).cuda() for _ in range(2)]          # default init: uniform(-1/sqrt(H), 1/sqrt(H))
    for c in d.cells:
        c.requires_grad_(False)
    d.ig = [torch.randn(V, 3 * H, device='cuda') * scale for _ in range(2)]
    d.h0 = [torch.rand(R, H, device='cuda') * 2 - 1 for _ in range(2)]
    d.gout = torch.randn(V, H, device='cuda')
    return d


def _gru_reference(d, k, grads):
    """nn.GRUCell's formulas unrolled in float64 on the rows still running (network/base_net.py:56,69; policy/vdn.py:174-191) for
    network k: hs (V, H), and with grads=True the float64 autograd gradients of sum(hs * gout) w.r.t. igates, h0, W_hh, b_ih, b_hh."""
    c = d.cells[k]
    leaf = lambda t: t.detach().double().cpu().requires_grad_(grads)
    ig, h0, w, bi, bh = leaf(d.ig[k]), leaf(d.h0[k]), leaf(c.weight_hh), leaf(c.bias_ih), leaf(c.bias_hh)
    h, outs, off = h0, [], 0
    with torch.set_grad_enabled(grads):
        for rt in d.step_rows:
            gi = ig[off:off + rt] + bi
            gh = h[:rt] @ w.t() + bh
            r_ = torch.sigmoid(gi[:, :H] + gh[:, :H])
            z_ = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
            n_ = torch.tanh(gi[:, 2 * H:] + r_ * gh[:, 2 * H:])
            hn = (1 - z_) * n_ + z_ * h[:rt]
            outs.append(hn)
            h = torch.cat([hn, h[rt:]], 0)
            off += rt
        hs = torch.cat(outs, 0)
        if not grads:
            return hs, None
        (hs * d.gout.double().cpu()).sum().backward()
    return hs.detach(), (ig.grad, h0.grad, w.grad, bi.grad, bh.grad)


def _gru_forward(lib, d, kind, k=0):
    """hs and gates buffers of network k from gru_seq_forward_packed ('valu') or gru_seq_forward_packed_pair ('mfma', both networks
    in one launch; returns network k's)."""
    c, V = d.cells, d.V
    if kind == 'valu':
        hs, gates = _out(V * H), _out(V * 4 * H)
        rc = lib.gru_seq_forward_packed(_p(d.ig[k]), _p(d.h0[k]), _p(c[k].weight_hh), _p(c[k].bias_ih), _p(c[k].bias_hh), d.T, d.R, H,
                                        _steps(d.step_rows), _p(hs), _p(gates), None)
        outs = [(hs, gates)]
    else:
        outs = [(_out(V * H), _out(V * 4 * H)) for _ in range(2)]
        a = []
        for j in range(2):
            a += [_p(d.ig[j]), _p(d.h0[j]), _p(c[j].weight_hh), _p(c[j].bias_ih), _p(c[j].bias_hh), _p(outs[j][0]), _p(outs[j][1])]
        rc = lib.gru_seq_forward_packed_pair(*a, d.T, d.R, H, _steps(d.step_rows), None)
    assert rc == 0
    torch.cuda.synchronize()
    for hs, gates in outs:
        _written_inside(hs, V * H)
        _written_inside(gates, V * 4 * H)
    return outs[k if kind == 'mfma' else 0]


def _gru_backward(lib, d, k, hs, gates):
    V, R = d.V, d.R
    nb = int(lib.gru_seq_row_blocks(R))
    o = types.SimpleNamespace(d_ig=_out(V * 3 * H), d_hg=_out(V * 3 * H), d_h0=_out(R * H), bias=_out(nb * 6 * H), h_prev=_out(V * H))
    rc = lib.gru_seq_backward_packed(_p(d.gout), _p(gates), _p(hs), _p(d.h0[k]), _p(d.cells[k].weight_hh), d.T, R, H, _steps(d.step_rows),
                                     _p(o.d_ig), _p(o.d_hg), _p(o.d_h0), _p(o.bias), _p(o.h_prev), None)
    assert rc == 0
    torch.cuda.synchronize()
    for buf, m in ((o.d_ig, V * 3 * H), (o.d_hg, V * 3 * H), (o.d_h0, R * H), (o.bias, nb * 6 * H), (o.h_prev, V * H)):
        _written_inside(buf, m)
    return o, nb


def _rel_l2_ok(got, want, tol=2e-4):
    return bool(torch.linalg.norm(got.double().cpu() - want) <= tol * torch.linalg.norm(want) + 1e-9)


RAGGED = [(9, [9, 9, 8, 7, 1]), (17, [17, 17, 16, 9, 8, 1]), (33, [31, 31, 16, 15])]


@pytest.mark.parametrize('R,step_rows', RAGGED, ids=['R9', 'R17', 'R33'])
@pytest.mark.parametrize('kind', ['valu', 'mfma'])
def test_gru_packed_nonzero_h0_forward_and_backward_match_float64(R, step_rows, kind):
    """Non-zero h0 and step_rows that cut inside an 8-row (VALU) and a 16-row (matrix-core) workgroup, R = 33 with two rows that never
    run: gru_seq_forward_packed or gru_seq_forward_packed_pair (d_h0_a / d_h0_b given), then gru_seq_backward_packed on what that
    forward saved.  h within 2e-5 of float64; d_igates, d_h0, dW_hh = d_hgates^T h_prev and both bias gradients (row-block partial
    sums added) at relative L2 2e-4 against float64 autograd; d_h0 exactly 0 on the rows that never run; the two forward kernels
    agree within 1e-5 on h and on the saved gates."""
    from marl_dmfb_amd import _lib
    lib = _lib.crnn_ops()
    d = _gru_inputs(R, step_rows, seed=100 + R)
    V = d.V
    hs_ref, (g_ig, g_h0, g_w, g_bi, g_bh) = _gru_reference(d, 0, grads=True)
    hs, gates = _gru_forward(lib, d, kind, 0)
    np.testing.assert_allclose(hs[:V * H].view(V, H).cpu().numpy(), hs_ref.numpy(), rtol=0, atol=2e-5)
    if kind == 'mfma':
        hs_b, _ = _gru_forward(lib, d, kind, 1)
        np.testing.assert_allclose(hs_b[:V * H].view(V, H).cpu().numpy(), _gru_reference(d, 1, grads=False)[0].numpy(), rtol=0, atol=2e-5)
        hs_v, gates_v = _gru_forward(lib, d, 'valu', 0)
        np.testing.assert_allclose(hs[:V * H].cpu().numpy(), hs_v[:V * H].cpu().numpy(), rtol=0, atol=1e-5)
        np.testing.assert_allclose(gates[:V * 4 * H].cpu().numpy(), gates_v[:V * 4 * H].cpu().numpy(), rtol=0, atol=1e-5)
    o, nb = _gru_backward(lib, d, 0, hs, gates)
    d_h0 = o.d_h0[:R * H].view(R, H)
    assert bool((d_h0[step_rows[0]:] == 0).all())                                   # rows that never run: written, with exact zeros
    assert bool((g_h0[step_rows[0]:] == 0).all())
    assert _rel_l2_ok(o.d_ig[:V * 3 * H].view(V, 3 * H), g_ig)
    assert _rel_l2_ok(d_h0, g_h0)
    d_hg = o.d_hg[:V * 3 * H].view(V, 3 * H).double().cpu()
    assert _rel_l2_ok(d_hg.t() @ o.h_prev[:V * H].view(V, H).double().cpu(), g_w)
    bias = o.bias[:nb * 6 * H].view(nb, 6 * H).double().cpu().sum(0)
    assert _rel_l2_ok(bias[:3 * H], g_bi) and _rel_l2_ok(bias[3 * H:], g_bh)


@pytest.mark.parametrize('kind', ['valu', 'mfma'])
def test_gru_packed_longest_sequence(kind):
    """T = GRU_SEQ_MAX_STEPS = 255 full-length steps, R = 9, h0 uniform in [-1, 1]: h of every step within 2e-5 of float64.  (A
    float32 unrolling of the same cell on the CPU stays within 2.6e-7 of float64 on such inputs, so 2e-5 is two orders of magnitude
    of room and still far below a wrong step offset.)"""
    from marl_dmfb_amd import _lib
    lib = _lib.crnn_ops()
    d = _gru_inputs(9, [9] * 255, seed=255)
    hs_ref, _ = _gru_reference(d, 0, grads=False)
    hs, _ = _gru_forward(lib, d, kind, 0)
    np.testing.assert_allclose(hs[:d.V * H].view(d.V, H).cpu().numpy(), hs_ref.numpy(), rtol=0, atol=2e-5)


def _gru_packed_calls(lib, d, T, R, step_rows):
    """Return codes of the three packed entry points for (T, R, step_rows) on buffers that must stay untouched."""
    c, k = d.cells[0], max(d.V, 1)
    hs, gates = _out(k * H), _out(k * 4 * H)
    outs = [_out(k * 3 * H), _out(k * 3 * H), _out(d.R * H), _out(int(lib.gru_seq_row_blocks(d.R)) * 6 * H), _out(k * H)]
    st = _steps(step_rows)
    rcs = [lib.gru_seq_forward_packed(_p(d.ig[0]), _p(d.h0[0]), _p(c.weight_hh), _p(c.bias_ih), _p(c.bias_hh), T, R, H, st, _p(hs), _p(gates), None),
           lib.gru_seq_forward_packed_pair(_p(d.ig[0]), _p(d.h0[0]), _p(c.weight_hh), _p(c.bias_ih), _p(c.bias_hh), _p(hs), _p(gates),
                                           None, None, None, None, None, None, None, T, R, H, st, None),
           lib.gru_seq_backward_packed(_p(d.gout), _p(d.ig[1]), _p(d.gout), _p(d.h0[0]), _p(c.weight_hh), T, R, H, st, *[_p(b) for b in outs], None)]
    torch.cuda.synchronize()
    for b in [hs, gates] + outs:
        _untouched(b)
    return rcs


def test_gru_packed_step_limit_and_step_rows_checks():
    """T = 256 > GRU_SEQ_MAX_STEPS: CRNN_ERR_UNSUPPORTED.  step_rows that grow, step_rows[0] > R and a negative count:
    CRNN_ERR_BAD_ARG.  All three packed entry points, nothing written."""
    from marl_dmfb_amd import _lib
    lib = _lib.crnn_ops()
    d = _gru_inputs(2, [2] * 256, seed=1)         # buffers large enough for what is refused
    d.ig[1] = torch.randn(d.V, 4 * H, device='cuda')
    assert _gru_packed_calls(lib, d, 256, 2, [2] * 256) == [UNSUPPORTED] * 3
    assert _gru_packed_calls(lib, d, 2, 2, [1, 2]) == [BAD_ARG] * 3
    assert _gru_packed_calls(lib, d, 2, 2, [3, 2]) == [BAD_ARG] * 3
    assert _gru_packed_calls(lib, d, 2, 2, [2, -1]) == [BAD_ARG] * 3
    assert _gru_packed_calls(lib, d, 1, 2, [-1]) == [BAD_ARG] * 3


@pytest.mark.parametrize('spikes', [False, True], ids=['x8', 'x8+1e4'])
def test_gru_packed_saturated_gates_stay_finite_and_accurate(spikes):
    """igates * 8 (gates deep in saturation; a float32 unrolling on the CPU is within 4e-7 of float64 there, so 2e-5 stays), and
    additionally a few entries at +/-1e4, where exp(-x) of the sigmoid overflows to inf: T = 12, R = 17, ragged.  Both forward kernels
    give h within 2e-5 of float64 and finite saved gates; every output of the backward on them is finite."""
    from marl_dmfb_amd import _lib
    lib = _lib.crnn_ops()
    step_rows = [17] * 4 + [16] * 4 + [9, 9, 8, 1]
    d = _gru_inputs(17, step_rows, seed=8, scale=8.0)
    if spikes:
        g = torch.Generator().manual_seed(9)
        for ig in d.ig:
            idx = torch.randint(0, ig.numel(), (60,), generator=g).cuda()
            ig.view(-1)[idx] = torch.where(torch.arange(60, device='cuda') % 2 == 0, 1.0e4, -1.0e4)
    V = d.V
    hs_ref, _ = _gru_reference(d, 0, grads=False)
    assert bool(torch.isfinite(hs_ref).all())
    for kind in ('valu', 'mfma'):
        hs, gates = _gru_forward(lib, d, kind, 0)
        assert bool(torch.isfinite(hs[:V * H]).all()) and bool(torch.isfinite(gates[:V * 4 * H]).all())
        np.testing.assert_allclose(hs[:V * H].view(V, H).cpu().numpy(), hs_ref.numpy(), rtol=0, atol=2e-5)
        o, nb = _gru_backward(lib, d, 0, hs, gates)
        for buf, m in ((o.d_ig, V * 3 * H), (o.d_hg, V * 3 * H), (o.d_h0, 17 * H), (o.bias, nb * 6 * H), (o.h_prev, V * H)):
            assert bool(torch.isfinite(buf[:m]).all())
