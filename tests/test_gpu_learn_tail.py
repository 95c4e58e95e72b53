"""The small-launch savers of the packed VDN learn against float64 torch computations of the same quantities:
  * crnn_mlp_backward as ONE launch (include/crnn_ops.h): partial vectors by row count, last-workgroup sum;
  * vdn_td_forward_sums / vdn_td_forward_packed_sums / vdn_td_backward_packed_pad and vdn_gather_units_batch (include/vdn_tail.h).
Tolerances are those of the neighbouring tests of the same kernels: GRAD_TOL of tests/test_gpu_crnn_ops.py for the mlp1 gradients,
the derived per-element bound of tests/test_gpu_packed_learn_kernels.py for the TD block (the two sums add the rounding of their own
additions, counted below), byte equality for the gather.  Every kernel with a last-workgroup tail is launched three times in a row
on the same input and must give the same bits each time (fixed summation order, the ticket word resets itself); none of the learn's
kernels runs inside a captured graph (VDN.learn_packed is launched eagerly), so there is no replay case."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import test_gpu_packed_learn_kernels as K
from test_gpu_crnn_ops import GRAD_TOL, _rel_l2

pytestmark = pytest.mark.gpu
vp = C.c_void_p


# ------------------------------------------------------------------------------------------------------------------------------
# 1. mlp1 backward
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dir_off,pad', [(243, 0), (1083, 22)], ids=['fov9', 'fov19_strided'])
@pytest.mark.parametrize('A', [0, 5, 16])
@pytest.mark.parametrize('rows', [1, 63, 64, 65, 257, 4099])
def test_mlp_backward_one_launch_matches_float64_and_repeats_bit_identically(rows, A, dir_off, pad):
    """rows: one partial vector with one wave (1, 63, 64) or two (65), two partial vectors with a ragged second workgroup (257),
    seventeen (4099).  The observation rows are strided (a wider allocation) in the fov-19 cases."""
    from marl_dmfb_amd import _lib
    lib = _lib.crnn_ops()
    g = torch.Generator(device='cuda').manual_seed(31 * rows + A + dir_off)
    obs_full = torch.randint(-4, 5, (rows, dir_off + 2 + pad), dtype=torch.int8, device='cuda', generator=g)
    obs = obs_full[:, :dir_off + 2]                                  # row stride dir_off + 2 + pad
    onehot = torch.zeros((rows, max(A, 1)), dtype=torch.int8, device='cuda')
    if A:
        onehot[torch.arange(rows, device='cuda'), torch.randint(0, A, (rows,), device='cuda', generator=g)] = 1
    onehot = onehot[:, :A].contiguous()
    col0 = 600
    cols = col0 + 10 + pad
    x = torch.randn((rows, cols), device='cuda', generator=g)
    x[:, col0:col0 + 10] = torch.relu(x[:, col0:col0 + 10])
    grad = torch.randn((rows, cols), device='cuda', generator=g)
    oh_ptr = vp(onehot.data_ptr()) if A else vp(obs.data_ptr())
    gz = (grad[:, col0:col0 + 10] * (x[:, col0:col0 + 10] > 0)).double()
    vec = torch.cat([obs[:, dir_off:dir_off + 2].double(), onehot.double()], dim=1)
    want_w, want_b = (gz.t() @ vec).cpu().numpy(), gz.sum(0).cpu().numpy()
    outs = []
    for _ in range(3):
        g_w = torch.full((10, 2 + A), float('nan'), device='cuda')
        g_b = torch.full((10,), float('nan'), device='cuda')
        part = torch.full((lib.crnn_mlp_backward_parts(),), float('nan'), device='cuda')
        rc = lib.crnn_mlp_backward(vp(obs.data_ptr()), obs.stride(0), dir_off, oh_ptr, A, rows, vp(x.data_ptr()), x.stride(0),
                                   vp(grad.data_ptr()), grad.stride(0), col0, vp(part.data_ptr()), vp(g_w.data_ptr()), vp(g_b.data_ptr()), None)
        assert rc == 0
        outs.append((g_w, g_b))
    torch.cuda.synchronize()
    ew, eb = _rel_l2(outs[0][0].cpu().numpy(), want_w), _rel_l2(outs[0][1].cpu().numpy(), want_b)
    print('mlp bwd rows=%d A=%d dir_off=%d: rel_l2 dW %.2e db %.2e' % (rows, A, dir_off, ew, eb))
    assert ew <= GRAD_TOL and eb <= GRAD_TOL
    for g_w, g_b in outs[1:]:
        assert torch.equal(g_w, outs[0][0]) and torch.equal(g_b, outs[0][1])


# ------------------------------------------------------------------------------------------------------------------------------
# 2. TD sums and the zero tail of the packed gradient
# ------------------------------------------------------------------------------------------------------------------------------
def _sum_roundings(U):
    """Additions on the longest path from a slot's square to the total: the square itself, 6 shuffle levels and 2 wave adds in the
    workgroup, then the lane-strided walk over the workgroups' pairs and 6 more shuffle levels."""
    return 1 + 6 + 2 + math.ceil(math.ceil(U / 256) / 64) + 6


def _packed_sums(lib, dg, rows_pad=None):
    U = dg.U
    mtd, mask = K._out(U), K._out(U)
    cnt = torch.zeros(1, dtype=torch.int32, device='cuda')
    part = torch.full((lib.vdn_td_sum_parts(U),), float('nan'), device='cuda')
    sums = torch.full((2 + K.GUARD,), K.SENT, device='cuda')
    rc = lib.vdn_td_forward_packed_sums(K._p(dg.q_e), K._p(dg.q_t), K._p(dg.units), U, K._p(dg.u), K._p(dg.r), K._p(dg.avail), K._p(dg.term),
                                        K._p(dg.padded), dg.n, dg.A, K.GAMMA, K._p(mtd), K._p(mask), K._p(cnt), K._p(part), K._p(sums), None)
    assert rc == 0
    torch.cuda.synchronize()
    K._written_inside(sums, 2)
    return mtd, mask, int(cnt[0]), sums[:2].clone()


@pytest.mark.parametrize('U', [1, 255, 256, 257, 2049])
def test_td_packed_sums_match_float64_and_the_gradient_tail_is_zero(U):
    """num = sum(mtd^2) and mask_sum out of the forward launch: one workgroup (1, 255, 256), two (257), nine (2049); padded ~30 %,
    terminated ~20 %.  mask_sum is a count and exact; num lies within the per-element bound of the neighbouring TD test carried
    through the squares plus the roundings of its own additions.  mtd / mask are what vdn_td_forward_packed writes, bit for bit."""
    from marl_dmfb_amd import _lib
    lib, old = _lib.vdn_tail(), _lib.vdn_ops()
    n, A = 4, 5
    d = K._td_inputs(n, A, U, seed=4242 + U)
    dg = K._to_gpu(d)
    mtd_ref, mask_ref, bound, _ = K._td_reference(d, d.units)
    runs = [_packed_sums(lib, dg) for _ in range(3)]
    mtd, mask, bad, sums = runs[0]
    for other in runs[1:]:
        assert torch.equal(other[3], sums) and torch.equal(other[0][:U], mtd[:U])       # fixed order; the ticket word reset itself
    mtd0, mask0, bad0 = K._packed_forward(old, dg)
    assert bad == 0 and bad0 == 0 and torch.equal(mtd[:U], mtd0[:U]) and torch.equal(mask[:U], mask0[:U])
    assert float(sums[1]) == float(mask_ref.sum())
    num64 = float((mtd_ref ** 2).sum())
    tol = float((2 * mtd_ref.abs() * bound + bound ** 2).sum()) + _sum_roundings(U) * K.U24 * num64
    print('td sums U=%d: num %.9g float64 %.9g err %.3g tol %.3g' % (U, float(sums[0]), num64, abs(float(sums[0]) - num64), tol))
    assert abs(float(sums[0]) - num64) <= tol
    # backward with padding rows: the buffer starts as NaN, the rows behind the last unit come out exactly zero
    rows_pad = -(-U * n // 64) * 64 + 64
    gq = torch.full((rows_pad * A + K.GUARD,), float('nan'), device='cuda')
    gnum = torch.full((1,), K.G_NUM, device='cuda')
    for _ in range(3):
        assert lib.vdn_td_backward_packed_pad(K._p(mtd), K._p(mask), K._p(dg.units), U, K._p(dg.u), K._p(gnum), n, A, rows_pad, K._p(gq), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(gq[:U * n * A].view(U, n, A), K._scatter_expected(dg, dg.units, mtd, mask, gnum))
    assert bool((gq[U * n * A: rows_pad * A] == 0).all()) and bool(torch.isnan(gq[rows_pad * A:]).all())
    assert lib.vdn_td_backward_packed_pad(K._p(mtd), K._p(mask), K._p(dg.units), U, K._p(dg.u), K._p(gnum), n, A, U * n - 1, K._p(gq), None) == K.BAD_ARG


def test_td_packed_sums_out_of_range_action_poisons_num_and_is_counted():
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_tail()
    U = 257
    d = K._td_inputs(3, 5, U, seed=99)
    d.padded[:] = 0
    d.u[int(d.units[200]), 1] = 5                     # one action outside [0, A)
    hits = int((d.units == d.units[200]).sum())
    dg = K._to_gpu(d)
    _, _, bad, sums = _packed_sums(lib, dg)
    assert bad == hits and math.isnan(float(sums[0])) and float(sums[1]) == U


@pytest.mark.parametrize('B,T', [(1, 1), (37, 7), (100, 6)])
def test_td_unpacked_sums_match_the_launch_without_them(B, T):
    """vdn_td_forward_sums: mtd / mask as vdn_td_forward writes them, the sums those of float64 over the kernel's own outputs within
    the roundings of the additions; a NULL d_sums is vdn_td_forward."""
    from marl_dmfb_amd import _lib
    lib, old = _lib.vdn_tail(), _lib.vdn_ops()
    n, A, Tl = 3, 5, 7
    g = torch.Generator().manual_seed(B * 10 + T)
    qe, qt = torch.randn(T, B, n, A, generator=g).cuda(), torch.randn(T, B, n, A, generator=g).cuda()
    u = torch.randint(0, A, (B, Tl, n, 1), generator=g).to(torch.int8).cuda()
    r = torch.randn(B, Tl, 1, generator=g).cuda()
    avail = torch.ones(B, Tl, n, A, dtype=torch.int8).cuda()
    term = (torch.rand(B, Tl, 1, generator=g) < 0.2).to(torch.uint8).cuda()
    padded = (torch.rand(B, Tl, 1, generator=g) < 0.3).to(torch.uint8).cuda()
    want_mtd, want_mask = K._out(B * T), K._out(B * T)
    assert old.vdn_td_forward(K._p(qe), K._p(qt), K._p(u), K._p(r), K._p(avail), K._p(term), K._p(padded), B, T, Tl, n, A, K.GAMMA,
                              K._p(want_mtd), K._p(want_mask), None, None) == 0
    results = []
    for with_sums in (True, True, True, False):
        mtd, mask = K._out(B * T), K._out(B * T)
        part = torch.full((lib.vdn_td_sum_parts(B * T),), float('nan'), device='cuda')
        sums = torch.full((2,), K.SENT, device='cuda')
        assert lib.vdn_td_forward_sums(K._p(qe), K._p(qt), K._p(u), K._p(r), K._p(avail), K._p(term), K._p(padded), B, T, Tl, n, A, K.GAMMA,
                                       K._p(mtd), K._p(mask), None, K._p(part) if with_sums else None, K._p(sums) if with_sums else None, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(mtd, want_mtd) and torch.equal(mask, want_mask)
        results.append(sums)
    assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2]) and bool((results[3] == K.SENT).all())
    num64 = float((want_mtd[:B * T].double() ** 2).sum())
    assert abs(float(results[0][0]) - num64) <= _sum_roundings(B * T) * K.U24 * num64
    assert float(results[0][1]) == float(want_mask[:B * T].double().sum())


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the learn's four gathers as one launch
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('U', [1, 37, 300])
def test_gather_units_batch_equals_four_single_gathers_and_zero_fills_the_padding(U):
    """o, o_next, u_onehot and the shifted u_onehot of a learn (shifts 0, 0, 0, -1; zero_below = B for the last): destinations of
    Vp rows (V rounded up to 64) pre-filled with 0x7f equal the single-tensor calls byte for byte, the padding rows are zero and
    nothing behind a destination is touched.  U = 37 runs with three agents: unit sizes that are no multiple of 4 (the byte kernel)."""
    from marl_dmfb_amd import _lib
    lib, old = _lib.vdn_tail(), _lib.vdn_ops()
    n, B, n_src = (3 if U == 37 else 4), min(U, 5), 50      # n = 3: units of 735 and 15 bytes, the byte kernel
    g = torch.Generator().manual_seed(U)
    units = torch.randint(1, n_src, (U,), generator=g, dtype=torch.int32).cuda()
    V = U * n
    Vp = -(-V // 64) * 64
    rows = [245, 245, 5, 5]
    srcs = [torch.randint(-128, 127, (n_src * n, row), generator=g).to(torch.int8).cuda() for row in rows[:3]]
    srcs.append(srcs[2])
    shifts, zbs = [0, 0, 0, -1], [0, 0, 0, B]
    unit_bytes = [n * row for row in rows]
    want = []
    for i in range(4):
        out = torch.full((U * unit_bytes[i],), 0x7f, dtype=torch.int8, device='cuda')
        assert old.vdn_gather_units(K._p(srcs[i]), unit_bytes[i], K._p(units), U, shifts[i], zbs[i], K._p(out), None) == 0
        want.append(out)
    k = 4
    for _ in range(3):
        dst_bytes = [Vp * row for row in rows]
        dsts = [torch.full((dst_bytes[i] + K.GUARD,), 0x7f, dtype=torch.int8, device='cuda') for i in range(4)]
        rc = lib.vdn_gather_units_batch(k, (vp * k)(*[t.data_ptr() for t in srcs]), (C.c_int32 * k)(*unit_bytes), (C.c_int32 * k)(*shifts),
                                        (C.c_int32 * k)(*zbs), (vp * k)(*[t.data_ptr() for t in dsts]), (C.c_int64 * k)(*dst_bytes),
                                        K._p(units), U, None)
        assert rc == 0
        torch.cuda.synchronize()
        for i in range(4):
            body = U * unit_bytes[i]
            assert torch.equal(dsts[i][:body], want[i]), i
            assert bool((dsts[i][body:dst_bytes[i]] == 0).all()) and bool((dsts[i][dst_bytes[i]:] == 0x7f).all()), i
    assert bool((want[3][:B * unit_bytes[3]] == 0).all())
    # argument checks: too many gathers, a destination shorter than its units
    assert lib.vdn_gather_units_batch(5, (vp * k)(), (C.c_int32 * k)(), (C.c_int32 * k)(), (C.c_int32 * k)(), (vp * k)(), (C.c_int64 * k)(),
                                      K._p(units), U, None) == K.BAD_ARG
    short = list(dst_bytes)
    short[0] = U * unit_bytes[0] - 1
    assert lib.vdn_gather_units_batch(k, (vp * k)(*[t.data_ptr() for t in srcs]), (C.c_int32 * k)(*unit_bytes), (C.c_int32 * k)(*shifts),
                                      (C.c_int32 * k)(*zbs), (vp * k)(*[t.data_ptr() for t in dsts]), (C.c_int64 * k)(*short), K._p(units), U,
                                      None) == K.BAD_ARG
