"""A null d_h0 in the packed GRU entry points (include/crnn_ops.h) stands for a zero initial state: 0.0f at the load, every later
operation unchanged, so hidden states, saved gates, Q values and gradients equal those of an explicit zero tensor in every bit.
20 rows with step rows [20, 12, 4] (three workgroups of the 8-row kernels, two of the 16-row pair kernel, a ragged last one) and
16 rows with one step."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
vp = C.c_void_p
H = 128
CASES = [(20, [20, 12, 4]), (16, [16])]


def _p(t):
    return None if t is None else vp(t.data_ptr())


def _setup(R, step_rows, seed):
    torch.manual_seed(seed)
    V = sum(step_rows)
    Vp = -(-V // 64) * 64
    cells = [torch.nn.GRUCell(H, H).cuda() for _ in range(2)]
    igs = [torch.randn(Vp, 3 * H, device='cuda') for _ in range(2)]
    for ig in igs:
        ig[V:].zero_()
    heads = [torch.nn.Linear(H, 5).cuda() for _ in range(2)]
    return V, Vp, cells, igs, heads, (C.c_int32 * len(step_rows))(*step_rows)


def _pair(lib, cells, igs, h0s, Vp, T, R, st):
    hs = [torch.full((Vp, H), 7.0, device='cuda') for _ in range(2)]
    gates = torch.full((Vp, 4 * H), 7.0, device='cuda')
    a, b = cells
    rc = lib.gru_seq_forward_packed_pair(_p(igs[0]), _p(h0s[0]), _p(a.weight_hh), _p(a.bias_ih), _p(a.bias_hh), _p(hs[0]), _p(gates),
                                         _p(igs[1]), _p(h0s[1]), _p(b.weight_hh), _p(b.bias_ih), _p(b.bias_hh), _p(hs[1]), None,
                                         T, R, H, st, None)
    assert rc == 0
    torch.cuda.synchronize()
    return hs, gates


@pytest.mark.parametrize('R,step_rows', CASES)
def test_pair_forward_null_h0_equals_explicit_zeros(R, step_rows):
    from marl_dmfb_amd import _lib
    lib = _lib.crnn_ops()
    V, Vp, cells, igs, heads, st = _setup(R, step_rows, 11 + R)
    zeros = [torch.zeros(R, H, device='cuda') for _ in range(2)]
    hs_n, gates_n = _pair(lib, cells, igs, [None, None], Vp, len(step_rows), R, st)
    hs_z, gates_z = _pair(lib, cells, igs, zeros, Vp, len(step_rows), R, st)
    for k in range(2):
        assert torch.equal(hs_n[k][:V], hs_z[k][:V])
        q_n = torch.addmm(heads[k].bias, hs_n[k][:V], heads[k].weight.t())
        q_z = torch.addmm(heads[k].bias, hs_z[k][:V], heads[k].weight.t())
        assert torch.equal(q_n, q_z)
    assert torch.equal(gates_n[:V], gates_z[:V])
    assert bool(torch.isfinite(hs_n[0][:V]).all()) and float(hs_n[0][:V].abs().max()) > 0.0


@pytest.mark.parametrize('R,step_rows', CASES)
def test_single_forward_null_h0_equals_explicit_zeros(R, step_rows):
    """gru_seq_forward_packed, and gru_seq_forward (time-major) on the first step's rows."""
    from marl_dmfb_amd import _lib
    lib = _lib.crnn_ops()
    V, Vp, cells, igs, heads, st = _setup(R, step_rows, 23 + R)
    c, T = cells[0], len(step_rows)
    outs = []
    for h0 in (None, torch.zeros(R, H, device='cuda')):
        hs = torch.full((Vp, H), 7.0, device='cuda')
        gates = torch.full((Vp, 4 * H), 7.0, device='cuda')
        assert lib.gru_seq_forward_packed(_p(igs[0]), _p(h0), _p(c.weight_hh), _p(c.bias_ih), _p(c.bias_hh), T, R, H, st, _p(hs), _p(gates),
                                          None) == 0
        hs1 = torch.full((R, H), 7.0, device='cuda')
        assert lib.gru_seq_forward(_p(igs[0]), _p(h0), _p(c.weight_hh), _p(c.bias_ih), _p(c.bias_hh), 1, R, H, _p(hs1), None, None) == 0
        torch.cuda.synchronize()
        outs.append((hs[:V], gates[:V], hs1, torch.addmm(heads[0].bias, hs[:V], heads[0].weight.t())))
    for n_, z_ in zip(*outs):
        assert torch.equal(n_, z_)
    assert torch.equal(outs[0][2][:step_rows[0]], outs[0][0][:step_rows[0]])   # step 0 of the packed run is the time-major step


@pytest.mark.parametrize('R,step_rows', CASES)
def test_pair_autograd_backward_equals_the_backward_from_explicit_zeros(R, step_rows):
    """_GRUSeqPairPacked keeps no h0 tensor and asks for no d_h0: its gradients against gru_seq_backward_packed called with an explicit
    zero h0 and a d_h0 buffer on the same forward."""
    from marl_dmfb_amd import _lib
    from marl_dmfb_amd.network.base_net import _GRUSeqPairPacked, _wgrad_splitk
    lib = _lib.crnn_ops()
    V, Vp, cells, igs, heads, st = _setup(R, step_rows, 37 + R)
    a, b = cells
    T = len(step_rows)
    ig_a = igs[0].clone().requires_grad_(True)
    hs_a, hs_b = _GRUSeqPairPacked.apply(ig_a, a.weight_hh, a.bias_ih, a.bias_hh, igs[1], b.weight_hh.detach(), b.bias_ih.detach(),
                                         b.bias_hh.detach(), step_rows, R)
    gout = torch.randn(Vp, H, device='cuda')
    gout[V:].zero_()
    (hs_a * gout).sum().backward()
    # the same forward through the C ABI with explicit zeros, then the backward with explicit zeros
    zeros = [torch.zeros(R, H, device='cuda') for _ in range(2)]
    hs_z, gates_z = _pair(lib, cells, igs, zeros, Vp, T, R, st)
    assert torch.equal(hs_z[0][:V], hs_a.detach()[:V]) and torch.equal(hs_z[1][:V], hs_b[:V])
    d_ig, d_hg = torch.zeros(Vp, 3 * H, device='cuda'), torch.zeros(Vp, 3 * H, device='cuda')
    h_prev, d_h0 = torch.zeros(Vp, H, device='cuda'), torch.zeros(R, H, device='cuda')
    bias_part = torch.empty((lib.gru_seq_row_blocks(R), 6 * H), device='cuda')
    assert lib.gru_seq_backward_packed(_p(gout), _p(gates_z), _p(hs_z[0]), _p(zeros[0]), _p(a.weight_hh), T, R, H, st, _p(d_ig), _p(d_hg),
                                       _p(d_h0), _p(bias_part), _p(h_prev), None) == 0
    torch.cuda.synchronize()
    d_b = bias_part.sum(0)
    assert torch.equal(ig_a.grad, d_ig)
    assert torch.equal(a.weight_hh.grad, _wgrad_splitk(d_hg, h_prev))
    assert torch.equal(a.bias_ih.grad, d_b[:3 * H]) and torch.equal(a.bias_hh.grad, d_b[3 * H:])
    assert float(ig_a.grad.abs().max()) > 0.0
