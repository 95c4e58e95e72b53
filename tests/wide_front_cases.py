"""Cases of the fov 11 / 13 front end (include/crnn_wide.h) shared by tests/test_gpu_crnn_wide.py, in the method of
tests/front_kernel_cases.py (whose tables end at fov 19 / 9 / 7 / 5): integer cases on which float32 arithmetic is EXACT, and
their float64 reference.  Pixels in [-2, 2], conv1 weights in {-1, 0, 1} at density 0.6, the od x od conv weights in {-1, 0, 1} at
density DENSITY, biases, mlp1 and the upstream gradient in {-1, 0, 1}: every product and partial sum, in any order, is an integer
below 2^22 (`conditions` asserts the bound from the reference run with absolute values and no ReLU)."""
import functools
import types

import torch
import torch.nn.functional as F

from front_kernel_cases import BOUND_LIMIT, MIN_POSITIVE, MIN_ZEROS, _ints

# make_case, run64, _reference and conditions restate make_case, _run, _reference and conditions of front_kernel_cases.py for the
# two-conv stride-1 stack: that file's RECIPE and _stack tables are keyed by fov and end at 5 / 7 / 9 / 19, and it may not change.
# What is generic there (_ints, guarded, the limits, N_PARTS) is imported, here and in tests/test_gpu_crnn_wide.py.
FOVS, ODS = (11, 13), (24, 32)
DENSITY = {(11, 24): 0.10, (11, 32): 0.08, (13, 24): 0.10, (13, 32): 0.08}
N_ACTIONS = 5


def n_pix(fov):
    return 3 * fov * fov


def n_conv(fov, od):
    return od * (fov - 4) ** 2


def padded_cols(fov, od):
    return (n_conv(fov, od) + 10 + 63) // 64 * 64


def n_grads(od):
    return od * od * 9 + od + od * 27 + od


def make_case(fov, od, rows):
    """Parameters depend on (fov, od) only, the rows on (fov, od, rows)."""
    g = torch.Generator().manual_seed(7000 + 10 * fov + od)
    c = types.SimpleNamespace(fov=fov, od=od, rows=rows, n_actions=N_ACTIONS)
    c.w1 = (_ints(g, (od, 3, 3, 3), -1, 1) * (torch.rand((od, 3, 3, 3), generator=g) < 0.6)).float()
    c.b1 = _ints(g, (od,), -1, 1).float()
    c.w2 = (_ints(g, (od, od, 3, 3), -1, 1) * (torch.rand((od, od, 3, 3), generator=g) < DENSITY[(fov, od)])).float()
    c.b2 = _ints(g, (od,), -1, 1).float()
    c.mlp_w = _ints(g, (10, 2 + N_ACTIONS), -1, 1).float()
    c.mlp_b = _ints(g, (10,), -1, 1).float()
    gr = torch.Generator().manual_seed(9000 + 100 * fov + od + 7 * rows)
    c.obs = _ints(gr, (rows, n_pix(fov) + 2), -2, 2).to(torch.int8)
    c.onehot = torch.zeros((rows, N_ACTIONS), dtype=torch.int8)
    act = _ints(gr, (rows,), 0, N_ACTIONS - 1)
    has = torch.rand((rows,), generator=gr) < 0.8
    c.onehot[torch.arange(rows)[has], act[has]] = 1
    c.g = _ints(gr, (rows, n_conv(fov, od) + 10), -1, 1).float()
    return c


def run64(c, absolute=False, backward=True):
    """float64 forward and autograd backward of sum(out * g); absolute: |.| of everything and no ReLU (the bound)."""
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    act = (lambda t: t) if absolute else torch.relu
    R, fov = c.rows, c.fov
    p = {k: f(getattr(c, k).double()).requires_grad_(backward) for k in ('w1', 'b1', 'w2', 'b2', 'mlp_w', 'mlp_b')}
    x = f(c.obs[:, :n_pix(fov)].double()).view(R, 3, fov, fov)
    z1 = F.conv2d(x, p['w1'], p['b1'])
    a1 = act(z1)
    z2 = F.conv2d(a1, p['w2'], p['b2'])
    a2 = act(z2)
    v = f(torch.cat([c.obs[:, n_pix(fov):], c.onehot], dim=1).double())
    out = torch.cat([a2.reshape(R, -1), act(v @ p['mlp_w'].t() + p['mlp_b'])], dim=1)
    if backward:
        a1.retain_grad()
        (out * f(c.g.double())).sum().backward()
    return p, (z1, z2), (a1, a2), out


@functools.lru_cache(maxsize=None)
def _reference(fov, od, rows, backward):
    c = make_case(fov, od, rows)
    p, zs, acts, out = run64(c, False, backward)
    r = types.SimpleNamespace(out=out.detach())
    r.zeros = [float((z == 0).double().mean()) for z in zs]
    r.positive = float((acts[1] > 0).double().mean())
    pa, _, acts_a, out_a = run64(c, True, backward)
    big = [out_a.detach(), acts_a[0].detach()]
    if backward:
        r.names = ['dW2', 'db2', 'dW1', 'db1']
        r.tensors = [p[k].grad.detach() for k in ('w2', 'b2', 'w1', 'b1')]
        r.grads = torch.cat([t.reshape(-1) for t in r.tensors])      # the flat layout of include/crnn_wide.h
        big += [acts_a[0].grad] + [t.grad for t in pa.values()]
    r.bound = max(float(t.abs().max()) for t in big)
    return r


def conditions(c, backward=True):
    """The float64 reference of `c` (cached, read-only), after asserting what makes the case exact and worth running."""
    r = _reference(c.fov, c.od, c.rows, backward)
    tag = 'fov %d od %d rows %d' % (c.fov, c.od, c.rows)
    assert r.bound < BOUND_LIMIT, (tag, r.bound)
    assert r.positive >= MIN_POSITIVE, (tag, r.positive)
    assert min(r.zeros) >= MIN_ZEROS, (tag, r.zeros)
    if backward:
        for name, t in zip(r.names, r.tensors):
            assert bool((t != 0).any()), (tag, name)
    return r
