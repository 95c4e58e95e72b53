"""Shared by tests/test_front_kernel_cases.py (CPU) and tests/test_gpu_front_kernels.py (GPU): integer cases of the CRNN front end
(network/base_net.py:23-33,59-68) on which float32 arithmetic is EXACT, and their float64 reference.

Pixels, weights, biases, one-hot and upstream gradient are small integers and the od x od conv weights are sparse, so every
product and every partial sum of the forward and of the backward -- in any order, with or without FMA contraction or the matrix
cores -- is an integer far below 2^24.  A float32 kernel and the float64 reference must then agree bit for bit; no tolerance, no
rows left out, and several percent of the pre-activations are exactly zero, so the ReLU boundary (`> 0`, gradient 0 at 0) is part
of what is compared.

`conditions(case)` states what makes a case usable and is computed from the reference alone:
  bound      the largest value the network reaches when it is run with |x|, |w|, |b|, |g| and NO ReLU, forward and backward
             (activations, their gradients, parameter gradients): every partial sum of the real computation, in any order, is at
             most that.  Required: < 2^22, a factor four under 2^24.
  positive   fraction of the final conv outputs that are > 0.  Required: >= 0.25.
  zeros      per layer, the fraction of pre-activations that are exactly 0.  Required: >= 0.01 each.
  grads      every parameter-gradient tensor of the reference is non-zero.
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

BOUND_LIMIT = 2.0 ** 22
MIN_POSITIVE, MIN_ZEROS = 0.25, 0.01
MARGIN = 256        # guard elements on each side of a guarded buffer (256 float32 keep the 16-byte alignment of the view)

# Rows per block of the kernels as the sources stand (re-derive when they move):
#   forward   crnn_mfma.h GeoM::RB 16 (od 24) / 12 (od 32); crnn_mfma19.h Geo::RB 8; crnn_fov.hip kRB 16
#   backward  crnn_ops.hip GeoB::RBB 10 / 6; crnn_bwd19.h GeoB19::RBB 4 / 2; crnn_fov.hip GeoBF::RB 8 (fov 7) / 32 (fov 5)
FWD_RB = {(9, 24): 16, (9, 32): 12, (19, 24): 8, (19, 32): 8, (7, 24): 16, (7, 32): 16, (5, 24): 16, (5, 32): 16}
BWD_RB = {(9, 24): 10, (9, 32): 6, (19, 24): 4, (19, 32): 2, (7, 24): 8, (7, 32): 8, (5, 24): 32, (5, 32): 32}


def _fov_lds_bytes(fov, od):
    """crnn_fov.hip GeoF::LDS_FLOATS * 4."""
    pad = (od * 9 + 10 + 63) // 64 * 64
    return 4 * (16 * 3 * fov * fov + (16 * (od * 25 + 1) if fov == 7 else 0) + 16 * (pad + 4) + 16 * 18 + 190)


def fwd_grid(fov, od):
    """The most workgroups a forward launches: 256 CUs x the workgroups a CU holds (fov 9 and 19: one; fov 5 / 7: launch_fwd's
    `resident`, LDS-limited)."""
    return 256 if fov in (9, 19) else 256 * (160 * 1024 // _fov_lds_bytes(fov, od))


def fwd_rows(fov, od):
    """1, RB-1, RB, RB+1 and a count at which the persistent loop wraps (every workgroup one block, workgroup 0 a second, and a
    ragged block of 5 rows (fov 19: 3) behind it)."""
    rb = FWD_RB[(fov, od)]
    return [1, rb - 1, rb, rb + 1, fwd_grid(fov, od) * rb + rb + (3 if fov == 19 else 5)]


def bwd_rows(fov, od):
    """1, RBB-1, RBB+1, 3 RBB+2, 10 RBB+3 (without repeats: RBB-1 = 1 for fov 19 / od 32)."""
    rb = BWD_RB[(fov, od)]
    return sorted({1, max(rb - 1, 1), rb + 1, 3 * rb + 2, 10 * rb + 3})


N_PARTS = (1, 2, 3, 7, 256)
# (fov, od) -> (seed, density of the od x od conv weights); the CPU test checks that every case built from them meets conditions()
RECIPE = {(9, 24): (1, 0.13), (9, 32): (2, 0.11), (19, 24): (3, 0.04), (19, 32): (4, 0.03), (7, 24): (5, 0.13), (7, 32): (6, 0.11),
          (5, 24): (7, 0.0), (5, 32): (8, 0.0)}
N_ACTIONS = 5


def n_pix(fov):
    return 3 * fov * fov


def n_conv(fov, od):
    """Conv features of a row: od x 5 x 5 for fov 9 and 19, od x 3 x 3 for fov 5 and 7."""
    return od * (25 if fov in (9, 19) else 9)


def padded_cols(fov, od):
    return (n_conv(fov, od) + 10 + 63) // 64 * 64


def n_grads(fov, od):
    return (od * od * 9 + od if fov != 5 else 0) + od * 27 + od


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g)


def make_case(fov, od, rows, n_actions=N_ACTIONS, seed=None, density=None):
    """int8 observation rows (pixels in [-2, 2], then dir_x, dir_y in [-2, 2]), an int8 one-hot of the last action (about a fifth
    of the rows without one), float32 parameters with integer values (conv1 in {-1, 0, 1} at density 0.6, the od x od conv in
    {-1, 0, 1} at `density`, biases and mlp1 in {-1, 0, 1}) and an integer upstream gradient in {-1, 0, 1} for the conv features and
    the ten vector features.  The parameters depend on (fov, od, n_actions, seed) only, not on `rows`."""
    rec = RECIPE[(fov, od)]
    seed = rec[0] if seed is None else seed
    density = rec[1] if density is None else density
    g = torch.Generator().manual_seed(1000 * seed + fov)
    c = types.SimpleNamespace(fov=fov, od=od, rows=rows, n_actions=n_actions, seed=seed, density=density)
    c.w1 = (_ints(g, (od, 3, 3, 3), -1, 1) * (torch.rand((od, 3, 3, 3), generator=g) < 0.6)).float()
    c.b1 = _ints(g, (od,), -1, 1).float()
    if fov == 5:
        c.w2 = c.b2 = None
    else:
        c.w2 = (_ints(g, (od, od, 3, 3), -1, 1) * (torch.rand((od, od, 3, 3), generator=g) < density)).float()
        c.b2 = _ints(g, (od,), -1, 1).float()
    gm = torch.Generator().manual_seed(1000 * seed + 500 + n_actions)
    c.mlp_w = _ints(gm, (10, 2 + n_actions), -1, 1).float()
    c.mlp_b = _ints(gm, (10,), -1, 1).float()
    gr = torch.Generator().manual_seed(1000 * seed + 700 + rows)
    c.obs = _ints(gr, (rows, n_pix(fov) + 2), -2, 2).to(torch.int8)
    c.onehot = torch.zeros((rows, n_actions), dtype=torch.int8)
    if n_actions > 0:
        act = _ints(gr, (rows,), 0, n_actions - 1)
        has = torch.rand((rows,), generator=gr) < 0.8
        c.onehot[torch.arange(rows)[has], act[has]] = 1
    c.g = _ints(gr, (rows, n_conv(fov, od) + 10), -1, 1).float()
    return c


def _stack(fov, x, w1, b1, w2, b2, act):
    """The conv stack of network/base_net.py:23-33 with `act` in place of the ReLU -> (pre-activations, activations)."""
    zs, acts = [], []
    z = F.conv2d(x, w1, b1, stride=2 if fov == 19 else 1)
    zs.append(z)
    acts.append(act(z))
    for _ in range({5: 0, 7: 1, 9: 1, 19: 2}[fov]):     # fov 19: conv3 twice, the SAME weights (base_net.py:31-32)
        z = F.conv2d(acts[-1], w2, b2)
        zs.append(z)
        acts.append(act(z))
    return zs, acts


def _run(c, absolute, backward=True):
    """float64 forward and (backward=True) autograd backward of sum(out * g); absolute=True: |.| of everything and no ReLU (the
    bound)."""
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    act = (lambda t: t) if absolute else torch.relu
    fov, R = c.fov, c.rows
    p = types.SimpleNamespace()
    for k in ('w1', 'b1', 'w2', 'b2', 'mlp_w', 'mlp_b'):
        t = getattr(c, k)
        setattr(p, k, None if t is None else f(t.double()).requires_grad_(backward))
    x = f(c.obs[:, :n_pix(fov)].double()).view(R, 3, fov, fov)
    zs, acts = _stack(fov, x, p.w1, p.b1, p.w2, p.b2, act)
    if backward:
        for a in acts:
            a.retain_grad()
    v = f(torch.cat([c.obs[:, n_pix(fov):n_pix(fov) + 2], c.onehot], dim=1).double())
    zv = v @ p.mlp_w.t() + p.mlp_b
    out = torch.cat([acts[-1].reshape(R, -1), act(zv)], dim=1)
    if backward:
        (out * f(c.g.double())).sum().backward()
    return p, zs, acts, zv, out


@functools.lru_cache(maxsize=None)
def _reference(fov, od, rows, n_actions, seed, density, backward):
    c = make_case(fov, od, rows, n_actions, seed, density)
    p, zs, acts, zv, out = _run(c, False, backward)
    r = types.SimpleNamespace()
    r.out = out.detach()                                   # [rows][n_conv + 10]: conv features | relu(mlp1(vec))
    r.conv = r.out[:, :n_conv(fov, od)]
    r.vec = r.out[:, n_conv(fov, od):]
    r.zeros = [float((z == 0).double().mean()) for z in zs]
    r.positive = float((r.conv > 0).double().mean())
    pa, _, acts_a, _, out_a = _run(c, True, backward)
    big = [out_a.detach()] + [a.detach() for a in acts_a]
    if not backward:                                       # a forward-only case: no sum over the rows is ever formed
        r.bound = max(float(t.abs().max()) for t in big)
        return r
    tensors = ([p.w2.grad, p.b2.grad] if fov != 5 else []) + [p.w1.grad, p.b1.grad]
    r.names = (['dW3', 'db3'] if fov == 19 else ['dW2', 'db2'] if fov != 5 else []) + ['dW1', 'db1']
    r.tensors = [t.detach() for t in tensors]
    r.grads = torch.cat([t.reshape(-1) for t in r.tensors])    # the flat layout of include/crnn_ops.h / crnn_fov.h
    r.mlp_dw, r.mlp_db = p.mlp_w.grad.detach(), p.mlp_b.grad.detach()
    big += [a.grad for a in acts_a]
    big += [t.grad for t in (pa.w1, pa.b1, pa.w2, pa.b2, pa.mlp_w, pa.mlp_b) if t is not None]
    r.bound = max(float(t.abs().max()) for t in big)
    return r


def reference(c, backward=True):
    """The float64 reference of case `c` (cached; treat as read-only): out / conv / vec and the case's `bound`, `positive`, `zeros`;
    with backward=True also the flat conv gradient `grads` with its parts `tensors` / `names` and mlp_dw / mlp_db, and `bound`
    covers the backward too."""
    return _reference(c.fov, c.od, c.rows, c.n_actions, c.seed, c.density, backward)


def conditions(c, backward=True):
    """Asserts what the module docstring requires of an exact case (backward=False: a forward-only case, no gradient taken)."""
    r = reference(c, backward)
    tag = 'fov %d od %d rows %d' % (c.fov, c.od, c.rows)
    assert r.bound < BOUND_LIMIT, (tag, r.bound)
    assert r.positive >= MIN_POSITIVE, (tag, r.positive)
    assert min(r.zeros) >= MIN_ZEROS, (tag, r.zeros)
    if backward:
        for name, t in zip(r.names + ['mlp_dw', 'mlp_db'], r.tensors + [r.mlp_dw, r.mlp_db]):
            assert bool((t != 0).any()), (tag, name)
    return r


def numpy_reference(c):
    """A second formulation that shares nothing with `reference` but the inputs: explicit loops over the taps in numpy float64,
    forward and backward (no conv2d, no autograd).  -> (out [rows][n_conv + 10], flat conv gradient, mlp dW, mlp db)."""
    fov, od, R = c.fov, c.od, c.rows
    x = c.obs[:, :n_pix(fov)].numpy().astype(np.float64).reshape(R, 3, fov, fov)

    def conv(a, w, b, s):
        n = (a.shape[2] - 3) // s + 1
        z = np.zeros((R, w.shape[0], n, n)) + b.reshape(1, -1, 1, 1)
        for kx in range(3):
            for ky in range(3):
                z += np.einsum('rcij,dc->rdij', a[:, :, kx:kx + s * n:s, ky:ky + s * n:s], w[:, :, kx, ky])
        return z

    def conv_back(dz, a, w, s):
        """-> (dW, db, da) of z = conv(a, w, b, s)."""
        n = dz.shape[2]
        dw, da = np.zeros(w.shape), np.zeros(a.shape)
        for kx in range(3):
            for ky in range(3):
                dw[:, :, kx, ky] = np.einsum('rdij,rcij->dc', dz, a[:, :, kx:kx + s * n:s, ky:ky + s * n:s])
                da[:, :, kx:kx + s * n:s, ky:ky + s * n:s] += np.einsum('rdij,dc->rcij', dz, w[:, :, kx, ky])
        return dw, dz.sum(axis=(0, 2, 3)), da

    w1, b1 = c.w1.numpy().astype(np.float64), c.b1.numpy().astype(np.float64)
    s1 = 2 if fov == 19 else 1
    layers = [(w1, b1, s1)]
    if fov != 5:
        w2, b2 = c.w2.numpy().astype(np.float64), c.b2.numpy().astype(np.float64)
        layers += [(w2, b2, 1)] * (2 if fov == 19 else 1)
    ins, zs = [x], []
    for w, b, s in layers:
        zs.append(conv(ins[-1], w, b, s))
        ins.append(np.maximum(zs[-1], 0.0))
    nc = n_conv(fov, od)
    g = c.g.numpy().astype(np.float64)
    da = g[:, :nc].reshape(ins[-1].shape)
    dw2, db2 = 0.0, 0.0
    for k in range(len(layers) - 1, -1, -1):
        dz = da * (zs[k] > 0)
        dw, db, da = conv_back(dz, ins[k], layers[k][0], layers[k][2])
        if k == 0:
            dw1, db1 = dw, db
        else:
            dw2, db2 = dw2 + dw, db2 + db       # fov 19: the two applications of conv3 add into one gradient
    v = np.concatenate([c.obs[:, n_pix(fov):].numpy(), c.onehot.numpy()], axis=1).astype(np.float64)
    zv = v @ c.mlp_w.numpy().astype(np.float64).T + c.mlp_b.numpy().astype(np.float64)
    gz = g[:, nc:] * (zv > 0)
    out = np.concatenate([ins[-1].reshape(R, -1), np.maximum(zv, 0.0)], axis=1)
    flat = ([dw2.reshape(-1), db2] if fov != 5 else []) + [dw1.reshape(-1), db1]
    return out, np.concatenate(flat), gz.T @ v, gz.sum(axis=0)


def guarded(shape, dtype=torch.float32, fill=0.0, device='cpu', offset=0):
    """A contiguous tensor of `shape` filled with `fill` that is a view into a larger buffer with MARGIN sentinel elements before
    and after it (and `offset` more before it: offset=1 gives a float32 view that is 4-byte but not 8-byte aligned)
    -> (view, check); check() asserts that no margin byte has changed."""
    n = int(np.prod(shape))
    buf = torch.empty(MARGIN + offset + n + MARGIN, dtype=dtype, device=device)
    sentinel = float('nan') if dtype.is_floating_point else 113
    buf.fill_(sentinel)
    view = buf[MARGIN + offset:MARGIN + offset + n]
    view.fill_(fill)
    before, after = buf[:MARGIN + offset], buf[MARGIN + offset + n:]
    want = (before.clone().view(torch.uint8), after.clone().view(torch.uint8))

    def check():
        assert torch.equal(before.view(torch.uint8), want[0]), 'written before the start of a buffer'
        assert torch.equal(after.view(torch.uint8), want[1]), 'written past the end of a buffer'
    return view.view(shape), check


def mlp_case(rows, n_actions, seed):
    """Integer inputs of crnn_mlp_backward alone: direction bytes in [-2, 2], a one-hot, forward-output columns in [-1, 2] (a
    third of them <= 0, a quarter exactly 0) and a gradient in {-1, 0, 1}; every sum is an integer of at most 2 rows."""
    g = torch.Generator().manual_seed(seed)
    c = types.SimpleNamespace(rows=rows, n_actions=n_actions)
    c.dirs = _ints(g, (rows, 2), -2, 2).to(torch.int8)
    c.onehot = torch.zeros((rows, n_actions), dtype=torch.int8)
    if n_actions > 0:
        c.onehot[torch.arange(rows), _ints(g, (rows,), 0, n_actions - 1)] = 1
    c.x = _ints(g, (rows, 10), -1, 2).float()
    c.g = _ints(g, (rows, 10), -1, 1).float()
    v = torch.cat([c.dirs, c.onehot], dim=1).double()
    gz = c.g.double() * (c.x > 0)
    c.dw, c.db = gz.t() @ v, gz.sum(0)
    c.bound = 2.0 * rows
    return c
