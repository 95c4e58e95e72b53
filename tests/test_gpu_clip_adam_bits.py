"""vdn_clip_adam_step (include/vdn_ops.h: k_sqnorm_partials + k_clip_adam) must give, bit for bit, what the library gave BEFORE a
thread's loads were moved ahead of its arithmetic: parameters, both moments, the gradients as clip_grad_norm_ leaves them and the
total norm, after three steps on fresh gradients.  The tolerance tests (tests/test_gpu_td_fused.py,
tests/test_gpu_packed_learn_kernels.py) cannot see a reordered sum; the weights of every later learn follow these bits.

tests/golden/clip_adam_bits.npz holds only recorded outputs (tools/record_clip_adam_fixture.py, run on an MI355X with the library of
the commit before the change); the inputs are regenerated here, on the host, from the seeds below.

One list of four tensors of 1, 255, 257 and 70 000 elements (70 513 in all: 128 norm workgroups of 551 elements, three per thread
with a ragged third; 69 Adam workgroups of 1022, four per thread; the small tensors share workgroups, so a thread's walk crosses
tensor boundaries).  Cases: with and without grad_div, gradients whose norm is far above max_norm (the clip rescales them) and far
below (coefficient 1: without grad_div the gradients are not rewritten).  The three small tensors are recorded whole; of the large
one every 97th element and a SHA-256 of all its bits."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

DEV = 'cuda'
NUMELS = (1, 255, 257, 70000)
SMALL = sum(NUMELS[:3])
STEPS = 3
MAX_NORM, LR, BETA1, BETA2, EPS = 10.0, 5e-4, 0.9, 0.999, 1e-8
GRAD_DIV = 7.0
CASES = [(div, clip) for div in (False, True) for clip in (True, False)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'clip_adam_bits.npz')
QUANTITIES = ('p', 'm', 'v', 'g')


def case_key(div, clip):
    return '%s_%s' % ('div' if div else 'nodiv', 'clip' if clip else 'noclip')


def inputs(div, clip):
    """Host inputs of a case: the parameters and STEPS gradient sets.  Norm of a set: about 265 (x 1/7 with grad_div) when the clip is
    to trigger, a thousandth of that when not."""
    g = np.random.default_rng(930000 + 2 * div + clip)
    total = sum(NUMELS)
    p = g.standard_normal(total, dtype=np.float32) * np.float32(0.1)
    scale = np.float32(1.0 if clip else 1e-3)
    grads = [g.standard_normal(total, dtype=np.float32) * scale for _ in range(STEPS)]
    return p, grads


def run_case(div, clip):
    """-> {'p', 'm', 'v', 'g': float32[70513] after STEPS steps (g: of the last step, as left in memory), 'norm': float32[STEPS]}."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_ops()
    p_h, grads_h = inputs(div, clip)
    offs = np.concatenate([[0], np.cumsum(NUMELS)])
    split = lambda a: [torch.from_numpy(a[offs[k]:offs[k + 1]].copy()).to(DEV) for k in range(len(NUMELS))]
    p = split(p_h)
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    partials = torch.full((128,), float('nan'), device=DEV)
    norm = torch.full((1,), float('nan'), device=DEV)
    d = torch.full((1,), GRAD_DIV, device=DEV) if div else None
    n = len(NUMELS)
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    norms = []
    for step in range(1, STEPS + 1):
        g = split(grads_h[step - 1])
        rc = lib.vdn_clip_adam_step(n, arr(p), arr(g), arr(m), arr(v), (C.c_int64 * n)(*NUMELS), MAX_NORM, LR, BETA1, BETA2, EPS,
                                    1.0 - BETA1 ** step, 1.0 - BETA2 ** step, C.c_void_p(partials.data_ptr()), C.c_void_p(norm.data_ptr()),
                                    None if d is None else C.c_void_p(d.data_ptr()), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        norms.append(float(norm[0]))
    cat = lambda ts: torch.cat(ts).cpu().numpy()
    return {'p': cat(p), 'm': cat(m), 'v': cat(v), 'g': cat(g), 'norm': np.asarray(norms, dtype=np.float32)}


def pack(res):
    """What the record keeps of a case: {quantity + '_small', '_every97', '_sha256'} and 'norm'."""
    out = {'norm': res['norm']}
    for q in QUANTITIES:
        a = np.ascontiguousarray(res[q])
        out[q + '_small'] = a[:SMALL]
        out[q + '_every97'] = a[SMALL::97]
        out[q + '_sha256'] = np.frombuffer(hashlib.sha256(a[SMALL:].tobytes()).digest(), dtype=np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _run_packed(div, clip):
    return pack(run_case(div, clip))


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    gb, wb = got.view(np.uint8 if got.dtype == np.uint8 else np.uint32), want.view(np.uint8 if want.dtype == np.uint8 else np.uint32)
    bad = np.argwhere(gb != wb)
    print('%s: %d of %d elements with other bits' % (what, len(bad), got.size))
    if len(bad):
        i = int(bad[0][0])
        raise AssertionError('%s: %d of %d elements differ from the record, first at %d: got %r, recorded %r' % (what, len(bad), got.size, i, got[i], want[i]))


def test_the_record_holds_every_case():
    g = _golden()
    names = ['norm'] + [q + s for q in QUANTITIES for s in ('_small', '_every97', '_sha256')]
    assert sorted(g) == sorted('%s__%s' % (case_key(*c), nm) for c in CASES for nm in names)
    for c in CASES:
        k = case_key(*c)
        assert g[k + '__norm'].shape == (STEPS,) and np.isfinite(g[k + '__norm']).all()
        for q in QUANTITIES:
            assert g['%s__%s_small' % (k, q)].shape == (SMALL,) and g['%s__%s_sha256' % (k, q)].shape == (32,)
            assert np.isfinite(g['%s__%s_small' % (k, q)]).all() and np.isfinite(g['%s__%s_every97' % (k, q)]).all()
    # the cases are what their names say: the clip triggers (norm above max_norm) or does not
    for div, clip in CASES:
        assert bool((g[case_key(div, clip) + '__norm'] > MAX_NORM).all()) == clip
    # without grad_div and without a clip the gradients stay as they were given
    _, grads = inputs(False, False)
    assert np.array_equal(g['nodiv_noclip__g_small'].view(np.uint32), grads[-1][:SMALL].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize('div,clip', CASES, ids=[case_key(*c) for c in CASES])
def test_clip_adam_bits_of_the_build_before(div, clip):
    got, g, k = _run_packed(div, clip), _golden(), case_key(div, clip)
    for nm in sorted(got):
        _same_bits(got[nm], g['%s__%s' % (k, nm)], '%s %s' % (k, nm))
