"""Every solution of a TunableOp results file against a float64 product (default: the shipped
marl_dmfb_amd/tuning/gemm_gfx950.csv, which pins the rocBLAS / hipBLASLt solution of the GEMMs of the rollout and the learn).

For each entry (op, key, solution) the operands are rebuilt from the key and the fp32 torch call the project makes for that op is
issued with the file loaded read-only by `common/gemm_tuning.enable()`, so the listed solution runs:

  GemmTunableOp_float_TN                F.linear(x, W)      x @ W^T      GRU input / hidden projections, heads
  GemmAndBiasTunableOp_float_TN         F.linear(x, W, b)   x @ W^T + b  heads, mlp1, conv GEMMs (bias epilogue)
  GemmTunableOp_float_NN                g @ W                            their data gradients
  GemmTunableOp_float_NT                g.t() @ x                        unsplit weight gradients
  GemmStridedBatchedTunableOp_float_NT  bmm(g_s^T, x_s)                  split-K weight gradients (`_wgrad_splitk`)

Keys are column-major BLAS terms, as TunableOp prints them: `tn_<m>_<n>_<k>[_B_<batch>]_ld_<lda>_<ldb>_<ldc>`.  A leading
dimension wider than its operand is a column slice of a wider row-major tensor (mlp1 reads columns 1083..1093 of the 1094-wide
MEDA input rows); it is rebuilt as the LAST columns of a NaN-filled tensor, so the pointer offset is the project's and a read
outside the view poisons the result.

Two passes per entry:
  exact      integer operands and bias, |v| <= 3: every partial sum is an integer below 2^24 for K <= 92 160 (9 K + 3 < 2^24), so
             the fp32 result must EQUAL the float64 product; any tile-tail, ld, batch-stride or split error shows.
  precision  full-mantissa normal operands, every row scaled by 2^U(-8, 8):
               element-wise  |C - C64| <= 1.01 K' 2^-24 (|A||B| + |b|)   (K' = K, +1 with a bias: the rigorous fp32 dot-product
                                                                          bound for any summation order; never fails on a correct kernel)
               aggregate     ||C - C64||_F / ||C64||_F <= 8 2^-24 sqrt(K) (inputs rounded to tf32 land near 3e-4, above it for
                                                                          every K in the file: tests/test_gemm_solution_checks.py)
             and the result must be finite.
C64 is formed on the GPU in float64, in pieces that keep the float64 temporaries near 256 MB.  A CPU spot check (~512 elements,
the first and last row and column of the first and last batch among them, float64 from CPU copies of the rows and columns
involved) holds both passes to the same comparison without going through rocBLAS.

Reached: the child runs with PYTORCH_TUNABLEOP_RECORD_UNTUNED=1, so TunableOp writes every GEMM it does not find in the file to
an untuned record.  After the child has exited, no fp32 key it issued may be in that record (each call was served from the
file), and a few control calls with shapes that are NOT in the file must be there under the keys predicted for them (the record
is live, and the keys above are what TunableOp sees).  The float64 reference GEMMs are recorded too and ignored.

    python tests/gemm_solution_worker.py [RESULTS.csv] [--callsite]    exit 0 only when every entry passed and was reached

TunableOp reads its environment once per process, so the check always runs in a fresh child process (`run`)."""
import argparse
import collections
import json
import math
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIPPED = os.path.join(ROOT, 'marl_dmfb_amd', 'tuning', 'gemm_gfx950.csv')
TUNED = 'tuned (shipped choices)'

U = 2.0 ** -24           # unit roundoff of fp32
ELEM_SLACK = 1.01        # gamma_K = K u / (1 - K u) <= 1.0056 K u for K <= 92 160
AGG_FACTOR = 8.0
EXACT_MAX = 3            # |v| of the exact pass's operands and bias
CHUNK_DOUBLES = 1 << 25  # float64 elements per reference piece (256 MB)
SPOT_ELEMS = 512

KINDS = {'GemmTunableOp_float_TN': 'linear', 'GemmAndBiasTunableOp_float_TN': 'linear_bias', 'GemmTunableOp_float_NN': 'dgrad',
         'GemmTunableOp_float_NT': 'wgrad', 'GemmStridedBatchedTunableOp_float_NT': 'wgrad_bmm'}
_KEY = re.compile(r'^(tn|nn|nt)_(\d+)_(\d+)_(\d+)(?:_B_(\d+))?_ld_(\d+)_(\d+)_(\d+)$')

Entry = collections.namedtuple('Entry', 'op key solution kind m n k batch lda ldb ldc')


def operand_shapes(e):
    """((rows, width) of the A operand, (rows, width) of the B operand) as row-major torch tensors with row stride lda / ldb.
    TN: A = W [m, k], B = x [n, k];  NN: A = W [k, m], B = g [n, k];  NT: A = x [batch k, m], B = g [batch k, n]."""
    if e.kind in ('linear', 'linear_bias'):
        return (e.m, e.k), (e.n, e.k)
    if e.kind == 'dgrad':
        return (e.k, e.m), (e.n, e.k)
    return (e.batch * e.k, e.m), (e.batch * e.k, e.n)


def parse_entry(op, key, solution='Default'):
    """One results line -> Entry; ValueError for an op or key this checker does not know (never skipped silently)."""
    kind = KINDS.get(op)
    if kind is None:
        raise ValueError('unknown TunableOp op %r' % op)
    mt = _KEY.match(key)
    if mt is None:
        raise ValueError('unparsable key %r of %s' % (key, op))
    trans, m, n, k, batch, lda, ldb, ldc = mt.groups()
    if trans != op[-2:].lower():
        raise ValueError('key %r does not match the layout of %s' % (key, op))
    if (batch is None) == (kind == 'wgrad_bmm'):
        raise ValueError('key %r: a batch count belongs to the strided-batched op, and only there (%s)' % (key, op))
    e = Entry(op, key, solution, kind, int(m), int(n), int(k), int(batch or 1), int(lda), int(ldb), int(ldc))
    if min(e.m, e.n, e.k, e.batch) < 1:
        raise ValueError('key %r: empty GEMM' % key)
    (_, wa), (_, wb) = operand_shapes(e)
    if e.lda < wa or e.ldb < wb or e.ldc != e.m:
        raise ValueError('key %r: leading dimensions do not fit the operands, or C is not dense' % key)
    if e.batch > 1 and (e.lda != wa or e.ldb != wb):
        raise ValueError('key %r: a strided batch of sub-matrix views is not a call the project makes' % key)
    return e


def read_entries(path=SHIPPED):
    """Entries of a results file in file order (validator lines skipped; anything else unrecognised is an error)."""
    out = []
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            line = line.strip()
            if not line or line.startswith('Validator,'):
                continue
            parts = line.split(',')
            if len(parts) < 3:
                raise ValueError('%s:%d: not an op,key,solution line: %r' % (path, no, line))
            out.append(parse_entry(parts[0], parts[1], parts[2]))
    return out


def format_key(e):
    b = '_B_%d' % e.batch if e.kind == 'wgrad_bmm' else ''
    return '%s_%d_%d_%d%s_ld_%d_%d_%d' % (e.op[-2:].lower(), e.m, e.n, e.k, b, e.lda, e.ldb, e.ldc)


def k_eff(e):
    return e.k + (1 if e.kind == 'linear_bias' else 0)


def elem_coef(e):
    return ELEM_SLACK * k_eff(e) * U


def agg_bound(k):
    return AGG_FACTOR * U * math.sqrt(k)


# ---------------------------------------------------------------------------------------------------------------------- operands

def fill_(t, mode, gen):
    """In place, on a 2-D (possibly column-sliced) view: integers in [-3, 3] ('exact') or normal values with every row scaled
    by 2^U(-8, 8) ('precision')."""
    import torch
    if mode == 'exact':
        return t.random_(-EXACT_MAX, EXACT_MAX + 1, generator=gen)
    t.normal_(generator=gen)
    scale = torch.empty(t.shape[0], dtype=t.dtype, device=t.device).uniform_(-8.0, 8.0, generator=gen).exp2_()
    return t.mul_(scale[:, None])


def _matrix(rows, width, ld, mode, gen, device):
    """[rows, width] float32 with row stride ld: the last `width` columns of a NaN-filled [rows, ld] tensor when ld > width."""
    import torch
    if ld == width:
        return fill_(torch.empty((rows, width), dtype=torch.float32, device=device), mode, gen)
    buf = torch.full((rows, ld), float('nan'), dtype=torch.float32, device=device)
    return fill_(buf[:, ld - width:], mode, gen)


def build(e, mode, gen, device):
    """The operands of one entry in the layout of the project's call: {'a', 'b', 'bias'} (see operand_shapes)."""
    import torch
    (ra, wa), (rb, wb) = operand_shapes(e)
    ops = {'a': _matrix(ra, wa, e.lda, mode, gen, device), 'b': _matrix(rb, wb, e.ldb, mode, gen, device), 'bias': None}
    if e.kind == 'linear_bias':
        bias = torch.empty(e.m, dtype=torch.float32, device=device)
        ops['bias'] = bias.random_(-EXACT_MAX, EXACT_MAX + 1, generator=gen) if mode == 'exact' else bias.normal_(generator=gen)
    return ops


def call(e, ops):
    """The torch call the project makes for this op: the GEMM under test."""
    import torch
    import torch.nn.functional as F
    a, b = ops['a'], ops['b']
    if e.kind == 'linear':
        return F.linear(b, a)
    if e.kind == 'linear_bias':
        return F.linear(b, a, ops['bias'])
    if e.kind == 'dgrad':
        return b @ a
    if e.kind == 'wgrad':
        return b.t() @ a
    return torch.bmm(b.view(e.batch, e.k, e.n).transpose(1, 2), a.view(e.batch, e.k, e.m))


def as_batched(e, ops):
    """(L [B, R, K], Rt [B, K, C]) views with out[b] = L[b] @ Rt[b] (+ bias): the one form the references use."""
    a, b = ops['a'], ops['b']
    if e.kind in ('linear', 'linear_bias'):
        return b[None], a.t()[None]
    if e.kind == 'dgrad':
        return b[None], a[None]
    if e.kind == 'wgrad':
        return b.t()[None], a[None]
    return b.view(e.batch, e.k, e.n).transpose(1, 2), a.view(e.batch, e.k, e.m)


# ------------------------------------------------------------------------------------------------------------------- comparison

def _pieces(B, R, K, C, budget=CHUNK_DOUBLES):
    """(batch slice, row slice) pieces of the [B, R, C] output whose float64 operands and temporaries stay near `budget`."""
    per_row = K + 5 * C
    per_batch = R * per_row + K * C
    if per_batch <= budget:
        nb = max(1, budget // per_batch)
        for b0 in range(0, B, nb):
            yield slice(b0, min(B, b0 + nb)), slice(0, R)
        return
    nr = max(1, (budget - K * C) // per_row)
    for b in range(B):
        for r0 in range(0, R, nr):
            yield slice(b, b + 1), slice(r0, min(R, r0 + nr))


def compare(e, mode, L, Rt, out, bias, budget=CHUNK_DOUBLES):
    """One pass against the float64 product, formed on the device of the operands (in `_pieces`).
    exact -> {'mismatches'}; precision -> {'elem_ratio', 'rel_fro', 'finite'}."""
    import torch
    B, R, K = L.shape
    C = Rt.shape[2]
    out = out.view(B, R, C)
    b64 = bias.double() if bias is not None else None
    coef = elem_coef(e)
    mism, ratio, err2, ref2, finite = 0, 0.0, 0.0, 0.0, True
    for bs, rs in _pieces(B, R, K, C, budget):
        l, r = L[bs, rs].double(), Rt[bs].double()
        ref = torch.matmul(l, r)
        if b64 is not None:
            ref += b64
        got = out[bs, rs].double()
        if mode == 'exact':
            mism += int((got != ref).sum())
        else:
            finite = finite and bool(torch.isfinite(got).all())
            mag = torch.matmul(l.abs_(), r.abs_())
            if b64 is not None:
                mag += b64.abs()
            d = (got - ref).abs_()
            ratio = max(ratio, float((d / mag.mul_(coef).add_(1e-300)).max()))
            err2 += float(d.square_().sum())
            ref2 += float(ref.square_().sum())
            del mag, d
        del l, r, ref, got
    if mode == 'exact':
        return {'mismatches': mism}
    return {'elem_ratio': ratio, 'rel_fro': math.sqrt(err2 / max(ref2, 1e-300)), 'finite': finite}


def _spot_index(n, want, gen):
    """Sorted indices into range(n): 0, n - 1 and random others, `want` in all (or n)."""
    import torch
    idx = {0, n - 1}
    want = min(want, n)
    while len(idx) < want:
        idx.update(torch.randint(0, n, (want,), generator=gen).tolist()[:want - len(idx)])
    return sorted(idx)


def spot_check(e, mode, L, Rt, out, bias, seed):
    """~512 output elements recomputed on the CPU in float64 from CPU copies of their rows and columns: True when they are
    finite and the pass's comparison (equality / element-wise bound) holds for every one."""
    import numpy as np
    import torch
    B, R, K = L.shape
    C = Rt.shape[2]
    out = out.view(B, R, C)
    gen = torch.Generator().manual_seed(seed)
    bi = _spot_index(B, 3, gen)
    ri = _spot_index(R, 16, gen)
    ci = _spot_index(C, -(-SPOT_ELEMS // (len(bi) * len(ri))), gen)
    bt, rt, ct = (torch.tensor(v, device=L.device) for v in (bi, ri, ci))
    # one gather each, so that no whole batch of a multi-GB operand or result is copied on the way
    lsel = L[bt[:, None], rt[None, :]].cpu().double().numpy()                          # [nb, nr, K]
    rsel = Rt[bt[:, None], :, ct[None, :]].transpose(1, 2).cpu().double().numpy()      # [nb, K, nc]
    got = out[bt[:, None, None], rt[None, :, None], ct[None, None, :]].cpu().double().numpy()
    ref = np.matmul(lsel, rsel)
    mag = np.matmul(np.abs(lsel), np.abs(rsel))
    if bias is not None:
        bsel = bias.index_select(0, ct).cpu().double().numpy()
        ref += bsel
        mag += np.abs(bsel)
    if not np.isfinite(got).all():
        return False
    if mode == 'exact':
        return bool((got == ref).all())
    return bool((np.abs(got - ref) <= elem_coef(e) * mag).all())


def check_entry(e, device, seed):
    """Both passes of one entry -> its JSON-able result; the operands are freed before it returns."""
    import torch
    t0 = time.time()
    res = {'op': e.op, 'key': e.key, 'solution': e.solution, 'kind': e.kind}
    spot = True
    for p, mode in enumerate(('exact', 'precision')):
        gen = torch.Generator(device=device).manual_seed(seed * 2 + p)
        ops = build(e, mode, gen, device)
        out = call(e, ops)
        L, Rt = as_batched(e, ops)
        res.update(compare(e, mode, L, Rt, out, ops['bias']))
        spot = spot_check(e, mode, L, Rt, out, ops['bias'], seed * 2 + p) and spot
        del ops, out, L, Rt
    res['exact_ok'] = res['mismatches'] == 0
    res['agg_ratio'] = res['rel_fro'] / agg_bound(k_eff(e))
    res['spot_ok'] = spot
    res['ok'] = bool(res['exact_ok'] and res['finite'] and res['elem_ratio'] <= 1.0 and res['agg_ratio'] <= 1.0 and spot)
    res['seconds'] = round(time.time() - t0, 3)
    return res


# ------------------------------------------------------------------------------------------------------- controls and call site

_CONTROLS = [('GemmTunableOp_float_TN', 'tn_24_100_40_ld_40_40_24'),
             ('GemmAndBiasTunableOp_float_TN', 'tn_10_100_11_ld_11_1094_10'),       # mlp1's sub-matrix view
             ('GemmTunableOp_float_NN', 'nn_40_100_24_ld_40_24_40'),
             ('GemmTunableOp_float_NT', 'nt_11_10_100_ld_1094_10_11'),              # its weight gradient
             ('GemmStridedBatchedTunableOp_float_NT', 'nt_40_24_100_B_4_ld_40_24_40')]


def control_entries(entries):
    """One small call per op kind (mlp1's two sub-matrix forms among them) whose key is NOT in the file: each must land in the
    untuned record under exactly this key."""
    have = {(x.op, x.key) for x in entries}
    clash = [c for c in _CONTROLS if c in have]
    if clash:
        raise ValueError('control keys are in the results file: %s' % clash)
    return [parse_entry(op, key) for op, key in _CONTROLS]


def splitk_chunks(M):
    """S of `_wgrad_splitk` (network/base_net.py): the largest of 64, 32, .., 2 that divides M with M / S >= 512, else 1."""
    return next((s for s in (64, 32, 16, 8, 4, 2) if M % s == 0 and M // s >= 512), 1)


CALLSITE = {'input projection': dict(rows=81920, real=610, cols=640, out=384, bias=False),   # fov 9, od 24: W_ih zero-padded
            'head': dict(rows=81920, real=128, cols=128, out=5, bias=True)}                # fc1 of DMFB, 5 actions


def callsite_keys(rows, cols, out, bias, **_):
    """(op, key) of the three GEMMs `_LinearSplitK` issues forward and backward at this shape."""
    S = splitk_chunks(rows)
    keys = [('GemmAndBiasTunableOp_float_TN' if bias else 'GemmTunableOp_float_TN',
             'tn_%d_%d_%d_ld_%d_%d_%d' % (out, rows, cols, cols, cols, out)),
            ('GemmTunableOp_float_NN', 'nn_%d_%d_%d_ld_%d_%d_%d' % (cols, rows, out, cols, out, cols))]
    if S == 1:
        keys.append(('GemmTunableOp_float_NT', 'nt_%d_%d_%d_ld_%d_%d_%d' % (cols, out, rows, cols, out, cols)))
    else:
        keys.append(('GemmStridedBatchedTunableOp_float_NT', 'nt_%d_%d_%d_B_%d_ld_%d_%d_%d' % (cols, out, rows // S, S, cols, out, cols)))
    return keys


def check_callsite(device, seed=5):
    """`_LinearSplitK` forward and backward (the project's glue: split-K weight gradient, two-stage bias gradient, zero-padded
    W_ih) in fp32 through the shipped solutions, against float64 autograd -> relative L2 per tensor."""
    import torch
    import torch.nn.functional as F
    from marl_dmfb_amd.network.base_net import _LinearSplitK
    res = {}
    gen = torch.Generator(device=device).manual_seed(seed)
    for name, c in CALLSITE.items():
        x = torch.randn((c['rows'], c['cols']), generator=gen, device=device)
        x[:, c['real']:] = 0.0                                     # the front end writes its rows zero-padded
        w = torch.randn((c['out'], c['real']), generator=gen, device=device) * 0.05
        b = torch.randn(c['out'], generator=gen, device=device) if c['bias'] else None
        gy = torch.randn((c['rows'], c['out']), generator=gen, device=device)
        got, want = [], []
        for dt, dst in ((torch.float32, got), (torch.float64, want)):
            leaves = [t.detach().to(dt, copy=True).requires_grad_(True) for t in (x, w) + ((b,) if b is not None else ())]
            xs, ws, bs = leaves[0], leaves[1], (leaves[2] if b is not None else None)
            wp = F.pad(ws, (0, c['cols'] - c['real']))
            if dt == torch.float32:
                y = _LinearSplitK.apply(xs, wp, bs)
            else:
                y = xs @ wp.t() + (bs if bs is not None else 0.0)
            grads = torch.autograd.grad(y, leaves, gy.to(dt))
            dst.extend(t.detach() for t in (y,) + tuple(grads))
            del leaves, xs, ws, bs, wp, y, grads
        rel = {t: float((g.double() - r).norm() / (r.norm() + 1e-300)) for t, g, r in zip(('y', 'gx', 'gw', 'gb'), got, want)}
        res[name] = {'rel_l2': rel, 'keys': [list(k) for k in callsite_keys(**c)]}
        del x, w, b, gy, got, want
        torch.cuda.empty_cache()
    return res


# ---------------------------------------------------------------------------------------------------------------------- child

def _emit(fh, rec):
    fh.write(json.dumps(rec) + '\n')
    fh.flush()


def _device_error(ex):
    msg = str(ex)
    return any(s in msg for s in ('HIP error', 'hipError', 'CUDA error', 'illegal memory', 'device-side'))


def child(results, out_path, with_callsite):
    sys.path.insert(0, ROOT)
    import torch
    from marl_dmfb_amd.common import gemm_tuning
    gemm_tuning.RESULTS = results                # the file enable() loads: the shipped one unless another is being checked
    gemm_tuning.enable()
    dev = 'cuda:0'
    with open(out_path, 'w') as fh:
        _emit(fh, {'mode': gemm_tuning.mode()})
        if gemm_tuning.mode() != TUNED:
            return 0
        entries = read_entries(results)
        t0 = time.time()
        for i, e in enumerate(entries):
            try:
                rec = check_entry(e, dev, seed=1000 + i)
            except RuntimeError as ex:           # e.g. a solution name this build does not register: a failed entry
                if _device_error(ex):
                    raise                        # a device fault ends the run: nothing more is started on the GPU
                rec = {'op': e.op, 'key': e.key, 'solution': e.solution, 'kind': e.kind, 'ok': False, 'error': str(ex)[:300]}
            torch.cuda.empty_cache()
            _emit(fh, rec)
            print('%3d/%d %-38s %-38s %s  %.2f s' % (i + 1, len(entries), e.op, e.key, 'ok' if rec['ok'] else 'FAIL',
                                                     rec.get('seconds', 0.0)), file=sys.stderr, flush=True)
        ctl = control_entries(entries)
        for i, e in enumerate(ctl):
            call(e, build(e, 'exact', torch.Generator(device=dev).manual_seed(7 + i), dev))
        torch.cuda.synchronize()
        _emit(fh, {'controls': [[e.op, e.key] for e in ctl], 'entries_seconds': round(time.time() - t0, 2)})
        if with_callsite:
            _emit(fh, {'callsite': check_callsite(dev)})
        torch.cuda.synchronize()
        _emit(fh, {'peak_bytes': torch.cuda.max_memory_allocated(), 'done': True})
    return 0


# --------------------------------------------------------------------------------------------------------------------- parent

def read_untuned(d):
    """{(op, key)} of the fp32 GEMMs TunableOp did not find in the file (the float64 reference GEMMs are left out)."""
    keys = set()
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name)) as fh:
            for line in fh:
                parts = line.strip().split(',')
                if len(parts) >= 2 and '_float_' in parts[0]:
                    keys.add((parts[0], parts[1]))
    return keys


def run(results=SHIPPED, timeout=600, with_callsite=False, stream_stderr=False):
    """The check in a fresh child process -> report dict.  'failed' holds the reason and the tail of the child's stderr when
    the child did not finish normally (crash, signal, time limit); nothing is started again."""
    results = os.path.abspath(results)
    work = tempfile.mkdtemp(prefix='gemm_solutions_')
    untuned = os.path.join(work, 'untuned')
    os.makedirs(untuned)
    out_path = os.path.join(work, 'records.jsonl')
    # the child's environment only: the record of untuned GEMMs on, and no inherited TunableOp or tuning switches
    env = {k: v for k, v in os.environ.items() if not k.startswith(('PYTORCH_TUNABLEOP_', 'MARL_DMFB_GEMM_'))}
    env.update(PYTORCH_TUNABLEOP_RECORD_UNTUNED='1', PYTORCH_TUNABLEOP_UNTUNED_FILENAME=os.path.join(untuned, 'untuned.csv'))
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--out', out_path, results] + (['--callsite'] if with_callsite else [])
    rep = {'results': results, 'failed': None}
    t0 = time.time()
    try:
        p = subprocess.run(cmd, env=env, cwd=ROOT, timeout=timeout, stdout=subprocess.PIPE,
                           stderr=None if stream_stderr else subprocess.PIPE, text=True)
        if p.returncode != 0:
            rep['failed'] = 'child exited with status %d\n%s\n%s' % (p.returncode, p.stdout[-2000:], (p.stderr or '')[-4000:])
    except subprocess.TimeoutExpired as ex:
        err = ex.stderr.decode(errors='replace') if isinstance(ex.stderr, bytes) else (ex.stderr or '')
        rep['failed'] = 'child killed after %d s\n%s' % (timeout, err[-4000:])
    rep['seconds'] = round(time.time() - t0, 1)
    recs = []
    if os.path.exists(out_path):
        with open(out_path) as fh:
            recs = [json.loads(line) for line in fh if line.strip()]
    rep['mode'] = next((r['mode'] for r in recs if 'mode' in r), None)
    rep['entries'] = [r for r in recs if 'key' in r]
    for r in recs:
        rep.update((k, r[k]) for k in ('controls', 'entries_seconds', 'callsite', 'peak_bytes', 'done') if k in r)
    if rep['failed'] is None and rep['mode'] == TUNED and not rep.get('done'):
        rep['failed'] = 'child exited without finishing its records'
    rep['untuned'] = sorted(read_untuned(untuned))
    shutil.rmtree(work, ignore_errors=True)
    return rep


def verdict(rep, expected):
    """Problems of a finished report (empty: every entry of `expected` was checked, passed and was served from the file)."""
    probs = []
    got = {(r['op'], r['key']): r for r in rep['entries']}
    missing = [(e.op, e.key) for e in expected if (e.op, e.key) not in got]
    if missing:
        probs.append('%d entries not checked: %s' % (len(missing), missing[:10]))
    for r in rep['entries']:
        if r['ok']:
            continue
        if 'error' in r:
            probs.append('FAILED %s %s (%s): %s' % (r['op'], r['key'], r['solution'], r['error']))
        else:
            probs.append('FAILED %s %s (%s): exact mismatches %d, element-wise ratio %.3g, rel Frobenius %.3g (%.3g of the bound), '
                         'finite %s, spot check %s' % (r['op'], r['key'], r['solution'], r['mismatches'], r['elem_ratio'],
                                                      r['rel_fro'], r['agg_ratio'], r['finite'], r['spot_ok']))
    untuned = {tuple(k) for k in rep['untuned']}
    unreached = sorted(k for k in got if k in untuned)
    if unreached:
        probs.append('%d entries NOT served from the file (in the untuned record): %s' % (len(unreached), unreached[:10]))
    controls = {tuple(k) for k in rep.get('controls', [])}
    if controls - untuned:
        probs.append('control calls missing from the untuned record (record not live, or keys not as predicted): %s'
                     % sorted(controls - untuned))
    stray = sorted(untuned - controls - set(got))
    if stray:
        probs.append('fp32 GEMMs issued with keys that are not in the file: %s' % stray[:10])
    return probs


def summary(rep):
    """Lines: entries checked / passed / reached, worst element-wise ratio and relative Frobenius error per op, time, memory."""
    untuned = {tuple(k) for k in rep['untuned']}
    es = rep['entries']
    lines = ['%d entries checked, %d passed, %d served from the file; child %.1f s (entries %.1f s), peak device memory %.2f GB'
             % (len(es), sum(r['ok'] for r in es), sum((r['op'], r['key']) not in untuned for r in es), rep['seconds'],
                rep.get('entries_seconds', float('nan')), rep.get('peak_bytes', 0) / 1e9)]
    by = collections.OrderedDict()
    for r in es:
        if 'error' not in r:
            by.setdefault(r['op'], []).append(r)
    for op, rs in by.items():
        w_e = max(rs, key=lambda r: r['elem_ratio'])
        w_f = max(rs, key=lambda r: r['agg_ratio'])
        lines.append('  %-37s %3d  worst element-wise ratio %.3f (%s), worst rel Frobenius %.2e = %.3f of its bound (%s)'
                     % (op, len(rs), w_e['elem_ratio'], w_e['key'], w_f['rel_fro'], w_f['agg_ratio'], w_f['key']))
    for name, c in rep.get('callsite', {}).items():
        lines.append('  _LinearSplitK %s: relative L2 %s' % (name, ', '.join('%s %.2e' % kv for kv in c['rel_l2'].items())))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description='Every solution of a TunableOp results file against a float64 product.')
    ap.add_argument('results', nargs='?', default=SHIPPED)
    ap.add_argument('--callsite', action='store_true', help='also _LinearSplitK at two shipped shapes against float64 autograd')
    ap.add_argument('--timeout', type=int, default=840, help='seconds for the child process')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--out', help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.child:
        return child(os.path.abspath(a.results), a.out, a.callsite)
    expected = read_entries(a.results)
    rep = run(a.results, timeout=a.timeout, with_callsite=a.callsite, stream_stderr=True)
    if rep['failed']:
        print(rep['failed'], file=sys.stderr)
        return 1
    if rep['mode'] != TUNED:
        print('nothing checked: GEMM solutions are "%s" with %s' % (rep['mode'], a.results), file=sys.stderr)
        return 2
    print('\n'.join(summary(rep)))
    probs = verdict(rep, expected)
    for p in probs:
        print(p, file=sys.stderr)
    return 1 if probs else 0


if __name__ == '__main__':
    sys.exit(main())
