"""CPU side of the check of the shipped GEMM solutions (tests/gemm_solution_worker.py; on the GPU: tests/test_gpu_gemm_solutions.py)
and of the project's split-K glue around those GEMMs (network/base_net.py: _wgrad_splitk, _colsum, _LinearSplitK):
* the worker reads every line of the shipped results file as one of the five calls the project makes, and refuses anything else;
* its bounds have power, at the smallest and the largest K of the file: sequential fp32 accumulation stays inside both, inputs
  rounded to tf32 or bf16 break the aggregate one, and a dropped K chunk or a shifted row breaks the exact pass;
* its whole per-entry check passes a correct product and fails a corrupted one (on the CPU, at small keys of every kind);
* the split-K glue against float64 at the boundaries of its split choices, and S is the documented choice."""
import numpy as np
import pytest
import torch

import gemm_solution_worker as W
from marl_dmfb_amd.network import base_net

GRAD_TOL = 5e-6   # relative L2 per tensor against float64 autograd (tests/test_gpu_crnn_ops.py)
K_RANGE = (5, 92160)


def _round_mantissa(a, bits):
    """float32 array rounded to nearest-even with `bits` explicit mantissa bits (10: tf32, 7: bf16)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    drop = 23 - bits
    u = ((u + ((1 << (drop - 1)) - 1) + ((u >> drop) & 1)) >> drop) << drop
    return u.astype(np.uint32).view(np.float32)


def _seq_fp32(A, B):
    """A @ B with every product rounded to fp32 and summed one after the other in fp32 (numpy's accumulate is sequential)."""
    A, B = np.asarray(A, dtype=np.float32), np.asarray(B, dtype=np.float32)
    return np.ascontiguousarray(np.cumsum(A[:, :, None] * B[None, :, :], axis=1, dtype=np.float32)[:, -1, :])


def _nn(M, K, N):
    """Entry of out [M, N] = g [M, K] @ W [K, N]: L = g, Rt = W in the worker's terms."""
    return W.parse_entry('GemmTunableOp_float_NN', 'nn_%d_%d_%d_ld_%d_%d_%d' % (N, M, K, N, K, N))


def _operands(M, K, N, mode, seed):
    g = torch.Generator().manual_seed(seed)
    return W.fill_(torch.empty(M, K), mode, g), W.fill_(torch.empty(K, N), mode, g)


def _check(mode, A, B, out):
    A, B = torch.as_tensor(A), torch.as_tensor(B)
    return W.compare(_nn(A.shape[0], A.shape[1], B.shape[1]), mode, A[None], B[None], torch.as_tensor(out), None)


# --------------------------------------------------------------------------------------------------------------------- parser

def test_parser_reads_every_shipped_line():
    es = W.read_entries()
    with open(W.SHIPPED) as fh:
        lines = [ln for ln in fh if ln.strip() and not ln.startswith('Validator,')]
    assert len(es) == len(lines) == 381
    assert {e.kind for e in es} == set(W.KINDS.values())
    assert all(W.format_key(e) == e.key for e in es)
    named = [e for e in es if e.solution != 'Default']
    roc = [e for e in named if e.solution.startswith('Gemm_Rocblas_')]
    lt = [e for e in named if e.solution.startswith('Gemm_Hipblaslt_')]
    assert (len(named), len(roc), len(lt)) == (343, 308, 35)
    assert sum(e.kind == 'linear_bias' for e in lt) == 14
    # mlp1 on columns 1083..1093 of the 1094-wide MEDA input rows, and its weight gradient: the only sub-matrix operands
    sub = sorted(e.key for e in es if (e.lda, e.ldb) != tuple(s[1] for s in W.operand_shapes(e)))
    assert sub == ['nt_11_10_61440_ld_1094_10_11', 'nt_11_10_92160_ld_1094_10_11',
                   'tn_10_61440_11_ld_11_1094_10', 'tn_10_92160_11_ld_11_1094_10']


def test_shipped_k_range_is_what_the_bounds_are_calibrated_for():
    """The calibration below runs at the smallest and the largest K of the file: the aggregate bound grows with sqrt(K) while the
    error of tf32-rounded inputs does not, so the largest K is where it discriminates least.  The exact pass needs 9 K + 3 < 2^24."""
    ks = [e.k for e in W.read_entries()]
    assert (min(ks), max(ks)) == K_RANGE
    assert W.EXACT_MAX ** 2 * max(ks) + W.EXACT_MAX < 2 ** 24


@pytest.mark.parametrize('op,key', [
    ('GemmTunableOp_double_TN', 'tn_4_4_4_ld_4_4_4'),                                  # not an fp32 op
    ('ScaledGemmTunableOp_Float8_e4m3fn_Float8_e4m3fn_float_TN', 'tn_4_4_4_ld_4_4_4'),
    ('GemmTunableOp_float_TT', 'tt_4_4_4_ld_4_4_4'),
    ('GemmTunableOp_float_TN', 'nt_4_4_4_ld_4_4_4'),                                   # key layout differs from the op's
    ('GemmTunableOp_float_TN', 'tn_4_4_4'),                                            # no leading dimensions
    ('GemmTunableOp_float_TN', 'tn_4_4_4_ld_4_4_4_rw_0_bias_float'),                   # trailing fields
    ('GemmTunableOp_float_TN', 'tn_4_4_4_B_2_ld_4_4_4'),                               # batch count on a plain GEMM
    ('GemmStridedBatchedTunableOp_float_NT', 'nt_4_4_4_ld_4_4_4'),                     # batched GEMM without one
    ('GemmTunableOp_float_TN', 'tn_10_100_11_ld_10_11_10'),                            # lda < k
    ('GemmTunableOp_float_NN', 'nn_4_4_4_ld_4_4_8'),                                   # C not dense
    ('GemmStridedBatchedTunableOp_float_NT', 'nt_4_4_4_B_2_ld_8_4_4'),                 # batch of sub-matrix views
    ('GemmTunableOp_float_NN', 'nn_0_4_4_ld_4_4_0'),
])
def test_parser_refuses_what_it_does_not_know(op, key):
    with pytest.raises(ValueError):
        W.parse_entry(op, key, 'Default')


def test_read_entries_refuses_a_bad_line(tmp_path):
    f = tmp_path / 'r.csv'
    f.write_text('Validator,PT_VERSION,2.10.0\nGemmTunableOp_float_TN,tn_4_4_4_ld_4_4_4,Default,0.01\n')
    assert [e.key for e in W.read_entries(str(f))] == ['tn_4_4_4_ld_4_4_4']
    for bad in ('GemmTunableOp_float_TN\n', 'GemmTunableOp_half_TN,tn_4_4_4_ld_4_4_4,Default,0.01\n'):
        f.write_text('Validator,PT_VERSION,2.10.0\n' + bad)
        with pytest.raises(ValueError):
            W.read_entries(str(f))


# ---------------------------------------------------------------------------------------------------------------- calibration

@pytest.mark.parametrize('K', K_RANGE)
def test_sequential_fp32_stays_inside_both_bounds(K):
    A, B = _operands(16, K, 16, 'precision', K)
    r = _check('precision', A, B, _seq_fp32(A, B))
    assert r['finite'] and r['elem_ratio'] <= 1.0, r
    assert r['rel_fro'] <= 0.1 * W.agg_bound(K), r          # measured: 0.03-0.09 of the bound


@pytest.mark.parametrize('bits', [10, 7], ids=['tf32', 'bf16'])
@pytest.mark.parametrize('K', K_RANGE)
def test_reduced_precision_inputs_break_the_aggregate_bound(K, bits):
    A, B = _operands(16, K, 16, 'precision', K)
    rounded = (_round_mantissa(A.numpy(), bits).astype(np.float64) @ _round_mantissa(B.numpy(), bits).astype(np.float64))
    r = _check('precision', A, B, rounded.astype(np.float32))
    assert r['rel_fro'] > W.agg_bound(K), (r, W.agg_bound(K))


@pytest.mark.parametrize('K', K_RANGE)
def test_exact_pass_is_exact_and_catches_dropped_or_shifted_data(K):
    A, B = _operands(8, K, 8, 'exact', K)
    assert _check('exact', A, B, _seq_fp32(A, B))['mismatches'] == 0
    # the largest partial sums the exact pass can meet: still exact in fp32
    A3, B3 = torch.full((2, K), 3.0), torch.full((K, 2), -3.0)
    assert _check('exact', A3, B3, _seq_fp32(A3, B3))['mismatches'] == 0
    # the K tail (one element at K = 5, a chunk of 64 at K = 92 160) left out of the sum
    keep = np.ones(K, dtype=bool)
    keep[K - (64 if K >= 64 else 1):] = False
    assert _check('exact', A, B, _seq_fp32(A.numpy()[:, keep], B.numpy()[keep]))['mismatches'] > 0
    # the last row read one element off along K
    out = _seq_fp32(A, B)
    out[-1] = _seq_fp32(np.roll(A.numpy()[-1:], 1, axis=1), B)[0]
    assert _check('exact', A, B, out)['mismatches'] > 0
    # the last output row written one column off
    out = _seq_fp32(A, B)
    out[-1] = np.roll(out[-1], 1)
    assert _check('exact', A, B, out)['mismatches'] > 0


# ------------------------------------------------------------------------------------------------------ the per-entry check

SMALL = [('GemmTunableOp_float_TN', 'tn_24_100_40_ld_40_40_24'),
         ('GemmTunableOp_float_TN', 'tn_7_33_13_ld_13_13_7'),
         ('GemmAndBiasTunableOp_float_TN', 'tn_10_100_11_ld_11_1094_10'),
         ('GemmAndBiasTunableOp_float_TN', 'tn_5_300_128_ld_128_128_5'),
         ('GemmTunableOp_float_NN', 'nn_40_100_24_ld_40_24_40'),
         ('GemmTunableOp_float_NT', 'nt_11_10_100_ld_1094_10_11'),
         ('GemmTunableOp_float_NT', 'nt_128_384_64_ld_128_384_128'),
         ('GemmStridedBatchedTunableOp_float_NT', 'nt_40_24_100_B_4_ld_40_24_40'),
         ('GemmStridedBatchedTunableOp_float_NT', 'nt_7_10_17_B_1_ld_7_10_7')]


@pytest.mark.parametrize('op,key', SMALL)
def test_entry_check_passes_a_correct_product(op, key):
    e = W.parse_entry(op, key)
    ops = W.build(e, 'exact', torch.Generator().manual_seed(0), 'cpu')
    (ra, wa), (rb, wb) = W.operand_shapes(e)
    assert ops['a'].shape == (ra, wa) and ops['a'].stride() == (e.lda, 1)
    assert ops['b'].shape == (rb, wb) and ops['b'].stride() == (e.ldb, 1)
    if e.ldb > wb:     # a view of the last columns of a NaN-filled row: the project's pointer offset (1083 for mlp1)
        base = ops['b'].as_strided((rb, e.ldb), (e.ldb, 1), ops['b'].storage_offset() - (e.ldb - wb))
        assert ops['b'].storage_offset() == e.ldb - wb and torch.isnan(base[:, :e.ldb - wb]).all()
    r = W.check_entry(e, 'cpu', 1)
    assert r['ok'], r


@pytest.mark.parametrize('corrupt', ['shifted_row', 'tf32_inputs', 'reads_slack'])
def test_entry_check_fails_a_corrupted_product(monkeypatch, corrupt):
    e = W.parse_entry('GemmAndBiasTunableOp_float_TN', 'tn_10_100_11_ld_11_1094_10')
    real = W.call

    def bad(e, ops):
        if corrupt == 'tf32_inputs':
            ops = dict(ops, a=torch.from_numpy(_round_mantissa(ops['a'].numpy(), 10)),
                       b=torch.from_numpy(_round_mantissa(ops['b'].numpy(), 10)))
        if corrupt == 'reads_slack':     # one column to the left: the NaN slack in front of the view
            b = ops['b']
            ops = dict(ops, b=b.as_strided(b.shape, b.stride(), b.storage_offset() - 1))
        out = real(e, ops)
        if corrupt == 'shifted_row':
            out[-1] = out[-1].roll(1)
        return out

    monkeypatch.setattr(W, 'call', bad)
    r = W.check_entry(e, 'cpu', 1)
    assert not r['ok']
    if corrupt == 'shifted_row':
        assert not r['exact_ok'] and not r['spot_ok']     # the last row is one of the spot-checked rows
    elif corrupt == 'tf32_inputs':
        assert r['exact_ok'] and r['agg_ratio'] > 1.0     # small integers are exact in tf32: the precision pass catches it
    else:
        assert not r['exact_ok'] and not r['finite']


@pytest.mark.parametrize('B,R,K,C,budget', [(1, 4515840, 32, 288, 1 << 25), (512, 32, 8820, 288, 1 << 25), (1, 10, 92160, 11, 1 << 25),
                                             (1, 100, 40, 24, 1000), (4, 24, 100, 40, 3000), (3, 7, 5, 2, 10)])
def test_reference_pieces_tile_the_output_once(B, R, K, C, budget):
    seen = np.zeros((B, R), dtype=np.int64)
    for bs, rs in W._pieces(B, R, K, C, budget):
        assert bs.stop > bs.start and rs.stop > rs.start
        seen[bs, rs] += 1
    assert (seen == 1).all()


def test_piecewise_comparison_matches_whole():
    """The float64 reference in many small pieces finds the same mismatches and the same errors as in one."""
    e = W.parse_entry('GemmStridedBatchedTunableOp_float_NT', 'nt_40_24_100_B_4_ld_40_24_40')
    res = []
    for budget in (W.CHUNK_DOUBLES, 3000):
        for mode in ('exact', 'precision'):
            ops = W.build(e, mode, torch.Generator().manual_seed(2), 'cpu')
            out = W.call(e, ops)
            out[2, -1, -1] += 1.0
            res.append(W.compare(e, mode, *W.as_batched(e, ops), out, None, budget=budget))
    assert res[0] == res[2] and res[0]['mismatches'] == 1
    assert res[1]['elem_ratio'] == res[3]['elem_ratio'] > 1.0
    assert res[1]['rel_fro'] == pytest.approx(res[3]['rel_fro'], rel=1e-12)


def test_controls_and_call_site_keys():
    es = W.read_entries()
    have = {(e.op, e.key) for e in es}
    ctl = W.control_entries(es)
    assert {e.kind for e in ctl} == set(W.KINDS.values()) and not have & {(e.op, e.key) for e in ctl}
    for c in W.CALLSITE.values():
        assert set(W.callsite_keys(**c)) <= have


# ---------------------------------------------------------------------------------------------------------- split-K glue

def _documented_splitk(M):
    """_wgrad_splitk: the largest S of 64, 32, .., 2 that divides M with M / S >= 512 chunk rows; 1 = one plain GEMM."""
    for S in (64, 32, 16, 8, 4, 2):
        if M % S == 0 and M // S >= 512:
            return S
    return 1


SPLITK_ROWS = [1, 511, 1023, 1024, 1025, 2047, 2048, 2048 * 3, 32767, 32768, 64 * 511, 64 * 512, 2048 * 40, 2048 * 45]


@pytest.mark.parametrize('M', SPLITK_ROWS)
def test_wgrad_splitk_against_float64(monkeypatch, M):
    seen = []
    bmm = torch.bmm
    monkeypatch.setattr(torch, 'bmm', lambda a, b: seen.append(a.shape[0]) or bmm(a, b))
    e = W.parse_entry('GemmTunableOp_float_NT', 'nt_10_7_%d_ld_10_7_10' % M)   # g [M, 7], x [M, 10] -> g^T x [7, 10]
    for mode in ('exact', 'precision'):
        gen = torch.Generator().manual_seed(M)
        g, x = W.fill_(torch.empty(M, 7), mode, gen), W.fill_(torch.empty(M, 10), mode, gen)
        got = base_net._wgrad_splitk(g, x)
        r = W.compare(e, mode, g.t()[None], x[None], got, None)
        if mode == 'exact':
            assert r['mismatches'] == 0
        else:
            assert r['finite'] and r['elem_ratio'] <= 1.0 and r['rel_fro'] <= W.agg_bound(M), r
    S = seen[0] if seen else 1
    assert S == _documented_splitk(M) == W.splitk_chunks(M)
    assert all(s == S for s in seen)
    if S > 1:
        assert M % S == 0 and M // S >= 512


def _documented_colsum(M):
    """_colsum: the largest first-stage split of 256, 128, 64, 32 that divides M and leaves >= 64 rows per part; 1 = one sum."""
    for c in (256, 128, 64, 32):
        if M % c == 0 and M // c >= 64:
            return c
    return 1


@pytest.mark.parametrize('M', [1, 31, 2047, 2048, 4096, 8191, 8192, 16383, 16384, 16384 * 3, 81920, 92160])
def test_colsum_against_float64(monkeypatch, M):
    parts = []
    reshape = torch.Tensor.reshape
    monkeypatch.setattr(torch.Tensor, 'reshape', lambda t, *s: parts.append(s[0]) or reshape(t, *s))
    for mode in ('exact', 'precision'):
        t = W.fill_(torch.empty(M, 5), mode, torch.Generator().manual_seed(M))
        got = base_net._colsum(t).double()
        want = t.double().sum(0)
        if mode == 'exact':
            assert torch.equal(got, want)
        else:
            bound = 1.01 * M * W.U * t.double().abs().sum(0)
            assert ((got - want).abs() <= bound).all()
    assert (parts[0] if parts else 1) == _documented_colsum(M)


@pytest.mark.parametrize('M,bias', [(1, True), (1023, True), (1024, False), (4096, True), (32768, False)])
def test_linear_splitk_against_float64_autograd(M, bias):
    """_LinearSplitK with a zero-padded weight (as the GRU input projection) against float64 autograd of x @ W^T + b."""
    gen = torch.Generator().manual_seed(M)
    x = torch.randn(M, 64, generator=gen)
    x[:, 60:] = 0.0
    w = torch.randn(5, 60, generator=gen) * 0.1
    b = torch.randn(5, generator=gen) if bias else None
    gy = torch.randn(M, 5, generator=gen)
    res = []
    for dt in (torch.float32, torch.float64):
        leaves = [t.to(dt, copy=True).requires_grad_(True) for t in (x, w) + ((b,) if bias else ())]
        wp = torch.nn.functional.pad(leaves[1], (0, 4))
        bb = leaves[2] if bias else None
        y = base_net._LinearSplitK.apply(leaves[0], wp, bb) if dt == torch.float32 else leaves[0] @ wp.t() + (bb if bias else 0.0)
        res.append((y.detach(),) + torch.autograd.grad(y, leaves, gy.to(dt)))
    for name, g, r in zip(('y', 'gx', 'gw', 'gb'), *res):
        assert g.dtype == torch.float32
        rel = float((g.double() - r).norm() / (r.norm() + 1e-300))
        assert rel <= GRAD_TOL, (name, rel)
