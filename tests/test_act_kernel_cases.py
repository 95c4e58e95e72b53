"""What can be verified of tests/test_gpu_act_kernels.py without a GPU: the float64 GRU cell + Q head of
tests/act_kernel_cases.py is nn.GRUCell + nn.Linear in double precision, its pick is the scalar rule of include/rollout_ops.h
restated here row by row with a Philox of its own, the helpers for the expected episode tensors put every pick where the header
says, and every input set that the GPU module compares with float64 by tolerance has at most 1 % near-tie rows."""
import numpy as np
import pytest
import torch

import act_kernel_cases as K


@pytest.mark.parametrize('A', [1, 5, 9, 16])
def test_reference_is_grucell_and_linear_in_double(A):
    rows, F = 37, 70
    torch.manual_seed(A)
    cell = torch.nn.GRUCell(F, K.H).double()
    fc = torch.nn.Linear(K.H, A).double()
    x = torch.randn(rows, F, dtype=torch.float64)
    h0 = torch.rand(rows, K.H, dtype=torch.float64) * 2 - 1
    with torch.no_grad():
        h_want = cell(x, h0)
        q_want = fc(h_want)
        ig = x @ cell.weight_ih.t()
        hg = h0 @ cell.weight_hh.t()
    h, q = K.gru_head_reference(ig.numpy(), hg.numpy(), cell.bias_ih.detach().numpy(), cell.bias_hh.detach().numpy(), h0.numpy(),
                                fc.weight.detach().numpy(), fc.bias.detach().numpy())
    assert h.dtype == np.float64 and q.dtype == np.float64 and q.shape == (rows, A)
    # rtol 1e-12; h' = n + z (h - n) is a difference of numbers of magnitude up to 1, each rounded to half an ulp of 1 (2^-53) in
    # either implementation, so an element that cancels to 1e-4 carries an ABSOLUTE error of a few 2^-53 whatever its size:
    # 8 * 2^-53 = 9e-16 is allowed for on top (ten orders of magnitude below the GPU tolerances)
    np.testing.assert_allclose(h, h_want.numpy(), rtol=1e-12, atol=8 * 2.0 ** -53)
    np.testing.assert_allclose(q, q_want.numpy(), rtol=1e-12, atol=8 * 2.0 ** -53)


def test_reference_survives_overflowing_gates():
    c = K.spike(K.make_inputs(17, 5, seed=1, scale=8.0))
    assert int((np.abs(c.ig) == 1.0e4).sum()) == 48
    h, q = K.gru_head_reference(c.ig, c.hg, c.b_ih, c.b_hh, c.h, c.fc_w, c.fc_b)
    assert np.isfinite(h).all() and np.isfinite(q).all() and np.abs(h).max() <= 1.0


def _philox_scalar(k0, k1, c):
    """Philox4x32-10 in Python integers (Salmon et al. 2011)."""
    c = [int(x) for x in c]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k1) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def _pick_scalar(q_row, seed, draw, eps, evaluate, row):
    """include/rollout_ops.h lines 30-32 for one row."""
    best = 0
    for k in range(1, len(q_row)):
        if q_row[k] > q_row[best]:
            best = k
    if evaluate:
        return best, None
    w = _philox_scalar(seed & 0xFFFFFFFF, seed >> 32, (row, draw, 0, 0x600))
    u1 = np.float32(w[0] >> 8) * np.float32(2.0 ** -24)
    if u1 < np.float32(eps):
        return (w[1] * len(q_row)) >> 32, u1
    return best, u1


def test_philox_known_answers():
    """The vectors of Random123's kat_vectors for philox4x32-10: the scalar restatement above and the oracle's."""
    from oracle.dmfb_oracle import philox
    for key, ctr, want in (((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
                            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(_philox_scalar(key[0], key[1], ctr)) == want
        assert tuple(int(x) for x in philox(key[0], key[1], ctr)) == want


@pytest.mark.parametrize('draw', K.DRAWS)
@pytest.mark.parametrize('A', [1, 5, 16, 127])
def test_pick_reference_is_the_scalar_rule(draw, A):
    rows = 67
    g = np.random.default_rng(A)
    q = g.standard_normal((rows, A)).astype(np.float32)
    q[3] = q[3, 0]                                   # all equal: the first
    if A >= 5:
        q[4, 1] = q[4, 3] = q[4].max() + 1.0         # a repeated maximum behind position 0
        q[5] = -1.0
        q[5, 2], q[5, 4] = -0.0, 0.0                 # -0.0 before +0.0: equal, so the first
    row_ids = np.arange(rows) * 1031 + 5             # not 0..rows-1: the counter takes the id, not the position
    seeds = (K.SEED, 0x00000001_00000000, 0x00000000_00000001)
    for seed in seeds:
        for eps in (0.0, 0.3, 1.0):
            act, u1 = K.pick_reference(q, seed, draw, eps, 0, row_ids)
            n_rand = 0
            for r in range(rows):
                want, wu = _pick_scalar(q[r], seed, draw, eps, 0, int(row_ids[r]))
                assert (int(act[r]), u1[r]) == (want, wu), (seed, eps, r)
                assert 0 <= act[r] < A and 0.0 <= u1[r] < 1.0
                n_rand += bool(wu < np.float32(eps))
            assert n_rand == {0.0: 0, 1.0: rows}.get(eps, n_rand)
    a_lo, _ = K.pick_reference(q, seeds[1], draw, 1.0, 0, row_ids)
    a_hi, _ = K.pick_reference(q, seeds[2], draw, 1.0, 0, row_ids)
    assert A == 1 or not np.array_equal(a_lo, a_hi), 'the two halves of the seed are interchangeable'
    act, u1 = K.pick_reference(q, K.SEED, draw, 0.3, 1, row_ids)
    assert [int(a) for a in act] == [_pick_scalar(q[r], K.SEED, draw, 0.3, 1, 0)[0] for r in range(rows)]
    assert act[3] == 0 and (A < 5 or (act[4] == 1 and act[5] == 2))


def test_epsilon_on_a_rows_draw_keeps_that_row_greedy():
    rows, A = 67, 5
    q = np.random.default_rng(0).standard_normal((rows, A)).astype(np.float32)
    u1 = K.draw_u1(K.SEED, 7, np.arange(rows))
    k = int(np.argsort(u1)[rows // 2])
    act, u1b = K.pick_reference(q, K.SEED, 7, float(u1[k]), 0, np.arange(rows))
    assert np.array_equal(u1, u1b) and float(u1[k]) == u1[k]
    greedy = K.first_max(q)
    rand = ((K.draw_words(K.SEED, 7, np.arange(rows))[:, 1] * np.uint64(A)) >> np.uint64(32)).astype(np.int64)
    assert act[k] == greedy[k]
    assert np.array_equal(act, np.where(u1 < u1[k], rand, greedy)) and int((u1 < u1[k]).sum()) >= rows // 2 - 1


def test_episode_helpers_put_each_pick_in_its_slot():
    E, n, A, T = 3, 2, 4, 5
    act = np.array([0, 3, 1, 1, 2, 0])
    assert np.array_equal(K.onehots(act, A).argmax(1), act) and (K.onehots(act, A).sum(1) == 1).all()
    u, oh = K.episode_slots(act, E, n, A, T, 4, -99)
    assert np.array_equal(u[:, 4].reshape(-1), act) and (u[:, :4] == -99).all()
    assert np.array_equal(oh[:, 4].reshape(-1, A), K.onehots(act, A)) and (oh[:, :4] == -99).all()
    u, oh = K.episode_slots(act, E, n, A, T, [0, 4, 2], -99, rows=[2, 3, 4, 5])
    assert (u[0] == -99).all() and (oh[0] == -99).all()
    assert u[1, 4].tolist() == [1, 1] and u[2, 2].tolist() == [2, 0] and int((u != -99).sum()) == 4
    assert int((oh != -99).sum()) == 4 * A and oh[2, 2, 0].tolist() == [0, 0, 1, 0]


def test_row_shapes_and_live_cases_cover_the_edges():
    assert [E * n for E, n in K.ROW_SHAPES] == [1, 7, 8, 9, 15, 16, 17, 4099]
    assert {n for _, n in K.ROW_SHAPES} >= {1, 3, 4}
    live = {'all': lambda E: E, 'none': lambda E: 0, 'first': lambda E: 1, 'last': lambda E: 1}
    mods = {live[kind](E) * n % K.ROWS_PER_GROUP for E, n, _, kind in K.LIVE_CASES if kind in live}
    assert mods >= {0, 1, 7}
    assert {kind for *_, kind in K.LIVE_CASES} == {'all', 'none', 'first', 'last', 'half'}


@pytest.mark.parametrize('rows,A,seed,scale', K.TOLERANCE_SETS)
def test_near_ties_are_at_most_one_percent_of_the_rows(rows, A, seed, scale):
    c = K.make_inputs(rows, A, seed, scale)
    h, q = K.reference(c)
    assert np.isfinite(h).all() and np.isfinite(q).all()
    ties = K.top2_gap(q) <= K.GAP
    assert ties.mean() <= K.MAX_TIE_ROWS, (rows, A, int(ties.sum()))
    assert A > 1 or not ties.any()


def test_float32_unrolling_sits_well_inside_the_tolerances():
    """The same formulas in float32 numpy against float64 at 4099 rows: the reference alone uses a third of H_TOL and a
    sixteenth of Q_TOL at the most, so the tolerances are the kernels' to spend."""
    worst_h = worst_q = 0.0
    for A in (5, 16):
        c = K.make_inputs(4099, A)
        f = np.float32
        sig = lambda x: f(1) / (f(1) + np.exp(-x))
        r = sig(c.ig[:, :K.H] + c.hg[:, :K.H] + c.b_ih[:K.H] + c.b_hh[:K.H])
        z = sig(c.ig[:, K.H:2 * K.H] + c.hg[:, K.H:2 * K.H] + c.b_ih[K.H:2 * K.H] + c.b_hh[K.H:2 * K.H])
        n = np.tanh(c.ig[:, 2 * K.H:] + c.b_ih[2 * K.H:] + r * (c.hg[:, 2 * K.H:] + c.b_hh[2 * K.H:]))
        h32 = n + z * (c.h - n)
        q32 = np.zeros((c.rows, A), dtype=np.float32)
        for k in range(K.H):
            q32 += h32[:, k:k + 1] * c.fc_w[:, k]
        q32 += c.fc_b
        assert h32.dtype == np.float32 and q32.dtype == np.float32
        h, q = K.reference(c)
        worst_h, worst_q = max(worst_h, np.abs(h32 - h).max()), max(worst_q, np.abs(q32 - q).max())
    assert worst_h <= K.H_TOL / 3 and worst_q <= K.Q_TOL / 16, (worst_h, worst_q)
