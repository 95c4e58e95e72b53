"""What can be verified of tests/test_gpu_front_kernels.py without a GPU: every exact case it uses meets the conditions that
make float32 exact on it (tests/front_kernel_cases.py), the float64 reference agrees with a second, independent formulation
(numpy loops over the taps), and the guarded allocator notices a write on either side."""
import numpy as np
import pytest
import torch

import front_kernel_cases as K

KEYS = sorted(K.RECIPE)


@pytest.mark.parametrize('fov,od', KEYS)
def test_backward_cases_meet_the_exactness_conditions(fov, od):
    for rows in K.bwd_rows(fov, od):
        r = K.conditions(K.make_case(fov, od, rows))
        assert r.grads.numel() == K.n_grads(fov, od)
        assert r.names == {5: ['dW1', 'db1'], 19: ['dW3', 'db3', 'dW1', 'db1']}.get(fov, ['dW2', 'db2', 'dW1', 'db1'])
        # integers throughout: the float32 image of the reference is the reference
        for t in (r.out, r.grads, r.mlp_dw, r.mlp_db):
            assert torch.equal(t, t.round()) and torch.equal(t.float().double(), t)


@pytest.mark.parametrize('fov,od', KEYS)
def test_forward_cases_meet_the_exactness_conditions(fov, od):
    rows = K.fwd_rows(fov, od)
    rb, grid = K.FWD_RB[(fov, od)], K.fwd_grid(fov, od)
    assert rows[:4] == [1, rb - 1, rb, rb + 1]
    n_blocks = -(-rows[4] // rb)
    assert n_blocks == grid + 2 and rows[4] % rb != 0       # workgroups 0 and 1 take a second block, the last one is ragged
    for n in rows:
        K.conditions(K.make_case(fov, od, n), backward=False)
    for n_actions in (0, 1, 16):
        K.conditions(K.make_case(fov, od, rb + 1, n_actions=n_actions), backward=False)


def test_wrapping_row_counts_are_the_ones_the_sources_give():
    assert K.fwd_rows(9, 24)[4] == 4096 + 16 + 5 and K.fwd_rows(9, 32)[4] == 3072 + 12 + 5
    assert K.fwd_rows(19, 24)[4] == K.fwd_rows(19, 32)[4] == 2048 + 8 + 3
    assert [K.fwd_grid(f, o) for f, o in ((7, 24), (7, 32), (5, 24), (5, 32))] == [512, 256, 1792, 1280]
    assert K.bwd_rows(9, 24) == [1, 9, 11, 32, 103] and K.bwd_rows(19, 32) == [1, 3, 8, 23] and K.bwd_rows(5, 24) == [1, 31, 33, 98, 323]


@pytest.mark.parametrize('fov,od,rows', [(9, 24, 11), (19, 24, 5), (7, 32, 9), (5, 24, 33)])
def test_reference_agrees_with_numpy_loops_over_the_taps(fov, od, rows):
    c = K.make_case(fov, od, rows)
    r = K.reference(c)
    out, flat, dw, db = K.numpy_reference(c)
    assert np.array_equal(out, r.out.numpy())
    assert np.array_equal(flat, r.grads.numpy())
    assert np.array_equal(dw, r.mlp_dw.numpy()) and np.array_equal(db, r.mlp_db.numpy())
    # one channel pair and the bias sums spelled out element by element, from the pre-activation gradients of the numpy form
    od_, nc = c.od, K.n_conv(fov, od)
    if fov in (7, 9):
        n2 = od_ * od_ * 9
        x = c.obs[:, :K.n_pix(fov)].numpy().astype(np.float64).reshape(rows, 3, fov, fov)
        w1, b1 = c.w1.numpy().astype(np.float64), c.b1.numpy().astype(np.float64)
        s = fov - 2
        a1 = np.zeros((rows, od_, s, s))
        for ch in range(od_):
            for i in range(s):
                for j in range(s):
                    a1[:, ch, i, j] = np.maximum((x[:, :, i:i + 3, j:j + 3] * w1[ch]).sum(axis=(1, 2, 3)) + b1[ch], 0.0)
        dz2 = (c.g.numpy()[:, :nc].astype(np.float64) * (r.conv.numpy() > 0)).reshape(rows, od_, s - 2, s - 2)
        c2, c1 = 3, od_ - 2
        for kx in range(3):
            for ky in range(3):
                want = sum(dz2[n, c2, i, j] * a1[n, c1, i + kx, j + ky] for n in range(rows) for i in range(s - 2) for j in range(s - 2))
                assert r.grads[(c2 * od_ + c1) * 9 + kx * 3 + ky].item() == want
        assert np.array_equal(r.grads[n2:n2 + od_].numpy(), dz2.sum(axis=(0, 2, 3)))


def test_mlp_case_reference_is_a_plain_sum():
    c = K.mlp_case(257, 5, seed=3)
    v = np.concatenate([c.dirs.numpy(), c.onehot.numpy()], axis=1).astype(np.float64)
    dw, db = np.zeros((10, 7)), np.zeros(10)
    for n in range(c.rows):
        for o in range(10):
            if c.x[n, o] > 0:
                dw[o] += float(c.g[n, o]) * v[n]
                db[o] += float(c.g[n, o])
    assert np.array_equal(dw, c.dw.numpy()) and np.array_equal(db, c.db.numpy())
    assert np.abs(dw).max() <= c.bound < K.BOUND_LIMIT and K.mlp_case(70001, 16, seed=4).bound < K.BOUND_LIMIT


@pytest.mark.parametrize('dtype,fill', [(torch.float32, float('nan')), (torch.float32, -777.25), (torch.int8, 127)])
def test_guarded_buffers_notice_a_write_on_either_side(dtype, fill):
    view, check = K.guarded((3, 5), dtype, fill, offset=1)
    assert view.shape == (3, 5) and view.is_contiguous() and view.data_ptr() % 8 == (4 if dtype == torch.float32 else 1)
    check()
    view.fill_(1)
    check()
    base = view.view(-1)
    for k in (-1, 15):      # the element just before and just behind the view
        t = torch.as_strided(base, (1,), (1,), base.storage_offset() + k)
        old = t.clone()
        t.fill_(2)
        with pytest.raises(AssertionError):
            check()
        t.copy_(old)
        check()
