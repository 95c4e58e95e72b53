"""The MEDA global state (include/meda_vec.h: meda_vec_global_obs / _append / _stage_first / _stage_close), int8[2][W][L] per chip
indexed [layer][y][x]: droplet boxes in layer 0, destination boxes in layer 1, value i + 1, clipped to the chip, the last droplet
index winning a shared cell.  Checked bit for bit against a numpy restatement of that contract built from get_state() / get_task()
over many chips and autoreset steps (non-square chips included, so that a y / x swap fails), the episode append rule, and the
continuous rollout's stage and close entry points with their argument checks."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def numpy_meda_state(W, L, pos, ends):
    """The contract restated: (E, n, 2) droplet centres and (E, n, 2) destination centres as (x, y) -> int8 (E, 2, W, L)."""
    E, n = pos.shape[:2]
    out = np.zeros((E, 2, W, L), np.int8)
    for e in range(E):
        for i in range(n):
            for layer, (x, y) in ((0, pos[e, i]), (1, ends[e, i])):
                out[e, layer, max(y - 2, 0):min(y + 2, W - 1) + 1, max(x - 2, 0):min(x + 2, L - 1) + 1] = i + 1
    return out


def env_state(env):
    pos = env.get_state()['pos'].cpu().numpy()
    ends = env.get_task()[1].cpu().numpy()
    return numpy_meda_state(env.width, env.length, pos, ends)


def overlapping_chips(pos):
    """Chips with two droplet boxes that share a cell (|dx| <= 4 and |dy| <= 4)."""
    d = np.abs(pos[:, :, None, :] - pos[:, None, :, :]).max(-1)
    n = pos.shape[1]
    d[:, np.arange(n), np.arange(n)] = 99
    return int((d <= 4).any(axis=(1, 2)).sum())


def _rand_bytes(shape, gen):
    return torch.randint(-128, 128, shape, dtype=torch.int8, device=DEV, generator=gen)


def _make(W, L, n, E, seed, version=2):
    from marl_dmfb_amd.env.meda import VecMEDA
    return VecMEDA(W, L, n, fov=19, n_envs=E, seed=seed, device=DEV, version=version)


CONFIGS = [(30, 30, 4, 4099), (45, 30, 6, 4099), (30, 60, 8, 4099), (80, 80, 10, 1031)]


@pytest.mark.parametrize('version', [0, 2])
@pytest.mark.parametrize('W,L,n,E', CONFIGS, ids=['%dx%d_%dd_E%d' % c for c in CONFIGS])
def test_many_chips_autoreset_against_restatement(W, L, n, E, version):
    env = _make(W, L, n, E, seed=W + L + n + version, version=version)
    assert env.state_shape == 2 * W * L == env.lib.meda_vec_state_len(env.h)
    env.reset()
    gen = torch.Generator(device=DEV).manual_seed(W * L + version)
    T = env.max_step
    overlaps = 0
    for t in range(T + T // 2):   # through the autoreset of the first episodes
        if t < 2 or t % 20 == 19:
            want = env_state(env)
            np.testing.assert_array_equal(env.global_obs().cpu().numpy(), want, err_msg='t=%d' % t)
            overlaps += overlapping_chips(env.get_state()['pos'].cpu().numpy())
        env.step(torch.randint(0, 9, (E, n), device=DEV, generator=gen, dtype=torch.int32), autoreset=True)
    assert overlaps > 0, 'no chip with overlapping droplet boxes: the last-writer rule was not exercised'
    # the masked form leaves the other rows alone
    out = torch.full((E, 2, W, L), 77, dtype=torch.int8, device=DEV)
    mask = (torch.arange(E, device=DEV) % 3 == 0).to(torch.uint8)
    env.global_obs(mask=mask, out=out)
    full = env.global_obs()
    m = mask.bool()
    assert torch.equal(out[m], full[m]) and bool((out[~m] == 77).all())


def test_state_on_a_hand_built_task():
    """Known boxes on a 30 x 45 chip (W = 30 rows y, L = 45 columns x): a box clipped at a corner, two overlapping droplet boxes
    (the higher index wins) and the (x, y) order of the centres."""
    env = _make(30, 45, 3, 2, seed=1)
    starts = np.array([[[3, 2], [5, 3], [40, 20]], [[10, 6], [1, 29], [14, 2]]], np.int32)
    ends = np.array([[[10, 6], [15, 2], [3, 9]], [[3, 13], [17, 8], [30, 2]]], np.int32)
    env.set_task(starts, ends)
    g = env.global_obs().cpu().numpy()
    assert g.shape == (2, 2, 30, 45)
    np.testing.assert_array_equal(g, numpy_meda_state(30, 45, starts, ends))
    assert g[0, 0, 2, 1] == 1 and g[0, 0, 3, 5] == 2 and g[0, 0, 0, 1] == 1 and g[0, 0, 20, 40] == 3
    assert g[0, 0, 3, 3] == 2   # shared by droplets 0 and 1
    assert g[0, 1, 6, 10] == 1 and g[0, 1, 10, 10] == 0 and g[0, 1, 9, 3] == 3
    assert (g[1, 0, 27:, :4] == 2).all() and g[1, 0, 26, 0] == 0 and g[1, 0, 29, 4] == 0   # clipped at the corner
    assert int((g[1, 0] == 2).sum()) == 12


def test_append_rule():
    E, W, L, n, T = 64, 30, 45, 4, 6
    env = _make(W, L, n, E, seed=2)
    env.reset()
    S = env.state_shape
    s = torch.zeros((E, T, S), dtype=torch.int8, device=DEV)
    sn = torch.zeros_like(s)
    alive = (torch.arange(E, device=DEV) % 4 != 0).to(torch.uint8)
    term = (torch.arange(E, device=DEV) % 4 == 1).to(torch.uint8)
    cur = env.global_obs().view(E, S)
    assert bool((cur.abs().sum(1) > 0).all())
    for t in (2, T - 1):
        env.global_obs_append(alive, term, t, s, sn)
        a, tm = alive.bool(), term.bool()
        assert torch.equal(sn[a, t], cur[a]) and bool((sn[~a, t] == 0).all())
        if t + 1 < T:
            keep = a & ~tm
            assert torch.equal(s[keep, t + 1], cur[keep]) and bool((s[~keep, t + 1] == 0).all())
    assert int(s[:, :3].abs().sum()) == 0 and int(s[:, 4:].abs().sum()) == 0   # nothing else written (t = T - 1 writes no s)
    assert int(sn[:, :2].abs().sum()) == 0 and int(sn[:, 3:T - 1].abs().sum()) == 0


STAGE = [(1, 30, 30, 4, 5), (65, 45, 30, 6, 4), (4099, 30, 30, 4, 5), (300, 80, 80, 10, 3)]


@pytest.mark.parametrize('E,W,L,n,T', STAGE, ids=['E%d_%dx%d' % c[:3] for c in STAGE])
def test_stage_and_close_against_restatement(E, W, L, n, T):
    """stage_first with a random mask, one random step, then stage_close with synthetic step indices (t = T - 1 included) and three
    closing patterns: a sparse random set, none, and every chip at once into a ring of exactly E slots about to wrap.  Rows of
    (T + 1) * S = 10 800 (8-byte aligned rows), 13 500 and 51 200 bytes (80x80: four close chunks)."""
    env = _make(W, L, n, E, seed=E + W)
    env.reset()
    S = env.state_shape
    gen = torch.Generator(device=DEV).manual_seed(E * 7 + W)
    stage = _rand_bytes((E, T + 1, S), gen)
    mask = (torch.rand(E, device=DEV, generator=gen) < 0.5).to(torch.uint8)
    mask[0] = 1
    want = stage.cpu().numpy()
    st0 = env_state(env).reshape(E, S)
    env.global_obs_stage_first(mask, stage)
    m = mask.cpu().numpy().astype(bool)
    want[m, 0] = st0[m]
    np.testing.assert_array_equal(stage.cpu().numpy(), want)
    env.step(torch.randint(0, 9, (E, n), device=DEV, generator=gen, dtype=torch.int32))
    st1 = env_state(env).reshape(E, S)
    for pattern in ('sparse', 'none', 'all_wrap'):
        slots = E if pattern == 'all_wrap' else E + 5
        ring = _rand_bytes((slots, T + 1, S), gen)
        t_ep = torch.randint(0, T, (E,), device=DEV, generator=gen, dtype=torch.int32)
        t_ep[::3] = T - 1
        if pattern == 'sparse':
            close = torch.full((E,), -1, dtype=torch.int32, device=DEV)
            pick = torch.rand(E, device=DEV, generator=gen) < 0.2
            pick[-1] = True
            close[pick] = torch.randperm(slots, device=DEV, generator=gen)[:int(pick.sum())].to(torch.int32)
        elif pattern == 'none':
            close = torch.full((E,), -1, dtype=torch.int32, device=DEV)
        else:
            close = ((E - 3 + torch.arange(E, device=DEV)) % E).to(torch.int32)
        want_st, want_ring = stage.cpu().numpy(), ring.cpu().numpy()
        te, cs = t_ep.cpu().numpy(), close.cpu().numpy()
        want_st[np.arange(E), te + 1] = st1
        for e in np.nonzero(cs >= 0)[0]:
            want_ring[cs[e], :te[e] + 2] = want_st[e, :te[e] + 2]
            want_ring[cs[e], te[e] + 2:] = 0
        env.global_obs_stage_close(t_ep, close, stage, ring)
        np.testing.assert_array_equal(stage.cpu().numpy(), want_st, err_msg=pattern)
        np.testing.assert_array_equal(ring.cpu().numpy(), want_ring, err_msg=pattern)


def test_misaligned_destinations_and_out_of_range():
    """Stage and ring one and three bytes off 16-byte alignment (the writer's byte head and tail, the close's byte path), and
    device-side values outside the contract: step indices -1 / T and slots >= slots are skipped, nothing else is written."""
    E, W, L, n, T = 65, 45, 30, 6, 6
    env = _make(W, L, n, E, seed=4)
    env.reset()
    S = env.state_shape
    gen = torch.Generator(device=DEV).manual_seed(3)
    st = env_state(env).reshape(E, S)
    for offset in (0, 1, 3):
        slots = E + 2
        flat_st = _rand_bytes((E * (T + 1) * S + 16,), gen)
        stage = flat_st[offset:offset + E * (T + 1) * S].view(E, T + 1, S)
        flat = _rand_bytes((slots * (T + 1) * S + 16,), gen)
        ring = flat[offset:offset + slots * (T + 1) * S].view(slots, T + 1, S)
        t_ep = torch.randint(0, T, (E,), device=DEV, generator=gen, dtype=torch.int32)
        close = torch.randperm(slots, device=DEV, generator=gen)[:E].to(torch.int32)
        t_ep[0], t_ep[1], close[2], close[3], close[4] = -1, T, slots, 1 << 30, -7
        want_flat_st, want_flat = flat_st.cpu().numpy(), flat.cpu().numpy()
        want_st = want_flat_st[offset:offset + E * (T + 1) * S].reshape(E, T + 1, S)
        want_ring = want_flat[offset:offset + slots * (T + 1) * S].reshape(slots, T + 1, S)
        te, cs = t_ep.cpu().numpy(), close.cpu().numpy()
        for e in range(E):
            if 0 <= te[e] < T:
                want_st[e, te[e] + 1] = st[e]
                if 0 <= cs[e] < slots:
                    want_ring[cs[e], :te[e] + 2] = want_st[e, :te[e] + 2]
                    want_ring[cs[e], te[e] + 2:] = 0
        env.global_obs_stage_close(t_ep, close, stage, ring)
        np.testing.assert_array_equal(flat_st.cpu().numpy(), want_flat_st, err_msg='stage, offset %d' % offset)
        np.testing.assert_array_equal(flat.cpu().numpy(), want_flat, err_msg='ring, offset %d' % offset)
        # the dense form into a misaligned buffer: the bytes around the rows stay
        flat_d = _rand_bytes((E * S + 32,), gen)
        want_d = flat_d.cpu().numpy()
        want_d[offset:offset + E * S] = st.reshape(-1)
        env.global_obs(out=flat_d[offset:offset + E * S].view(E, 2, W, L))
        np.testing.assert_array_equal(flat_d.cpu().numpy(), want_d, err_msg='dense, offset %d' % offset)


def test_bad_arguments_are_refused_before_any_launch():
    E, T = 8, 4
    env = _make(30, 30, 2, E, seed=1)
    S = env.state_shape
    stage = torch.full((E, T + 1, S), 5, dtype=torch.int8, device=DEV)
    ring = torch.full((E, T + 1, S), 6, dtype=torch.int8, device=DEV)
    s = torch.full((E, T, S), 7, dtype=torch.int8, device=DEV)
    t_ep = torch.zeros(E, dtype=torch.int32, device=DEV)
    close = torch.zeros(E, dtype=torch.int32, device=DEV)
    alive = torch.ones(E, dtype=torch.uint8, device=DEV)
    lib, h, null = env.lib, env.h, None
    p = lambda t: t.data_ptr()
    first = [(h, null, 0, p(stage), null), (h, null, -1, p(stage), null), (h, null, T, null, null), (null, null, T, p(stage), null)]
    close_ = [(h, null, p(close), T, p(stage), p(ring), E, null), (h, p(t_ep), null, T, p(stage), p(ring), E, null),
              (h, p(t_ep), p(close), T, null, p(ring), E, null), (h, p(t_ep), p(close), T, p(stage), null, E, null),
              (null, p(t_ep), p(close), T, p(stage), p(ring), E, null), (h, p(t_ep), p(close), 0, p(stage), p(ring), E, null),
              (h, p(t_ep), p(close), T, p(stage), p(ring), E - 1, null)]
    append = [(h, null, p(alive), 0, T, p(s), p(s), null), (h, p(alive), null, 0, T, p(s), p(s), null),
              (h, p(alive), p(alive), 0, T, null, p(s), null), (h, p(alive), p(alive), 0, T, p(s), null, null),
              (h, p(alive), p(alive), -1, T, p(s), p(s), null), (h, p(alive), p(alive), T, T, p(s), p(s), null),
              (null, p(alive), p(alive), 0, T, p(s), p(s), null)]
    for a in first:
        with pytest.raises(ValueError):
            lib.meda_vec_global_obs_stage_first(*a)
    for a in close_:
        with pytest.raises(ValueError):
            lib.meda_vec_global_obs_stage_close(*a)
    for a in append:
        with pytest.raises(ValueError):
            lib.meda_vec_global_obs_append(*a)
    for a in [(h, null, null, null), (null, null, p(stage), null)]:
        with pytest.raises(ValueError):
            lib.meda_vec_global_obs(*a)
    assert lib.meda_vec_state_len(null) < 0
    torch.cuda.synchronize()
    assert bool((stage == 5).all()) and bool((ring == 6).all()) and bool((s == 7).all())
    one = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    one[3] = 2
    lib.meda_vec_global_obs_stage_close(h, p(t_ep), p(one), T, p(stage), p(ring), E, null)   # a legal call does write
    torch.cuda.synchronize()
    assert not bool((ring == 6).all())
