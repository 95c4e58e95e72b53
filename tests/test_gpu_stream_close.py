"""rollout_stream_step (include/rollout_ops.h, continuous rollout) against an independent restatement of its contract.

The kernel is driven directly through the C ABI with synthetic inputs, lock-step after lock-step with alternating parity as
common/rollout.py: _play_stream drives it.  The test stages the picks (u / one-hot) itself; rewards, constraints and success
come from a seeded generator; observation bytes are a cheap hash of (chip, lock-step, byte) with a different salt for the
observation the step was chosen from, the one after it and the terminal one.  Termination is random at a set density and
forced at t_ep == T - 1 (the env guarantees that at episode_limit).  Chips may start in the middle of an episode: the earlier
part of it is pre-staged from the same hashes.

After every lock-step the host model (numpy: step indices, running sums, ring cursor / size / total, slots, statistics,
epsilon, draw counter) and the device state must agree bit for bit, and the ring rows of every episode closed in that
lock-step are rebuilt on the device (exact integer torch ops) and compared with torch.equal.  There is no float tolerance
anywhere.  The matrix reaches every form of the kernel (per-chip dword copy, shared dword copy, byte rows, a misaligned
pointer), one and several passes of both counting schemes, unaligned flag tails, every chip closing at once and a ring
of exactly n_envs slots whose cursor is about to wrap."""
import ctypes as C

import numpy as np
import pytest
import torch

from marl_dmfb_amd import _lib

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
M32 = 0xFFFFFFFF
PREV, NEW, TERM, PICK = 1, 2, 3, 4        # hash salts
COOP_MIN_WORDS = 16384                    # rollout_ops.hip: kCoopMinWords (only used to label the form a case takes)


def _key(salt, e, s):
    """32-bit hash of (salt, chip, lock-step) as int64 (s >= -8192)."""
    x = (salt * 0x9E3779B1 + e * 0x85EBCA6B + (s + 8192) * 0xC2B2AE35) & M32
    x = (((x >> 16) ^ x) * 0x45D9F3B) & M32
    x = (((x >> 16) ^ x) * 0x45D9F3B) & M32
    return (x >> 16) ^ x


def _rows(salt, e, s, row):
    """Observation row of (chip e, lock-step s): uint8 (..., row); byte k = byte k % 4 of the hash + a fixed pattern of k."""
    dev = e.device if isinstance(e, torch.Tensor) else s.device
    h = torch.as_tensor(_key(salt, e, s), device=dev)
    b = ((h.unsqueeze(-1) >> torch.tensor([0, 8, 16, 24], device=dev)) & 255).to(torch.uint8)
    k = torch.arange(row, device=dev)
    return b[..., k % 4] + ((k * 157 + (k >> 2) * 59 + 11) & 255).to(torch.uint8)


def _picks(e, s, n, A):
    """Staged action of every droplet of (chip e, lock-step s): int64 (..., n) in [0, A)."""
    h = _key(PICK, e, s)
    return (h.unsqueeze(-1) >> (3 * torch.arange(n, device=h.device))) % A


def _buf(shape, dtype, off=0):
    """A device tensor whose data pointer is `off` bytes past an aligned allocation."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    return raw[off:off + nbytes].view(dtype).view(shape)


def _form(row, T, aligned):
    dw = row % 4 == 0 and aligned
    if not dw:
        return 'byte'
    return 'coop' if T * (row // 4) > COOP_MIN_WORDS else 'dword'


# id: (E, n, row bytes, T, form, term density, obs_term given, constraints f64, slots S, lock-steps, preset, options)
#   'dword': k_stream_step<uint32_t, false> (BENCH: 10x10, 4 droplets, fov 9 -> 980-byte rows, T = 40)
#   'coop':  k_stream_step<uint32_t, true> (T x row / 4 = 16 400 words, just over kCoopMinWords)
#   'byte':  k_stream_step<int8_t, true> (row % 4 != 0, or a 4-byte row behind a misaligned pointer)
CASES = {
    'e1_dword':              (1, 4, 980, 40, 'dword', 0.05, True, False, 4, 90, True, {}),
    'e15_dword_forced_only': (15, 4, 980, 40, 'dword', 0.0, False, False, 15, 85, False, {}),
    'e16_coop':              (16, 4, 1640, 40, 'coop', 0.1, True, False, 16, 60, True, {}),
    'e16_coop_forced_only':  (16, 4, 1640, 40, 'coop', 0.0, False, True, 16, 45, False, {}),
    'e17_byte_f64':          (17, 1, 245, 40, 'byte', 0.1, False, True, 17, 60, True, {}),
    'e17_dword_all_close':   (17, 4, 980, 40, 'dword', 1.0, True, False, 17, 6, True, {}),
    'e4095_dword':           (4095, 4, 980, 40, 'dword', 0.02, True, False, 4095, 20, True, {}),
    'e4096_coop_all_close':  (4096, 4, 1640, 40, 'coop', 1.0, False, True, 4096, 4, True, {}),
    'e4096_byte':            (4096, 1, 245, 40, 'byte', 0.05, True, False, 4096, 10, True, {'anneal': 0.0}),
    'e4097_dword_all_close': (4097, 4, 980, 40, 'dword', 1.0, True, False, 4097, 4, True, {}),
    'e4097_coop':            (4097, 4, 1640, 40, 'coop', 0.02, True, True, 3 * 4097 + 5, 16, True, {}),
    'e8193_dword_term_off':  (8193, 4, 980, 40, 'dword', 0.05, False, False, 8193, 10, True, {'term_off': 3}),
    'e8193_coop':            (8193, 4, 1640, 40, 'coop', 0.05, True, False, 8193, 10, True, {'term_off': 5}),
    'e8193_misaligned_byte': (8193, 4, 980, 40, 'byte', 0.05, True, True, 8193, 8, True, {'obs_off': 1}),
    'e32768_dword':          (32768, 4, 980, 40, 'dword', 0.01, True, False, 32768, 5, True, {'eps0': 0.1}),   # epsilon clamps
    'e32768_coop_all_close': (32768, 4, 1640, 40, 'coop', 1.0, False, True, 32768, 3, True, {}),
    'e32768_coop_sparse':    (32768, 4, 1640, 40, 'coop', 0.003, True, False, 32768, 4, True, {'term_off': 1}),
}


@pytest.mark.parametrize('case', list(CASES))
def test_stream_step_matches_host_restatement(case):
    E, n, row, T, form, dens, with_term, f64, S, L, preset, opt = CASES[case]
    A, H = 5, 24
    obs_off, term_off = opt.get('obs_off', 0), opt.get('term_off', 0)
    assert _form(row, T, obs_off % 4 == 0) == form
    assert S >= E and E <= _lib.ROLLOUT_STREAM_MAX_ENVS
    lib = _lib.rollout_ops()
    rng = np.random.default_rng(E * 1009 + row)
    dev = torch.device(DEV)
    chips = torch.arange(E, device=dev)
    tt = torch.arange(T, device=dev)

    # ---- per (lock-step, chip) scalars for lock-steps -T .. L-1 (row s + T): the pre-staged part and the played part
    R = rng.normal(0.0, 3.0, (T + L, E)) * rng.choice([1.0, 1e-3, 7.0], (T + L, E))
    CONS = (rng.random((T + L, E)) * 5.0) if f64 else rng.integers(0, 6, (T + L, E)).astype(np.int32)
    SU = (rng.random((T + L, E)) < 0.04).astype(np.uint8)
    R_dev = torch.as_tensor(R, device=dev)

    # ---- device buffers (rollout_stage, rollout_ring) and the host model
    t0 = rng.integers(0, T, E) if preset else np.zeros(E, np.int64)
    st_t_ep = torch.zeros((2, E), dtype=torch.int32, device=dev)
    st_t_ep[0] = torch.as_tensor(t0, device=dev)
    st_o0 = torch.empty((E, row), dtype=torch.uint8, device=dev)
    st_o_next = torch.full((E, T, row), 0xEE, dtype=torch.uint8, device=dev)
    st_u = torch.zeros((E, T, n), dtype=torch.int8, device=dev)
    st_oh = torch.zeros((E, T, n, A), dtype=torch.int8, device=dev)
    st_r = torch.zeros((E, T), dtype=torch.float32, device=dev)
    st_acc = torch.zeros((E, 3), dtype=torch.float64, device=dev)
    st_chip = torch.zeros((E, 4), dtype=torch.int64, device=dev)
    st_close = torch.full((E,), 123, dtype=torch.int32, device=dev)
    st_alt = torch.zeros(4, dtype=torch.int64, device=dev)
    start = -t0.astype(np.int64)        # lock-step in which the running episode of each chip began
    start_dev = torch.as_tensor(start, device=dev)
    chunk = max(1, (1 << 27) // (T * row))
    for c0 in range(0, E, chunk):       # pre-stage the first t0[e] steps of each running episode
        e = chips[c0:c0 + chunk]
        s_ = start_dev[c0:c0 + chunk, None] + tt
        live = (tt < torch.as_tensor(t0[c0:c0 + chunk], device=dev)[:, None])
        st_o0[c0:c0 + chunk] = _rows(PREV, e, start_dev[c0:c0 + chunk], row)
        st_o_next[c0:c0 + chunk] = torch.where(live[..., None], _rows(NEW, e[:, None], s_, row), st_o_next[c0:c0 + chunk])
        u = _picks(e[:, None], s_, n, A)
        st_u[c0:c0 + chunk] = torch.where(live[..., None], u, 0).to(torch.int8)
        st_oh[c0:c0 + chunk] = (torch.nn.functional.one_hot(u, A) * live[..., None, None]).to(torch.int8)
        st_r[c0:c0 + chunk] = torch.where(live, R_dev[(s_ + T).clamp(0, T + L - 1), e[:, None]].float(), 0.0)
    acc = np.zeros((E, 3))              # running (reward, constraints, success), summed step by step as the kernel does
    for s in range(-T, 0):
        m = s >= start
        acc[m, 0] = acc[m, 0] + R[s + T][m]
        acc[m, 1] = acc[m, 1] + CONS[s + T][m].astype(np.float64)
        acc[m, 2] = acc[m, 2] + SU[s + T][m].astype(np.float64)
    st_acc.copy_(torch.as_tensor(acc, device=dev))
    t_host = t0.astype(np.int64).copy()
    chip_acc = np.zeros((E, 4), np.int64)

    ring = {'o': _buf((S, T, row), torch.uint8, 2 * obs_off), 'o_next': _buf((S, T, row), torch.uint8),
            'u': torch.empty((S, T, n), dtype=torch.int8, device=dev), 'u_onehot': torch.empty((S, T, n, A), dtype=torch.int8, device=dev),
            'avail_u': torch.empty((S, T, n, A), dtype=torch.int8, device=dev), 'avail_u_next': torch.empty((S, T, n, A), dtype=torch.int8, device=dev),
            'r': torch.empty((S, T), dtype=torch.float32, device=dev), 'padded': torch.empty((S, T), dtype=torch.uint8, device=dev),
            'terminated': torch.empty((S, T), dtype=torch.uint8, device=dev)}
    for v in ring.values():
        v.view(torch.uint8).fill_(0xA5)
    ring_len = torch.zeros(S, dtype=torch.int32, device=dev)
    ring_stats = torch.zeros((S, 4), dtype=torch.float64, device=dev)
    cursor, size, total = max(0, S - 3), max(0, S - 2 * E), 1000      # the cursor wraps in the first lock-step that closes 3+
    ring_state = torch.tensor([cursor, size, total, 77], dtype=torch.int64, device=dev)
    len_host, stats_host = np.zeros(S, np.int32), np.zeros((S, 4))
    eps = np.float32(opt.get('eps0', 0.9))
    anneal, min_eps = np.float32(opt.get('anneal', 2.5e-6)), np.float32(0.05)
    eps_dev = torch.tensor([eps], device=dev)
    draw = M32 - 1                                                    # wraps after two lock-steps
    draw_dev = torch.tensor([draw - (1 << 32)], dtype=torch.int32, device=dev)   # uint32 on the device

    stage = _lib.RolloutStage(st_t_ep.data_ptr(), st_o0.data_ptr(), st_o_next.data_ptr(), st_u.data_ptr(), st_oh.data_ptr(),
                              st_r.data_ptr(), st_acc.data_ptr(), st_chip.data_ptr(), st_close.data_ptr(), st_alt.data_ptr())
    rs = _lib.RolloutRing(S, ring['o'].data_ptr(), ring['o_next'].data_ptr(), ring['u'].data_ptr(), ring['u_onehot'].data_ptr(),
                          ring['avail_u'].data_ptr(), ring['avail_u_next'].data_ptr(), ring['r'].data_ptr(), ring['padded'].data_ptr(),
                          ring['terminated'].data_ptr(), ring_len.data_ptr(), ring_stats.data_ptr(), ring_state.data_ptr())
    obs_prev, obs_new = _buf((E, row), torch.uint8, obs_off), _buf((E, row), torch.uint8, obs_off)
    obs_term = _buf((E, row), torch.uint8, obs_off) if with_term else None
    term = _buf((E,), torch.uint8, term_off)
    hidden = torch.empty((E * n, H), dtype=torch.float32, device=dev)
    last_oh = torch.empty((E * n, A), dtype=torch.int8, device=dev)
    cons_dev = torch.empty(E, dtype=torch.float64 if f64 else torch.int32, device=dev)
    succ_dev = torch.empty(E, dtype=torch.uint8, device=dev)
    tr_dev = torch.empty(E, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    closes = 0

    for s in range(L):
        p = s & 1
        tm = (rng.random(E) < dens) | (t_host == T - 1)
        # inputs of lock-step s; the picks are staged at each chip's own step (rollout_gru_head_select_stream does that)
        term.copy_(torch.as_tensor(tm.astype(np.uint8), device=dev))
        tr_dev.copy_(R_dev[s + T])
        cons_dev.copy_(torch.as_tensor(CONS[s + T], device=dev))
        succ_dev.copy_(torch.as_tensor(SU[s + T], device=dev))
        obs_prev.copy_(_rows(PREV, chips, s, row))
        obs_new.copy_(_rows(NEW, chips, s, row))
        if with_term:
            obs_term.copy_(_rows(TERM, chips, s, row))
        t_dev = torch.as_tensor(t_host, device=dev)
        u = _picks(chips, s, n, A)
        st_u[chips, t_dev] = u.to(torch.int8)
        st_oh[chips, t_dev] = torch.nn.functional.one_hot(u, A).to(torch.int8)
        hidden.fill_(s + 1.5)
        last_oh.fill_(1)
        rc = lib.rollout_stream_step(E, n, A, T, row, H, obs_prev.data_ptr(), obs_new.data_ptr(),
                                     obs_term.data_ptr() if with_term else None, term.data_ptr(), tr_dev.data_ptr(),
                                     cons_dev.data_ptr(), int(f64), succ_dev.data_ptr(), C.byref(stage), C.byref(rs), p,
                                     hidden.data_ptr(), last_oh.data_ptr(), eps_dev.data_ptr(), float(anneal), float(min_eps),
                                     draw_dev.data_ptr(), stream)
        assert rc == 0

        # ---- the host model of the contract
        ln = t_host + 1
        rew = acc[:, 0] + R[s + T]
        cons = acc[:, 1] + CONS[s + T].astype(np.float64)
        succ = acc[:, 2] + SU[s + T].astype(np.float64)
        who = np.nonzero(tm)[0]                                   # closers in ascending chip order
        slots = (cursor + np.arange(len(who))) % S
        infl = np.where(succ > 0, ln, T)
        len_host[slots] = ln[who]
        stats_host[slots] = np.stack([rew[who], infl[who].astype(np.float64), cons[who], succ[who]], 1)
        chip_acc[:, 0] += tm
        chip_acc[:, 1] += np.where(tm, infl, 0)
        chip_acc[:, 2] += tm & (succ > 0)
        chip_acc[:, 3] += 1
        acc = np.where(tm[:, None], 0.0, np.stack([rew, cons, succ], 1))
        close_slot = np.full(E, -1, np.int32)
        close_slot[who] = slots
        closed = [(slots, who, start[who], ln[who])]
        t_prev = t_host
        t_host = np.where(tm, 0, t_host + 1)
        start = np.where(tm, s + 1, start)
        state_in = np.array([cursor, size, total, 77])
        cursor, size, total = (cursor + len(who)) % S, min(S, size + len(who)), total + len(who)
        if anneal > 0:
            eps = np.maximum(np.float32(eps - np.float32(anneal * np.float32(E))), min_eps)
        draw = (draw + 1) & M32
        closes += len(who)

        # ---- the device state, in one transfer
        out, keep = (st_alt, ring_state) if p == 0 else (ring_state, st_alt)
        got = [v.cpu().numpy() for v in (st_t_ep, st_close, st_acc, st_chip, out, keep, eps_dev, draw_dev, ring_len, ring_stats)]
        np.testing.assert_array_equal(got[0][1 - p], t_host, err_msg='t_ep written at lock-step %d' % s)
        np.testing.assert_array_equal(got[0][p], t_prev, err_msg='t_ep read row changed at lock-step %d' % s)
        np.testing.assert_array_equal(got[1], close_slot, err_msg='close_slot at lock-step %d' % s)
        np.testing.assert_array_equal(got[2].view(np.int64), acc.view(np.int64), err_msg='ep_acc at lock-step %d' % s)
        np.testing.assert_array_equal(got[3], chip_acc, err_msg='chip_acc at lock-step %d' % s)
        np.testing.assert_array_equal(got[4], [cursor, size, total, 77], err_msg='ring state at lock-step %d' % s)
        np.testing.assert_array_equal(got[5], state_in, err_msg='ring state read buffer at lock-step %d' % s)
        assert got[6].view(np.uint32)[0] == np.float32(eps).view(np.uint32), (s, got[6][0], eps)
        assert int(got[7][0]) & M32 == draw
        np.testing.assert_array_equal(got[8], len_host, err_msg='ring len at lock-step %d' % s)
        np.testing.assert_array_equal(got[9].view(np.int64), stats_host.view(np.int64), err_msg='ring stats at lock-step %d' % s)
        tm_dev = torch.as_tensor(tm, device=dev).repeat_interleave(n)[:, None]
        assert torch.equal(hidden, torch.where(tm_dev, 0.0, s + 1.5).expand(-1, H)), 'hidden at lock-step %d' % s
        assert torch.equal(last_oh, torch.where(tm_dev, 0, 1).to(torch.int8).expand(-1, A)), 'last_onehot at lock-step %d' % s
        _check_ring(ring, closed, T, L, row, n, A, R_dev, with_term, s)
    assert closes > 0 and (dens < 1.0 or closes == E * L)


def _check_ring(ring, closed, T, L, row, n, A, R_dev, with_term, s_close):
    """The ring rows of the episodes closed in lock-step s_close, rebuilt from the hashes (rollout.py:131-141 padding)."""
    slots, who, start, ln = closed[0]
    if len(who) == 0:
        return
    dev = R_dev.device
    tt = torch.arange(T, device=dev)
    chunk = max(1, (1 << 27) // (T * row))
    for c0 in range(0, len(who), chunk):
        sl = torch.as_tensor(slots[c0:c0 + chunk], device=dev)
        e = torch.as_tensor(who[c0:c0 + chunk], device=dev)
        s0 = torch.as_tensor(start[c0:c0 + chunk], device=dev)
        le = torch.as_tensor(ln[c0:c0 + chunk], device=dev)
        assert torch.equal(s0 + le - 1, torch.full_like(s0, s_close))
        s_ = s0[:, None] + tt
        valid = tt < le[:, None]
        on = _rows(NEW, e[:, None], s_, row)
        if with_term:    # the row of the closing step is the terminal observation
            on[torch.arange(len(e), device=dev), le - 1] = _rows(TERM, e, s0 + le - 1, row)
        on *= valid[..., None]
        o = torch.zeros_like(on)
        o[:, 0] = _rows(PREV, e, s0, row)
        o[:, 1:] = on[:, :-1]
        o *= valid[..., None]
        what = 'lock-step %d, slots %s..' % (s_close, slots[c0:c0 + 3])
        assert torch.equal(ring['o_next'][sl], on), 'o_next, ' + what
        assert torch.equal(ring['o'][sl], o), 'o, ' + what
        u = _picks(e[:, None], s_, n, A) * valid[..., None]
        assert torch.equal(ring['u'][sl], u.to(torch.int8)), 'u, ' + what
        oh = torch.nn.functional.one_hot(u, A) * valid[..., None, None]
        assert torch.equal(ring['u_onehot'][sl], oh.to(torch.int8)), 'u_onehot, ' + what
        av = valid[..., None, None].expand(-1, -1, n, A).to(torch.int8)
        assert torch.equal(ring['avail_u'][sl], av) and torch.equal(ring['avail_u_next'][sl], av), 'avail, ' + what
        r = torch.where(valid, R_dev[(s_ + T).clamp(0, T + L - 1), e[:, None]].float(), 0.0)
        assert torch.equal(ring['r'][sl].view(torch.int32), r.view(torch.int32)), 'r, ' + what
        assert torch.equal(ring['padded'][sl], (tt >= le[:, None]).to(torch.uint8)), 'padded, ' + what
        assert torch.equal(ring['terminated'][sl], (tt >= le[:, None] - 1).to(torch.uint8)), 'terminated, ' + what
