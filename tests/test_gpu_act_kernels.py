"""The rollout's pick kernels (csrc/rollout_ops.hip: k_select, k_gru_head_select with its live and stream paths, k_post,
k_obs_append) through their C ABI (include/rollout_ops.h), row by row against the host restatement of tests/act_kernel_cases.py:

  values        h' and q of the fused kernel against float64 at 1, 7, 8, 9, 15, 16, 17 and 4099 rows (8 rows per workgroup) and
                A = 1, 2, 5, 9, 16, with the project's own tolerances (h 1e-6, q 1e-5 absolute; 2e-5 on h with saturated gates);
                two runs give the same bits, and so does a run without d_q
  greedy pick   the first maximum of the kernel's own q, the float64 argmax on every row that is no near tie (at most 1 % are:
                tests/test_act_kernel_cases.py asserts that for the same inputs), exact ties won by the lower index
  exploration   every entry point against the documented Philox draw: draws 0, 7 and 2^32 - 1, a seed with two different halves,
                epsilon 0, 1, interior, and exactly one row's U1 (that row stays greedy: the comparison is strict)
  outputs       every buffer sits between guard regions (front_kernel_cases.guarded) and starts out filled with a sentinel: what
                the contract does not name keeps it -- other slots of the episode tensors, rows of finished chips, everything
                when an argument is refused
  live, stream  against the references, not against the full kernel alone: compact x-side rows with NaN behind them, picks keyed
                by the chip-order row; every chip's pick staged at its own step
  post step     the last step of an episode (no o row is written), 1 to 513 chips, dword and byte observation rows, epsilon's
                clamp, the minimal set of outputs, the workspace across three calls
  arguments     each refusal of the wrappers, one bad argument at a time among otherwise valid buffers.

Largest deviation from float64 on an MI355X (over the value cases below; the tolerances were not derived from these):
h 2.64e-07 and q 1.59e-07 at unit scale (4099 rows x 16 actions); h 1.22e-06 with saturated gates."""
import types

import numpy as np
import pytest
import torch

import act_kernel_cases as K
from front_kernel_cases import guarded

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENT_F = -777.125          # float outputs
SENT_I = -7                # actions
SENT_B = -99               # int8 outputs: no action index and no one-hot entry
OK, BAD_ARG = 0, -1

HEAD = ['ig', 'hg', 'b_ih', 'b_hh', 'h', 'fc_w', 'fc_b', 'n_envs', 'n_agents', 'hidden', 'n_actions', 'eps', 'evaluate', 'seed', 'draw',
        'actions', 'last', 'ep_u', 'ep_oh', 'T']
ARGS = {'select': ['q', 'n_envs', 'n_agents', 'n_actions', 'eps', 'evaluate', 'seed', 'draw', 'actions', 'last', 'ep_u', 'ep_oh', 'T', 't',
                   'stream'],
        'full': HEAD + ['t', 'q', 'stream'],
        'live': HEAD + ['t', 'q', 'lst', 'cnt', 'stream'],
        'stream': HEAD + ['t_ep', 'q', 'stream'],
        'post': ['n_envs', 'T', 't', 'alive', 'term', 'tr', 'cons', 'f64', 'succ', 'ep_r', 'ep_pad', 'ep_term', 'sum_r', 'sum_c', 'sum_s',
                 'steps', 'eps', 'anneal', 'min_eps', 'ws', 'draw', 'obs', 'row', 'ep_o', 'ep_on', 'stream']}
FN = {'select': 'rollout_select_actions', 'full': 'rollout_gru_head_select', 'live': 'rollout_gru_head_select_live',
      'stream': 'rollout_gru_head_select_stream', 'post': 'rollout_post_step'}


def _lib():
    from marl_dmfb_amd import _lib
    return _lib.rollout_ops()


def _call(entry, v):
    args = [x.data_ptr() if torch.is_tensor(x) else x for x in (v[k] for k in ARGS[entry])]
    return getattr(_lib(), FN[entry])(*args)


def _put(d, a, offset=0):
    """A copy of numpy array `a` on the GPU between guard regions."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    v, chk = guarded(tuple(t.shape), t.dtype, 0, DEV, offset)
    v.copy_(t)
    d.checks.append(chk)
    return v


def _out(d, shape, dtype, fill):
    v, chk = guarded(tuple(shape), dtype, fill, DEV)
    d.checks.append(chk)
    return v


def _u32(x):
    return np.array([x], dtype=np.uint32).view(np.int32)


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(a, b, names):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        assert x is None or np.array_equal(_bits(x), _bits(y)), name


def _inputs(rows, A, seed=0):
    """The input set of a comparison with float64: one of those whose near ties the CPU test has counted."""
    assert (rows, A, seed, 1.0) in K.TOLERANCE_SETS
    return K.make_inputs(rows, A, seed)


def _live(E, kind, seed=1):
    """The live list of `kind` through rollout_compact_alive -> namespace(lst, cnt, chips, k); the unused tail of the list holds
    chip 0 (a valid id: nothing may read it, and a kernel that did would not leave the buffers)."""
    alive = np.zeros(E, dtype=np.uint8)
    if kind == 'all':
        alive[:] = 1
    elif kind == 'first':
        alive[0] = 1
    elif kind == 'last':
        alive[E - 1] = 1
    elif kind == 'half':
        alive[:] = np.random.default_rng(seed).random(E) < 0.5
        alive[0], alive[E - 1] = 0, 1
    d = types.SimpleNamespace(checks=[])
    a = _put(d, alive)
    lv = types.SimpleNamespace(lst=_out(d, (E,), torch.int32, 0), cnt=_out(d, (1,), torch.int32, -1))
    assert _lib().rollout_compact_alive(E, a.data_ptr(), lv.lst.data_ptr(), lv.cnt.data_ptr(), None) == OK
    torch.cuda.synchronize()
    for chk in d.checks:
        chk()
    lv.chips = np.flatnonzero(alive)
    lv.k = len(lv.chips)
    assert int(lv.cnt[0]) == lv.k and np.array_equal(lv.lst.cpu().numpy()[:lv.k], lv.chips) and not bool(lv.lst[lv.k:].any())
    return lv


def _rows_of(chips, n):
    return (np.asarray(chips)[:, None] * n + np.arange(n)[None, :]).reshape(-1)


def _run(entry, c, E, n, *, evaluate=1, eps=None, draw=None, seed=K.SEED, T=3, t=0, want_q=True, ep='both', live=None, t_ep=None,
         q_in=None):
    """One call of an entry point on fresh, sentinel-filled buffers -> CPU numpy outputs (None where no buffer was given).  Checks
    the return code, every guard region and that no input changed."""
    A = q_in.shape[1] if entry == 'select' else c.A
    R = E * n
    d = types.SimpleNamespace(checks=[])
    v = dict(n_envs=E, n_agents=n, hidden=K.H, n_actions=A, evaluate=evaluate, seed=seed, T=T, t=t, stream=None)
    if entry == 'select':
        ins = dict(q=q_in)
    else:
        ig = c.ig
        if entry == 'live':   # compact: row k * n + a belongs to chip live.chips[k]; NaN behind the live rows
            ig = np.full_like(c.ig, np.nan)
            ig[:live.k * n] = c.ig[_rows_of(live.chips, n)]
        ins = dict(ig=ig, hg=c.hg, b_ih=c.b_ih, b_hh=c.b_hh, fc_w=c.fc_w, fc_b=c.fc_b)
    if eps is not None:
        ins['eps'] = np.float32([eps])
    if draw is not None:
        ins['draw'] = _u32(draw)
    if entry == 'stream':
        ins['t_ep'] = np.asarray(t_ep, dtype=np.int32)
    v.update(eps=None, draw=None)
    for k, a in ins.items():
        v[k] = _put(d, a)
    if entry != 'select':
        v['h'] = _put(d, c.h)
        v['q'] = _out(d, (R, A), torch.float32, SENT_F) if want_q else None
    v['actions'] = _out(d, (R,), torch.int32, SENT_I)
    v['last'] = _out(d, (R, A), torch.int8, SENT_B)
    v['ep_u'] = _out(d, (E, T, n), torch.int8, SENT_B) if ep in ('both', 'u') else None
    v['ep_oh'] = _out(d, (E, T, n, A), torch.int8, SENT_B) if ep == 'both' else None
    if entry == 'live':
        v['lst'], v['cnt'] = live.lst, live.cnt
    assert _call(entry, v) == OK
    torch.cuda.synchronize()
    for chk in d.checks:
        chk()
    for k, a in ins.items():
        assert np.array_equal(_bits(v[k].cpu().numpy()), _bits(a)), ('an input was written', k)
    o = types.SimpleNamespace()
    for k in ('actions', 'last', 'ep_u', 'ep_oh', 'h', 'q'):
        x = v.get(k)
        setattr(o, k, x.cpu().numpy() if torch.is_tensor(x) else None)
    if entry == 'select':
        o.q = q_in
    return o


def _check_picks(o, E, n, A, T, t, want, rows=None):
    """actions, last_onehot and slot t (one step, or one per chip) of the episode tensors hold the picks `want` in the rows `rows`
    (default: all of them) and their sentinel everywhere else."""
    R = E * n
    written = np.zeros(R, dtype=bool)
    written[slice(None) if rows is None else rows] = True
    want = np.asarray(want)
    assert np.array_equal(o.actions, np.where(written, want, SENT_I))
    assert np.array_equal(o.last, np.where(written[:, None], K.onehots(want, A), SENT_B))
    u, oh = K.episode_slots(want, E, n, A, T, t, SENT_B, rows=np.flatnonzero(written))
    assert o.ep_u is None or np.array_equal(o.ep_u, u)
    assert o.ep_oh is None or np.array_equal(o.ep_oh, oh)


def _rand_picks(seed, draw, rows, A):
    return ((K.draw_words(seed, draw, rows)[:, 1] * np.uint64(A)) >> np.uint64(32)).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------------------
# values and the greedy pick
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('A', K.ACTIONS)
@pytest.mark.parametrize('E,n', K.ROW_SHAPES)
def test_fused_values_and_greedy_pick(E, n, A):
    c = _inputs(E * n, A)
    h64, q64 = K.reference(c)
    T, t = 3, 2
    o = _run('full', c, E, n, T=T, t=t)
    dev_h, dev_q = float(np.abs(o.h - h64).max()), float(np.abs(o.q - q64).max())
    print('deviation from float64, %d rows x %d actions: h %.3e q %.3e' % (E * n, A, dev_h, dev_q))
    assert dev_h <= K.H_TOL and dev_q <= K.Q_TOL, (dev_h, dev_q)
    _check_picks(o, E, n, A, T, t, K.first_max(o.q))                   # the first maximum of the kernel's own q, exactly
    clear = K.top2_gap(q64) > K.GAP
    assert float((~clear).mean()) <= K.MAX_TIE_ROWS
    assert np.array_equal(o.actions[clear], K.first_max(q64)[clear])
    _same_bits(o, _run('full', c, E, n, T=T, t=t), ('h', 'q', 'actions', 'last', 'ep_u', 'ep_oh'))
    _same_bits(o, _run('full', c, E, n, T=T, t=t, want_q=False), ('h', 'actions', 'last', 'ep_u', 'ep_oh'))


@pytest.mark.parametrize('spikes', [False, True])
def test_fused_saturated_gates_stay_finite_and_accurate(spikes):
    """ig, hg * 8 (gates deep in saturation) and additionally 48 entries of ig at +-1e4, where expf(-x) of the sigmoid overflows
    to inf: 43 x 3 rows, ragged.  Tolerance and reasoning of test_gru_packed_saturated_gates_stay_finite_and_accurate."""
    E, n, A = 43, 3, 5
    c = K.make_inputs(E * n, A, seed=8, scale=8.0)
    if spikes:
        K.spike(c)
    h64, q64 = K.gru_head_reference(c.ig, c.hg, c.b_ih, c.b_hh, c.h, c.fc_w, c.fc_b)
    assert np.isfinite(h64).all() and np.isfinite(q64).all()
    o = _run('full', c, E, n)
    assert np.isfinite(o.h).all() and np.isfinite(o.q).all()
    dev_h = float(np.abs(o.h - h64).max())
    print('deviation from float64, saturated gates, spikes %s: h %.3e q %.3e' % (spikes, dev_h, float(np.abs(o.q - q64).max())))
    assert dev_h <= K.SAT_TOL
    _check_picks(o, E, n, A, 3, 0, K.first_max(o.q))


def test_select_greedy_takes_the_first_of_equal_maxima():
    E, n, A = 5, 3, 7
    q = np.random.default_rng(2).standard_normal((E * n, A)).astype(np.float32)
    want = K.first_max(q)
    q[0] = 0.25
    q[1, 2] = q[1, 5] = 9.0
    q[2, 6] = q[2, 0] = 9.0
    q[3, 5] = q[3, 6] = 9.0
    q[4] = -1.0
    q[4, 3], q[4, 4] = -0.0, 0.0                     # equal: the first, whichever sign it carries
    q[5] = -1.0
    q[5, 1], q[5, 6] = 0.0, -0.0
    q[6, :] = -np.float32(3.5)
    q[7, 1:] = q[7, 0] - np.float32(1.0)
    q[7, 4] = q[7, 0]
    want[:8] = [0, 2, 0, 5, 3, 1, 0, 0]
    assert np.array_equal(K.first_max(q), want)
    o = _run('select', None, E, n, q_in=q, T=2, t=1)
    _check_picks(o, E, n, A, 2, 1, want)
    assert np.array_equal(o.actions, np.argmax(q.astype(np.float64), axis=1))


@pytest.mark.parametrize('A,same', [(5, (1, 3)), (9, (0, 8)), (16, tuple(range(16)))])
def test_fused_duplicated_head_rows_tie_bit_for_bit(A, same):
    """Rows `same` of fc_w and their fc_b entries are one and the same: those actions' Q values come out of the same operations
    in the same order, so they are equal bit for bit and the lowest index wins every tie."""
    E, n = 37, 3
    c = K.make_inputs(E * n, A, seed=4)
    c.fc_w[list(same)] = c.fc_w[same[0]]
    c.fc_b[list(same)] = c.fc_b[same[0]]
    o = _run('full', c, E, n)
    for k in same[1:]:
        assert np.array_equal(o.q[:, k].view(np.int32), o.q[:, same[0]].view(np.int32))
        assert not bool((o.actions == k).any())
    q64 = K.gru_head_reference(c.ig, c.hg, c.b_ih, c.b_hh, c.h, c.fc_w, c.fc_b)[1]
    tied = np.isin(np.argmax(q64, axis=1), same) & (K.top2_gap(np.delete(q64, same[1:], axis=1)) > K.GAP)
    assert int(tied.sum()) >= 5, 'too few rows whose maximum is the duplicated action'
    assert bool((o.actions[tied] == same[0]).all())
    _check_picks(o, E, n, A, 3, 0, K.first_max(o.q))


# ------------------------------------------------------------------------------------------------------------------------------
# the exploring pick against Philox
# ------------------------------------------------------------------------------------------------------------------------------
EXPLORE = [('select', 5), ('select', 127)] + [(e, A) for e in ('full', 'live', 'stream') for A in (1, 5, 9, 16)]


@pytest.mark.parametrize('entry,A', EXPLORE, ids=['%s_A%d' % x for x in EXPLORE])
def test_exploring_pick_is_the_documented_philox_draw(entry, A):
    E, n, T = 37, 3, 4
    R = E * n                                          # 111 rows: 13 full workgroups of the fused kernel and one with 7 rows
    c = K.make_inputs(R, A, seed=5)
    q_in = np.random.default_rng(A).standard_normal((R, A)).astype(np.float32) if entry == 'select' else None
    live = _live(E, 'half') if entry == 'live' else None
    rows = _rows_of(live.chips, n) if live else np.arange(R)
    t = np.arange(E) % T if entry == 'stream' else T - 1
    kw = dict(T=T, t=0 if entry == 'stream' else t, t_ep=t, live=live, q_in=q_in)
    base = _run(entry, c, E, n, **kw)                  # greedy: the Q values that every exploring run must reproduce
    greedy = K.first_max(base.q)
    _check_picks(base, E, n, A, T, t, greedy, rows)
    for draw in K.DRAWS:
        u1 = K.draw_u1(K.SEED, draw, np.arange(R))
        rand = _rand_picks(K.SEED, draw, np.arange(R), A)
        assert rand.min() >= 0 and rand.max() < A
        # the row whose U1 becomes epsilon: a middle one of those whose random pick differs from its greedy one
        cand = [r for r in rows if rand[r] != greedy[r]] or list(rows)
        k = sorted(cand, key=lambda r: u1[r])[len(cand) // 2]
        for eps in (0.0, 1.0, 0.37, float(u1[k])):
            o = _run(entry, c, E, n, evaluate=0, eps=eps, draw=draw, **kw)
            if entry != 'select':
                _same_bits(o, base, ('h', 'q'))
            want, u1_ref = K.pick_reference(o.q, K.SEED, draw, eps, 0, np.arange(R))
            assert np.array_equal(u1_ref, u1)
            _check_picks(o, E, n, A, T, t, want, rows)
            got = o.actions[rows]
            assert got.min() >= 0 and got.max() < A
            if eps == 0.0:
                assert np.array_equal(got, greedy[rows])
            elif eps == 1.0:
                assert np.array_equal(got, rand[rows])
            elif eps == float(u1[k]):
                below = rows[u1[rows] < u1[k]]
                assert len(below) > 0 and np.array_equal(o.actions[below], rand[below])
                assert o.actions[k] == greedy[k], 'U1 == epsilon must stay greedy'
            else:
                n_rand = int((u1[rows] < np.float32(eps)).sum())
                assert 0 < n_rand < len(rows)
    if A == 1:
        assert not bool(o.actions[rows].any())
    # the two halves of the seed are not interchangeable
    swapped = ((K.SEED & 0xffffffff) << 32) | (K.SEED >> 32)
    o = _run(entry, c, E, n, evaluate=0, eps=1.0, draw=7, seed=swapped, **kw)
    _check_picks(o, E, n, A, T, t, K.pick_reference(o.q, swapped, 7, 1.0, 0, np.arange(R))[0], rows)
    assert A == 1 or not np.array_equal(o.actions[rows], _rand_picks(K.SEED, 7, rows, A))


def test_select_row_ids_wider_than_sixteen_bits():
    E, n, A, T, t = 21846, 3, 5, 2, 1
    R = E * n
    assert R > 65536
    q = np.random.default_rng(11).standard_normal((R, A)).astype(np.float32)
    o = _run('select', None, E, n, q_in=q, evaluate=0, eps=0.5, draw=7, T=T, t=t)
    want, u1 = K.pick_reference(q, K.SEED, 7, 0.5, 0, np.arange(R))
    assert 0.45 * R < int((u1 < 0.5).sum()) < 0.55 * R
    _check_picks(o, E, n, A, T, t, want)


@pytest.mark.parametrize('E,n,A', [(37, 3, 5), (5, 4, 9), (17, 1, 16), (9, 1, 1)])
def test_fused_kernel_is_select_on_its_own_q(E, n, A):
    c = K.make_inputs(E * n, A, seed=6)
    T, t = 5, 2
    for evaluate, eps in ((0, 0.4), (1, None)):
        f = _run('full', c, E, n, evaluate=evaluate, eps=eps, draw=7, T=T, t=t)
        s = _run('select', None, E, n, q_in=f.q, evaluate=evaluate, eps=eps, draw=7, T=T, t=t)
        _same_bits(f, s, ('actions', 'last', 'ep_u', 'ep_oh'))
        assert int((f.actions != K.first_max(f.q)).sum()) > 0 or evaluate or A == 1


# ------------------------------------------------------------------------------------------------------------------------------
# outputs
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ['select', 'full', 'live', 'stream'])
def test_first_and_last_slot_and_optional_outputs(entry):
    E, n, A, T = 5, 3, 5, 4
    R = E * n
    c = K.make_inputs(R, A, seed=7)
    q_in = np.random.default_rng(7).standard_normal((R, A)).astype(np.float32) if entry == 'select' else None
    live = _live(E, 'all') if entry == 'live' else None
    for t in (0, T - 1):
        for ep in ('both', 'u', None):
            if entry == 'stream' and ep is None:
                continue                                # d_stage_u is required there
            o = _run(entry, c, E, n, evaluate=0, eps=0.5, draw=7, T=T, t=0 if entry == 'stream' else t, t_ep=[t] * E, ep=ep,
                     live=live, q_in=q_in)
            assert (o.ep_u is None) == (ep is None) and (o.ep_oh is None) == (ep != 'both')
            _check_picks(o, E, n, A, T, t, K.pick_reference(o.q, K.SEED, 7, 0.5, 0, np.arange(R))[0])


# ------------------------------------------------------------------------------------------------------------------------------
# the live variant
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E,n,A,kind', K.LIVE_CASES, ids=['E%d_n%d_A%d_%s' % x for x in K.LIVE_CASES])
def test_live_variant_against_the_references(E, n, A, kind):
    R = E * n
    c = _inputs(R, A, K.LIVE_SEED)
    h64, q64 = K.reference(c)
    live = _live(E, kind)
    rows = _rows_of(live.chips, n)
    dead = np.ones(R, dtype=bool)
    dead[rows] = False
    T, t = 4, 1
    o = _run('live', c, E, n, evaluate=0, eps=0.5, draw=7, T=T, t=t, live=live)
    assert np.array_equal(o.h[dead].view(np.int32), c.h[dead].view(np.int32)), 'hidden state of a finished chip was written'
    assert bool((o.q[dead] == SENT_F).all())
    if len(rows):
        dev_h, dev_q = float(np.abs(o.h[rows] - h64[rows]).max()), float(np.abs(o.q[rows] - q64[rows]).max())
        print('deviation from float64, live %s, %d of %d rows: h %.3e q %.3e' % (kind, len(rows), R, dev_h, dev_q))
        assert dev_h <= K.H_TOL and dev_q <= K.Q_TOL, (dev_h, dev_q)
    want = K.pick_reference(o.q, K.SEED, 7, 0.5, 0, np.arange(R))[0]      # keyed by the chip-order row
    _check_picks(o, E, n, A, T, t, want, rows)
    if kind == 'half':   # the same chips among all chips: nothing of a row depends on who else is alive
        everyone = _run('live', c, E, n, evaluate=0, eps=0.5, draw=7, T=T, t=t, live=_live(E, 'all'))
        for name in ('h', 'q', 'actions', 'last'):
            assert np.array_equal(_bits(getattr(o, name))[rows], _bits(getattr(everyone, name))[rows]), name
        assert 0 < len(rows) < R
        assert int((want[rows] != K.first_max(o.q)[rows]).sum()) > 0.2 * len(rows)


# ------------------------------------------------------------------------------------------------------------------------------
# the stream variant
# ------------------------------------------------------------------------------------------------------------------------------
def test_stream_variant_stages_each_pick_at_its_chips_own_step():
    E, n, A, T = 37, 3, 5, 6
    R = E * n
    c = K.make_inputs(R, A, seed=9)
    t_ep = np.random.default_rng(9).integers(0, T, E)
    t_ep[[0, E - 2]] = 0
    t_ep[[1, E - 1]] = T - 1
    assert len(set(t_ep.tolist())) == T
    full = _run('full', c, E, n, evaluate=0, eps=0.4, draw=7, T=T, t=0, ep=None)
    assert int((full.actions != K.first_max(full.q)).sum()) > 0.2 * R
    for ep in ('both', 'u'):
        s = _run('stream', c, E, n, evaluate=0, eps=0.4, draw=7, T=T, t_ep=t_ep, ep=ep)
        _same_bits(s, full, ('h', 'q', 'actions', 'last'))
        assert (s.ep_oh is None) == (ep == 'u')
        _check_picks(s, E, n, A, T, t_ep, full.actions)


# ------------------------------------------------------------------------------------------------------------------------------
# rollout_post_step
# ------------------------------------------------------------------------------------------------------------------------------
POST_TENSORS = ['alive', 'term', 'tr', 'cons', 'succ', 'ep_r', 'ep_pad', 'ep_term', 'sum_r', 'sum_c', 'sum_s', 'steps', 'eps', 'ws', 'draw',
                'obs', 'ep_o', 'ep_on']


def _post_setup(E, T, row, *, f64=False, seed=0, obs_offset=0, episode=True, eps=0.75, draw=41, p_alive=0.7):
    """Valid arguments of rollout_post_step with random inputs and sentinel-filled episode tensors -> (values by name, checks)."""
    g = np.random.default_rng(1009 * seed + E)
    d = types.SimpleNamespace(checks=[])
    v = dict(n_envs=E, T=T, t=0, f64=int(f64), row=row, anneal=0.0, min_eps=0.0, stream=None)
    v['alive'] = _put(d, (g.random(E) < p_alive).astype(np.uint8))
    v['term'] = _put(d, (g.random(E) < 0.3).astype(np.uint8))
    v['tr'] = _put(d, g.standard_normal(E))
    cons = g.integers(0, 4, E).astype(np.int32)
    v['cons'] = _put(d, cons * 0.6 if f64 else cons)
    v['succ'] = _put(d, (g.random(E) < 0.2).astype(np.uint8))
    v['ep_r'] = _out(d, (E, T), torch.float32, SENT_F) if episode else None
    v['ep_pad'] = _out(d, (E, T), torch.uint8, 77) if episode else None
    v['ep_term'] = _out(d, (E, T), torch.uint8, 77) if episode else None
    v['sum_r'] = _put(d, g.standard_normal(E))
    v['sum_c'] = _put(d, g.standard_normal(E))
    v['sum_s'] = _put(d, g.integers(0, 5, E))
    v['steps'] = _put(d, g.integers(0, 50, E))
    v['eps'] = None if eps is None else _put(d, np.float32([eps]))
    v['ws'] = _put(d, np.zeros(4, dtype=np.int32))
    v['draw'] = None if draw is None else _put(d, _u32(draw))
    v['obs'] = _put(d, g.integers(-3, 9, (E, row)).astype(np.int8), obs_offset) if row else None
    v['ep_o'] = _out(d, (E, T, row), torch.int8, SENT_B) if row else None
    v['ep_on'] = _out(d, (E, T, row), torch.int8, SENT_B) if row else None
    return v, d.checks


def _snap(v):
    return {k: v[k].cpu().numpy().copy() for k in POST_TENSORS if torch.is_tensor(v[k])}


def _post_expect(b, v):
    """include/rollout_ops.h lines 68-80 applied to the snapshot `b` taken before the call."""
    T, t = v['T'], v['t']
    a = {k: x.copy() for k, x in b.items()}
    was, tm = b['alive'] != 0, b['term'] != 0
    if 'ep_r' in a:
        a['ep_r'][:, t] = b['tr'].astype(np.float32)
        a['ep_pad'][:, t] = ~was
        a['ep_term'][:, t] = tm
    a['sum_r'] = b['sum_r'] + b['tr']
    a['sum_c'] = b['sum_c'] + b['cons'].astype(np.float64)
    a['sum_s'] = b['sum_s'] + b['succ']
    a['steps'] = b['steps'] + was
    a['alive'] = (was & ~tm).astype(np.uint8)
    if v['anneal'] > 0:
        a['eps'] = np.maximum(b['eps'] - np.float32(v['anneal']) * np.float32(was.sum()), np.float32(v['min_eps'])).astype(np.float32)
    a['ws'] = np.array([int(a['alive'].sum()), 0, 0, 0], dtype=np.int32)
    if 'draw' in a:
        a['draw'] = (b['draw'].view(np.uint32) + np.uint32(1)).view(np.int32)
    if 'ep_on' in a:
        a['ep_on'][was, t] = b['obs'][was]
        if t + 1 < T:
            a['ep_o'][was & ~tm, t + 1] = b['obs'][was & ~tm]
    return a


def _post_call(v, checks):
    before = _snap(v)
    assert _call('post', v) == OK
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    after, want = _snap(v), _post_expect(before, v)
    for k in want:
        x, y = after[k], want[k]
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y), k
    return before, after


@pytest.mark.parametrize('row,offset,f64', [(8, 0, False), (7, 0, True), (8, 1, False), (980, 0, True)],
                         ids=['dwords', 'odd_length', 'odd_address', 'dmfb_row'])
@pytest.mark.parametrize('E', [1, 255, 256, 257, 513])
def test_post_step_first_and_last_step(E, row, offset, f64):
    """Every tensor after steps t = 0 and t = T - 1 against the header's rule, the observation rows through the dword path, the
    byte path of a row length that is no multiple of 4 and the byte path of an odd address.  At t = T - 1 no row of o is written:
    o[e][T] would be slot 0 of chip e + 1."""
    T = 3
    for t in (0, T - 1):
        v, checks = _post_setup(E, T, row, f64=f64, seed=t, obs_offset=offset)
        assert (v['obs'].data_ptr() % 4 != 0) == (offset == 1)
        v.update(t=t, anneal=2.0 ** -12, min_eps=0.05)
        before, after = _post_call(v, checks)
        if t == T - 1:
            assert bool((after['ep_o'] == SENT_B).all()), 'a row of o was written at the last step'
            alive = before['alive'] != 0
            assert np.array_equal(after['ep_on'][alive, t], before['obs'][alive])
        else:
            assert bool((after['ep_o'][:, 0] == SENT_B).all()) and bool((after['ep_o'][:, 2:] == SENT_B).all())
        assert E < 5 or 0 < int(after['ws'][0]) < int((before['alive'] != 0).sum())


def test_post_step_epsilon_anneals_clamps_and_stays():
    E, T = 257, 3
    for eps, anneal, min_eps, want in ((0.75, 2.0 ** -10, 0.05, None), (0.06, 2.0 ** -10, 0.05, np.float32(0.05)),
                                       (0.123456, 0.0, 0.5, np.float32(0.123456))):
        v, checks = _post_setup(E, T, 8, eps=eps)
        v.update(t=1, anneal=anneal, min_eps=min_eps)
        before, after = _post_call(v, checks)
        n_was = int((before['alive'] != 0).sum())
        assert 100 < n_was < E
        if want is None:                               # 0.75 - n / 1024: exact in float32 whether or not the product is fused
            want = np.float32(0.75 - n_was / 1024.0)
            assert float(want) == 0.75 - n_was / 1024.0
        assert after['eps'].view(np.int32)[0] == np.float32(want).view(np.int32)


def test_post_step_minimal_outputs():
    """No episode tensors, no draw counter, no epsilon, no observations: only the sums, steps, alive and n_alive change."""
    v, checks = _post_setup(513, 3, 0, episode=False, eps=None, draw=None)
    v.update(t=7)                                      # t is not looked at without episode tensors
    before, after = _post_call(v, checks)
    assert sorted(k for k in after if not np.array_equal(after[k], before[k])) == ['alive', 'steps', 'sum_c', 'sum_r', 'sum_s', 'ws']


def test_post_step_three_calls_on_one_workspace():
    E, T = 513, 4
    v, checks = _post_setup(E, T, 12, p_alive=0.95)
    v.update(anneal=2.0 ** -12, min_eps=0.05)
    g = np.random.default_rng(3)
    counts = []
    for t in range(3):
        v['t'] = t
        v['term'].copy_(torch.from_numpy((g.random(E) < 0.3).astype(np.uint8)))
        before, after = _post_call(v, checks)          # n_alive[1..3] back to zero, [0] right: part of the comparison
        counts.append(int(after['ws'][0]))
        moved = after['steps'] - before['steps']
        assert np.array_equal(moved, (before['alive'] != 0).astype(np.int64))
        assert int(after['draw'].view(np.uint32)[0]) == 42 + t
    assert E > counts[0] > counts[1] > counts[2] > 0


# ------------------------------------------------------------------------------------------------------------------------------
# the argument contract
# ------------------------------------------------------------------------------------------------------------------------------
CE, CN, CA, CT = 3, 2, 5, 4
CAP_A, CAP_H = 128, 256    # every buffer is large enough for any value a refused call carries, should a refusal ever fail


def _contract_values(entry):
    d = types.SimpleNamespace(checks=[])
    R = CE * CN
    f32, i8, i32 = torch.float32, torch.int8, torch.int32
    if entry == 'post':
        v, d.checks = _post_setup(CE, CT, 8)
        v.update(t=1, anneal=2.0 ** -10, min_eps=0.05)
        return v, d.checks
    v = dict(n_envs=CE, n_agents=CN, hidden=K.H, n_actions=CA, evaluate=0, seed=K.SEED, T=CT, t=1, stream=None)
    v['eps'], v['draw'] = _put(d, np.float32([0.5])), _put(d, _u32(7))
    v['actions'] = _out(d, (R,), i32, SENT_I)
    v['last'] = _out(d, (R * CAP_A,), i8, SENT_B)
    v['ep_u'] = _out(d, (CE * (CT + 1) * CN,), i8, SENT_B)
    v['ep_oh'] = _out(d, (CE * (CT + 1) * CN * CAP_A,), i8, SENT_B)
    v['q'] = _out(d, (R * CAP_A,), f32, 0.5)
    if entry != 'select':
        for k, size in (('ig', R * 3 * CAP_H), ('hg', R * 3 * CAP_H), ('b_ih', 3 * CAP_H), ('b_hh', 3 * CAP_H), ('h', R * CAP_H),
                        ('fc_w', CAP_A * CAP_H), ('fc_b', CAP_A)):
            v[k] = _out(d, (size,), f32, 0.125)
    if entry == 'live':
        v['lst'], v['cnt'] = _put(d, np.arange(CE, dtype=np.int32)), _put(d, np.int32([CE]))
    if entry == 'stream':
        v['t_ep'] = _put(d, np.zeros(CE, dtype=np.int32))
    return v, d.checks


def _bad_cases(entry):
    if entry == 'post':
        ptrs = ['alive', 'term', 'tr', 'cons', 'succ', 'sum_r', 'sum_c', 'sum_s', 'steps', 'ws']
        other = [dict(n_envs=-1), dict(eps=None), dict(t=CT), dict(t=-1), dict(row=0), dict(obs=None),
                 dict(t=CT, ep_o=None, ep_on=None), dict(t=CT, ep_r=None, ep_pad=None, ep_term=None, ep_o=None)]
    else:
        ptrs = ['actions', 'last'] + (['q'] if entry == 'select' else ['ig', 'hg', 'b_ih', 'b_hh', 'h', 'fc_w', 'fc_b'])
        other = [dict(n_actions=0), dict(n_actions=128 if entry == 'select' else 17), dict(n_agents=0), dict(n_envs=-1), dict(eps=None),
                 dict(draw=None)]
        if entry != 'select':
            other += [dict(hidden=64), dict(hidden=256)]
        if entry != 'stream':
            other += [dict(t=-1), dict(t=CT)]
        if entry == 'live':
            other += [dict(lst=None), dict(cnt=None)]
        if entry == 'stream':
            other += [dict(t_ep=None), dict(ep_u=None)]
    return [{k: None} for k in ptrs] + other


@pytest.mark.parametrize('entry', ['select', 'full', 'live', 'stream', 'post'])
def test_refused_arguments_leave_every_buffer_alone(entry):
    v, checks = _contract_values(entry)
    assert _call(entry, v) == OK                       # the arguments are valid as they stand
    assert _call(entry, dict(v, n_actions=16) if entry in ('full', 'live', 'stream') else v) == OK
    if entry == 'select':
        assert _call(entry, dict(v, n_actions=127)) == OK
    torch.cuda.synchronize()
    tensors = {k: x for k, x in v.items() if torch.is_tensor(x)}
    before = {k: x.clone() for k, x in tensors.items()}
    for bad in _bad_cases(entry):
        assert _call(entry, dict(v, **bad)) == BAD_ARG, bad
    assert _call(entry, dict(v, n_envs=0)) == OK       # nothing to do, and nothing done
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    for k, x in tensors.items():
        assert torch.equal(x, before[k]), ('a refused call wrote', k)
