"""Shared by tests/test_act_kernel_cases.py (CPU) and tests/test_gpu_act_kernels.py (GPU): a host restatement of what the
rollout's pick kernels compute (include/rollout_ops.h: rollout_select_actions, rollout_gru_head_select and its _live / _stream
variants), in numpy, row by row.

  gru_head_reference   the GRU cell's gate math and the Q head in float64 from the two projections (gate order r|z|n)
  pick_reference       first maximum, and for evaluate == 0 the documented Philox draw through oracle.dmfb_oracle.philox
                       (pinned to the known-answer vectors by tests/test_oracle_dmfb_golden.py)
  make_inputs          the inputs of the fused kernel at unit scale (or `scale` times that for the saturated case)
  onehots, episode_slots   the expected last_onehot and episode tensors of a set of picks

A NEAR TIE is a row whose two largest float64 Q values are GAP = 2e-5 or less apart, twice the project's float32 tolerance on q
(tests/test_gpu_rollout_ops.py: h 1e-6, q 1e-5 absolute): float32 may pick either there.  The GPU tests compare the greedy pick
with the float64 argmax on every other row and require the near ties to be at most MAX_TIE_ROWS of the rows; TOLERANCE_SETS
lists every input set they do that on, and the CPU test asserts the condition for each, so it holds without a GPU."""
import functools
import types

import numpy as np

H = 128                                  # rnn_hidden_dim of the fused kernel
ROWS_PER_GROUP = 8                       # csrc/rollout_ops.hip: half a wave per row, 256 threads per workgroup
H_TOL, Q_TOL = 1e-6, 1e-5                # tests/test_gpu_rollout_ops.py::test_gru_head_select_matches_grucell_and_linear
SAT_TOL = 2e-5                           # tests/test_gpu_packed_learn_kernels.py::test_gru_packed_saturated_gates_...
GAP = 2 * Q_TOL
MAX_TIE_ROWS = 0.01
SEED = 0x1234567811223344                # the two halves differ: a swapped key draws other numbers
DRAWS = (0, 7, 0xffffffff)

# (E, n): E * n = 1, 7, 8, 9, 15, 16, 17 and 4099 rows -- one row, one short of a workgroup, exactly one, one over, one short
# of two, two, one over, and 513 workgroups with a ragged last one (4099 is prime)
ROW_SHAPES = [(1, 1), (7, 1), (2, 4), (3, 3), (5, 3), (4, 4), (17, 1), (4099, 1)]
ACTIONS = [1, 2, 5, 9, 16]
# (E, n, A, who is alive) of the live-variant cases: n_live * n = 24, 0, 1, 1, 7, 7, about 300 and 609 (mod 8: 0, 1 and 7 occur)
LIVE_CASES = [(8, 3, 5, 'all'), (8, 3, 5, 'none'), (9, 1, 5, 'first'), (9, 1, 9, 'last'), (5, 7, 5, 'first'), (5, 7, 16, 'last'),
              (203, 3, 5, 'half'), (203, 3, 5, 'all')]
LIVE_SEED = 3
# (rows, A, seed, scale) of every input set that the GPU module compares with float64 by tolerance
TOLERANCE_SETS = sorted({(E * n, A, 0, 1.0) for E, n in ROW_SHAPES for A in ACTIONS} |
                        {(E * n, A, LIVE_SEED, 1.0) for E, n, A, _ in LIVE_CASES})


def make_inputs(rows, A, seed=0, scale=1.0):
    """ig, hg float32[rows][3H] unit normal times `scale`, h uniform in (-1, 1), biases / fc_w / fc_b uniform in
    +-1/sqrt(H) (the initialisation range of nn.GRUCell / nn.Linear)."""
    g = np.random.default_rng(1000003 * seed + 131 * rows + A)
    k = 1.0 / np.sqrt(H)
    c = types.SimpleNamespace(rows=rows, A=A, seed=seed, scale=scale)
    c.ig = (g.standard_normal((rows, 3 * H)) * scale).astype(np.float32)
    c.hg = (g.standard_normal((rows, 3 * H)) * scale).astype(np.float32)
    c.h = g.uniform(-1.0, 1.0, (rows, H)).astype(np.float32)
    c.b_ih = g.uniform(-k, k, 3 * H).astype(np.float32)
    c.b_hh = g.uniform(-k, k, 3 * H).astype(np.float32)
    c.fc_w = g.uniform(-k, k, (A, H)).astype(np.float32)
    c.fc_b = g.uniform(-k, k, A).astype(np.float32)
    return c


def _sigmoid(x):
    with np.errstate(over='ignore'):     # exp(-x) = inf for x << 0 gives exactly 0, as it should
        return 1.0 / (1.0 + np.exp(-x))


def gru_head_reference(ig, hg, b_ih, b_hh, h, fc_w, fc_b):
    """float64 (h', q) of include/rollout_ops.h: r = s(i_r + h_r + b_ir + b_hr), z alike, n = tanh(i_n + b_in + r (h_n + b_hn)),
    h' = n + z (h - n), q = h' W^T + b."""
    ig, hg, b_ih, b_hh, h, fc_w, fc_b = (np.asarray(a, dtype=np.float64) for a in (ig, hg, b_ih, b_hh, h, fc_w, fc_b))
    hid = h.shape[1]
    r = _sigmoid(ig[:, :hid] + hg[:, :hid] + b_ih[:hid] + b_hh[:hid])
    z = _sigmoid(ig[:, hid:2 * hid] + hg[:, hid:2 * hid] + b_ih[hid:2 * hid] + b_hh[hid:2 * hid])
    n = np.tanh(ig[:, 2 * hid:] + b_ih[2 * hid:] + r * (hg[:, 2 * hid:] + b_hh[2 * hid:]))
    h_new = n + z * (h - n)
    return h_new, h_new @ fc_w.T + fc_b


@functools.lru_cache(maxsize=None)
def _reference(rows, A, seed, scale):
    c = make_inputs(rows, A, seed, scale)
    return gru_head_reference(c.ig, c.hg, c.b_ih, c.b_hh, c.h, c.fc_w, c.fc_b)


def reference(c):
    """gru_head_reference of an unmodified make_inputs case (cached; treat as read-only)."""
    return _reference(c.rows, c.A, c.seed, c.scale)


def first_max(q):
    """Index of the first maximum of every row, scanning with > (+0.0 and -0.0 compare equal)."""
    q = np.asarray(q)
    best = np.zeros(q.shape[0], dtype=np.int64)
    bv = q[:, 0].copy()
    for k in range(1, q.shape[1]):
        better = q[:, k] > bv
        best[better] = k
        bv = np.where(better, q[:, k], bv)
    return best


def top2_gap(q):
    """Distance between the two largest entries of every row (inf for a single action)."""
    q = np.asarray(q, dtype=np.float64)
    if q.shape[1] == 1:
        return np.full(q.shape[0], np.inf)
    s = np.sort(q, axis=1)
    return s[:, -1] - s[:, -2]


@functools.lru_cache(maxsize=None)
def _words(seed, draw, row):
    from oracle.dmfb_oracle import philox
    w = philox(seed & 0xffffffff, seed >> 32, (row, draw, 0, 0x600))
    return int(w[0]), int(w[1])


def draw_words(seed, draw, row_ids):
    """Philox words 0 and 1 of the rows `row_ids` -> uint64[len][2]."""
    out = np.zeros((len(row_ids), 2), dtype=np.uint64)
    for k, r in enumerate(row_ids):
        out[k] = _words(int(seed), int(draw), int(r))
    return out


def draw_u1(seed, draw, row_ids):
    w = draw_words(seed, draw, row_ids)
    return (w[:, 0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def pick_reference(q, seed, draw, eps, evaluate, row_ids):
    """(actions int64[rows], u1 float32[rows]) of rows `row_ids` (their chip-order index e * n + a) with Q values q[rows][A]:
    the first maximum, or, when evaluate == 0 and u1 < float32(eps), (w1 * A) >> 32.  u1 is all ones when evaluate != 0."""
    q = np.asarray(q)
    A = q.shape[1]
    act = first_max(q)
    if evaluate:
        return act, np.ones(q.shape[0], dtype=np.float32)
    w = draw_words(seed, draw, row_ids)
    u1 = (w[:, 0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    rand = ((w[:, 1] * np.uint64(A)) >> np.uint64(32)).astype(np.int64)
    return np.where(u1 < np.float32(eps), rand, act), u1


def onehots(actions, A):
    """int8[rows][A] one-hot of the picks."""
    return (np.arange(A)[None, :] == np.asarray(actions)[:, None]).astype(np.int8)


def episode_slots(actions, E, n, A, T, t, fill, rows=None):
    """The expected u int8[E][T][n] and u_onehot int8[E][T][n][A] of buffers that held `fill` everywhere: the pick of row
    e * n + a at slot (e, t, a), t one step for all chips or one per chip; `rows` (chip-order row ids) limits the written rows."""
    t = np.broadcast_to(np.asarray(t, dtype=np.int64), (E,))
    u = np.full((E, T, n), fill, dtype=np.int8)
    oh = np.full((E, T, n, A), fill, dtype=np.int8)
    actions = np.asarray(actions)
    for r in (range(E * n) if rows is None else rows):
        e, a = divmod(int(r), n)
        u[e, t[e], a] = actions[r]
        oh[e, t[e], a] = np.arange(A) == actions[r]
    return u, oh


def spike(c, count=48, seed=9):
    """`count` entries of ig at +-1e4 (in place), where expf(-x) of the sigmoid overflows."""
    g = np.random.default_rng(seed)
    idx = g.choice(c.ig.size, count, replace=False)
    c.ig.reshape(-1)[idx] = np.where(np.arange(count) % 2 == 0, 1.0e4, -1.0e4).astype(np.float32)
    return c
