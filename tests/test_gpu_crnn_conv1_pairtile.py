"""conv1 of the fov-9 front end at od 24 (marl_dmfb_amd/csrc/crnn_mfma.h): the channels 16..23 run on PAIR tiles -- 8 channels x 2
adjacent output positions (horizontal pairs in columns 0..5, vertical pairs in column 6) over the union of their 3x3 windows, 12
taps x 3 input channels = 9 k-steps -- and the 49 positions are dealt out to the waves by role.  What can go wrong there: a weight
in the wrong union tap (a shifted or a neighbour's pixel), the wrong input channel, a position left out, written twice or written
by the masked half of the last vertical pair, a channel in the wrong column.

Exact integer cases through the C ABI (include/crnn_ops.h), expected values from an int64 numpy convolution, compared with ==:
27 networks whose conv1 has exactly ONE weight per output channel -- slot (t + channel) % 27 of the 27 (input channel, tap) slots
in network t, so every slot of every channel (16..23, and 0..15 as the control) is singled out once -- and whose conv2 copies channel
c through ONE tap, tap t % 9, so that the 25 outputs of a channel show the conv1 positions (y + ty, x + tx): every one of the 49
positions, each through every tap that can reach it, over the set.  1, 15, 16, 17 and 33 rows (row block: 16), crnn_front9_forward
and crnn_conv9_forward, and the live-row list."""
import functools

import numpy as np
import pytest
import torch

import front_kernel_cases as K
import test_gpu_crnn_pairtile as P

gpu = pytest.mark.gpu
OD, A, PAD, NF, DEV, SENT = P.OD, P.A, P.PAD, P.NF, P.DEV, P.SENT
N_NETS = 27
ROW_COUNTS = (1, 15, 16, 17, 33)


@functools.lru_cache(maxsize=None)
def _net(t):
    """Network t: conv1 weight 1 + (c + t) % 3 at slot (t + c) % 27 of output channel c, biases 0..3 (pixels are 0..4: activations
    of 0..15, most of them different); conv2 = channel c through tap t % 9 with weight 1, biases in {-1, 0, 1}; mlp1 in {-1, 0, 1}."""
    g = np.random.default_rng(300 + t)
    n = dict(w1=np.zeros((OD, 3, 3, 3), dtype=np.int64), b1=g.integers(0, 4, (OD,)), w2=np.zeros((OD, OD, 3, 3), dtype=np.int64),
             b2=g.integers(-1, 2, (OD,)), mlp_w=g.integers(-1, 2, (10, 2 + A)), mlp_b=g.integers(-1, 2, (10,)))
    tap = t % 9
    for c in range(OD):
        slot = (t + c) % 27
        n['w1'][c, slot // 9, (slot % 9) // 3, slot % 3] = 1 + (c + t) % 3
        n['w2'][c, c, tap // 3, tap % 3] = 1
    return n


def test_one_weight_networks_single_out_every_slot_and_show_every_position():
    """Over the 27 networks every (input channel, tap) slot of every conv1 output channel carries a weight exactly once, and the
    outputs of every channel show each of the 49 conv1 positions (conv2 tap t % 9 shifts the 5x5 outputs over the 7x7 map)."""
    hit = sum((_net(t)['w1'] != 0).astype(np.int64) for t in range(N_NETS))
    assert hit.shape == (OD, 3, 3, 3) and bool((hit == 1).all())
    for t in range(N_NETS):
        assert int((_net(t)['w1'] != 0).sum()) == OD and int((_net(t)['w2'] != 0).sum()) == OD
    seen = np.zeros((OD, 7, 7), dtype=np.int64)
    for t in range(N_NETS):
        c2, c1, ty, tx = np.nonzero(_net(t)['w2'])
        assert bool((c2 == c1).all())
        for c, y, x in zip(c1, ty, tx):
            seen[c, y:y + 5, x:x + 5] += 1
    # a corner position is reached through one tap only, that is by three of the 27 networks (the dense network of
    # tests/test_gpu_crnn_pairtile.py has every slot at every position at once)
    assert int(seen.min()) == 3


@functools.lru_cache(maxsize=None)
def _expected(t, rows):
    n = _net(t)
    obs, onehot = P._rows(rows)
    x = obs[:, :243].astype(np.int64).reshape(rows, 3, 9, 9)
    a2 = P._conv_i64(P._conv_i64(x, n['w1'], n['b1']), n['w2'], n['b2'])
    assert int(np.abs(a2).max()) < 2 ** 20
    v = np.concatenate([obs[:, 243:], onehot], axis=1).astype(np.int64)
    out = np.concatenate([a2.reshape(rows, -1), np.maximum(v @ n['mlp_w'].T + n['mlp_b'], 0)], axis=1)
    out.setflags(write=False)
    return out


def test_the_expected_outputs_depend_on_the_singled_out_weight():
    """Host only: the reference is not blind -- in network t the outputs of channel c are b2 + relu(b1 + w * pixel) of ONE pixel."""
    rows, t = 3, 5
    n, want = _net(t), _expected(t, rows)
    obs, _ = P._rows(rows)
    x = obs[:, :243].astype(np.int64).reshape(rows, 3, 9, 9)
    tap = t % 9
    for c in (0, 16, 23):
        slot = (t + c) % 27
        c0, ky, kx = slot // 9, (slot % 9) // 3, slot % 3
        pix = x[:, c0, ky + tap // 3:ky + tap // 3 + 5, kx + tap % 3:kx + tap % 3 + 5]
        a = np.maximum(n['b2'][c] + np.maximum(n['b1'][c] + (1 + (c + t) % 3) * pix, 0), 0)
        assert np.array_equal(want[:, c * 25:(c + 1) * 25], a.reshape(rows, 25))


@gpu
@pytest.mark.parametrize('rows', ROW_COUNTS)
def test_front9_one_weight_conv1_networks_exact(rows):
    """crnn_front9_forward, the 27 networks, 640 columns into a wider sentinel-filled buffer, observation stride 245 + 11."""
    obs_np, oh_np = P._rows(rows)
    obs, chk_obs = P._strided_obs(obs_np, 11)
    oh = torch.from_numpy(oh_np).to(DEV)
    for t in range(N_NETS):
        d = P._dev_net(_net(t))
        out, chk_out = K.guarded((rows + 3, PAD + 4), torch.float32, SENT, DEV)
        assert P._call('front9', d, obs, oh, rows, out, PAD + 4, PAD) == 0
        torch.cuda.synchronize()
        chk_out()
        chk_obs()
        P._equal(out[:rows, :NF], _expected(t, rows), 'conv1 network %d rows %d' % (t, rows))
        assert bool((out[:rows, NF:PAD] == 0).all()), 'columns 610..639 are not zero'
        assert bool((out[:rows, PAD:] == SENT).all()) and bool((out[rows:] == SENT).all()), 'written beside the rows'


@gpu
@pytest.mark.parametrize('rows', ROW_COUNTS)
def test_conv9_one_weight_conv1_networks_exact(rows):
    """crnn_conv9_forward (no vector branch, 600 columns), contiguous rows and an odd output stride."""
    obs_np, _ = P._rows(rows)
    obs, chk_obs = P._strided_obs(obs_np, 0)
    for t in range(N_NETS):
        d = P._dev_net(_net(t))
        out, chk_out = K.guarded((rows + 2, 607), torch.float32, SENT, DEV)
        assert P._call('conv9', d, obs, None, rows, out, 607, 0) == 0
        torch.cuda.synchronize()
        chk_out()
        chk_obs()
        P._equal(out[:rows, :600], _expected(t, rows)[:, :600], 'conv9, conv1 network %d rows %d' % (t, rows))
        assert bool((out[:rows, 600:] == SENT).all()) and bool((out[rows:] == SENT).all()), 'written beside the rows'


@gpu
def test_front9_live_list_one_weight_conv1_networks_exact():
    """crnn_front9_forward_live on 5 chips of 7 rows, chips 1, 3 and 4 live: their rows, compacted, exact; nothing behind them."""
    rpc, live = 7, [1, 3, 4]
    rows = 5 * rpc
    obs_np, oh_np = P._rows(rows)
    obs, chk_obs = P._strided_obs(obs_np, 3)
    oh = torch.from_numpy(oh_np).to(DEV)
    ids, chk_ids = K.guarded((5,), torch.int32, 0, DEV)
    ids[:len(live)] = torch.tensor(live, dtype=torch.int32, device=DEV)
    n_live, chk_n = K.guarded((1,), torch.int32, len(live), DEV)
    src = np.array([c * rpc + a for c in live for a in range(rpc)], dtype=np.int64)
    for t in range(N_NETS):
        d = P._dev_net(_net(t))
        out, chk_out = K.guarded((rows + 2, PAD), torch.float32, SENT, DEV)
        assert P._call('live', d, obs, oh, rows, out, PAD, PAD, live=(ids, n_live, rpc)) == 0
        torch.cuda.synchronize()
        for chk in (chk_out, chk_obs, chk_ids, chk_n):
            chk()
        n = len(src)
        assert bool((out[n:] == SENT).all()), 'rows behind the live ones were written'
        P._equal(out[:n, :NF], _expected(t, rows)[src], 'live, conv1 network %d' % t)
        assert bool((out[:n, NF:] == 0).all()), 'columns 610..639 are not zero'
