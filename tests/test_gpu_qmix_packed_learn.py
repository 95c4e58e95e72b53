"""QMIX.learn_packed (args.qmix_packed): the learn on the valid steps of the drawn episodes.

  * the two learn goldens (tests/golden/qmix_learn_*.npz, the reference's numbers) through learn_packed, the golden batch as the
    ring and its episodes in the order ReplayBuffer.draw hands them over, at the tolerances of qmix_helpers.qmix_learn_golden_check
    (rtol = atol = 1e-5, mixer weights at 1e-5);
  * padded steps are never read: the same episodes at scattered slots of a larger ring whose padded steps, state rows above the
    length and other slots hold 0x7f / NaN give the same bits;
  * the Trainer in stream mode with the flag learns, by the criteria of test_qmix_trainer_with_stream_state_learns, and never
    gathers a padded batch;
  * VDN ignores the flag."""
import glob
import os

import numpy as np
import pytest
import torch

from qmix_helpers import load_learn_golden, qmix_agents, qmix_check_sampled, replay_batch
from vdn_helpers import det_init

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FILES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'qmix_learn_*.npz')))
IDS = [os.path.basename(p)[:-4] for p in FILES]


def _agents(g):
    W, L, n, fov, hh, clip, T, T_b = [int(v) for v in g['cfg']]
    agents = qmix_agents(W, L, n, fov, DEV, qmix_packed=True)
    pol = agents.policy
    assert pol.args.hyper_hidden_dim == hh and pol.args.grad_norm_clip == clip
    det_init(pol.eval_rnn)
    det_init(pol.target_rnn, salt=0.5)
    det_init(pol.eval_qmix_net, salt=0.3)
    pol.target_qmix_net.load_state_dict(pol.eval_qmix_net.state_dict())
    assert [str(x) for x in g['names']] == [k for k, _ in pol.eval_rnn.named_parameters()]
    assert [str(x) for x in g['mixer_names']] == [k for k, _ in pol.eval_qmix_net.named_parameters()]
    return agents


def _draw(ring):
    lens = (~ring['padded'][:, :, 0]).sum(1).cpu().numpy()
    order = np.argsort(-lens, kind='stable')
    return order, lens[order]


def _check_step(g, pol, step, rtol=1e-5, atol=1e-5):
    """The assertions of qmix_helpers.qmix_learn_golden_check for one learn."""
    qmix_check_sampled(g, step, pol.last_loss, pol.last_grad_norm, [(k, p.grad, p) for k, p in pol.eval_rnn.named_parameters()],
                       [(k, p.grad, p) for k, p in pol.eval_qmix_net.named_parameters()], rtol, atol)


@pytest.mark.parametrize('path', FILES, ids=IDS)
def test_learn_packed_matches_the_reference(path):
    g = load_learn_golden(path)
    pol = _agents(g).policy
    for step in range(2):
        ring = replay_batch(g, DEV, ring_layout=True)
        assert pol.packed_ok(ring), 'the packed learn must apply to this golden'
        idx, lens = _draw(ring)
        assert int(lens.sum()) < ring['o'].shape[0] * ring['o'].shape[1]        # there are padded steps to leave out
        pol.learn_packed(ring, idx, lens, step)
        _check_step(g, pol, step)
    pol.check_td_inputs()


def _poison(t):
    if t.dtype == torch.float32:
        t.fill_(float('nan'))
    else:
        t.view(torch.uint8).fill_(0x7f)


def _scattered(ring, lens_by_slot, gen):
    """The episodes of `ring` at scattered slots of a ring three times the size; every byte that no valid step owns -- the padded
    steps of every tensor, the state rows above an episode's closing state, every other slot -- holds 0x7f (NaN in `r`)."""
    B, T = ring['o'].shape[:2]
    slots = 3 * B + 5
    place = torch.randperm(slots, generator=gen)[:B]
    states = torch.empty((slots, T + 1, ring['s'].shape[-1]), dtype=torch.int8, device=DEV)
    _poison(states)
    big = {}
    for k, src in ring.items():
        if k in ('s', 's_next'):
            continue
        big[k] = torch.empty((slots,) + tuple(src.shape[1:]), dtype=src.dtype, device=DEV)
        _poison(big[k])
    for b in range(B):
        ln, slot = int(lens_by_slot[b]), int(place[b])
        for k in big:
            big[k][slot, :ln] = ring[k][b, :ln]
        states[slot, :ln] = ring['s'][b, :ln]
        states[slot, ln] = ring['s_next'][b, ln - 1]
    big['s'], big['s_next'] = states[:, :T], states[:, 1:]
    return big, place.numpy()


def test_padded_steps_and_other_slots_are_never_read():
    g = load_learn_golden(FILES[-1])
    outs = []
    for scattered in (False, True):
        pol = _agents(g).policy
        ring = replay_batch(g, DEV, ring_layout=True)
        idx, lens = _draw(ring)
        if scattered:
            by_slot = np.empty(len(idx), np.int64)
            by_slot[idx] = lens
            ring, place = _scattered(ring, by_slot, torch.Generator().manual_seed(3))
            assert pol.packed_ok(ring)
            assert bool((ring['u'].view(torch.uint8) == 0x7f).any()) and bool(torch.isnan(ring['r']).any())
            idx = place[idx]
        pol.learn_packed(ring, idx, lens, 0)
        pol.check_td_inputs()
        outs.append([pol.last_loss.reshape(1), pol.last_grad_norm.reshape(1)] +
                    [p.grad.clone() for p in list(pol.eval_rnn.parameters()) + list(pol.eval_qmix_net.parameters())])
    assert bool(torch.isfinite(outs[0][0]).all())
    for k, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'tensor %d differs between the compact and the scattered ring' % k


def test_qmix_trainer_with_the_packed_learn_learns():
    from test_gpu_qmix_stream import _trainer
    torch.manual_seed(0)
    rounds = 60
    tr = _trainer(rounds=rounds, stream_state=True, qmix_packed=True)
    assert tr.stream
    r0, _, c0, _ = tr.rolloutWorker.evaluate(2)
    seen = []
    tr.agents.train = lambda *a, **kw: seen.append(1)
    for _ in range(rounds):
        assert tr.collect_and_learn() == 512 * 40
    r1, _, c1, _ = tr.rolloutWorker.evaluate(2)
    print('qmix packed greedy reward %.2f -> %.2f, constraints %.2f -> %.2f' % (r0, r1, c0, c1))
    assert tr._packed is True and not seen             # every learn was a packed one
    assert tr.trained_times == 4 * rounds
    assert torch.isfinite(tr.agents.policy.last_loss)
    assert r1 > r0 + 40.0, (r0, r1)
    assert c1 < 0.2 * c0 + 1.0, (c0, c1)
    tr.agents.policy.check_td_inputs()


def test_the_flag_without_a_packed_learn_raises_at_the_first_learn():
    from test_gpu_qmix_stream import _trainer
    tr = _trainer(E=64, stream_state=True, qmix_packed=True, fused_mix=False)     # outside packed_ok's limits
    with pytest.raises(RuntimeError, match='qmix_packed'):
        tr.collect_and_learn()
    assert tr._packed is False


def test_vdn_ignores_the_flag():
    from test_gpu_qmix_stream import _trainer
    outs = []
    for flag in (False, True):
        torch.manual_seed(0)
        tr = _trainer(E=64, alg='vdn', qmix_packed=flag)
        assert tr.stream
        for _ in range(3):
            tr.collect_and_learn()
        assert tr._packed is True
        filled = tr.buffer.current_size                    # the slots behind it were never written
        assert filled >= 64
        outs.append((filled, {k: v[:filled].clone() for k, v in tr.buffer.buffers.items()},
                     {k: v.clone() for k, v in tr.agents.policy.eval_rnn.state_dict().items()}))
    assert outs[0][0] == outs[1][0]
    for part in (1, 2):
        for k, v in outs[0][part].items():
            assert torch.equal(v, outs[1][part][k]), k
