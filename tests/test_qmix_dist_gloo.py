"""Data-parallel QMIX learner on CPU (gloo, world_size 2): two ranks learning on the two halves of a minibatch, with the one
flat all-reduce of [gradients of the un-normalised loss, mask count] that VDN uses (tests/test_dist_gloo.py), end with the same
network and mixer weights as one rank learning on the whole minibatch."""
import os
import socket

import numpy as np
import torch
import torch.multiprocessing as mp

from qmix_helpers import GOLDEN, load_learn_golden, qmix_agents, replay_batch
from vdn_helpers import det_init

PATH = os.path.join(GOLDEN, 'qmix_learn_4d_od24.npz')


def _agents(dist):
    torch.manual_seed(0)
    ag = qmix_agents(10, 10, 4, 9, 'cpu', dist=dist)
    det_init(ag.policy.eval_rnn)
    det_init(ag.policy.target_rnn, salt=0.5)
    det_init(ag.policy.eval_qmix_net, salt=0.3)
    ag.policy.target_qmix_net.load_state_dict(ag.policy.eval_qmix_net.state_dict())
    return ag


def _batch(sl):
    b = replay_batch(load_learn_golden(PATH), 'cpu', ring_layout=False)
    b = {k: v[sl].clone() for k, v in b.items()}
    b['padded'][0, 25:] = True      # uneven shards: the mask-count all-reduce matters
    b['terminated'][0, 24:] = True
    b['s'][0, 25:] = 0
    b['s_next'][0, 25:] = 0
    return b


def _state(ag):
    return {**{'rnn.' + k: v.clone() for k, v in ag.policy.eval_rnn.state_dict().items()},
            **{'mix.' + k: v.clone() for k, v in ag.policy.eval_qmix_net.state_dict().items()}}


def _grads(ag):
    """The clipped gradients the first learn left (all-reduced over the ranks, divided by the global mask count)."""
    return {n: p.grad.detach().clone() for n, p in list(ag.policy.eval_rnn.named_parameters()) +
            [('mix.' + n, p) for n, p in ag.policy.eval_qmix_net.named_parameters()]}


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.distributed.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    ag = _agents(dist=True)
    if rank == 1:
        det_init(ag.policy.eval_qmix_net, salt=2.0)   # wrong on purpose: the broadcast must fix it
    ag.policy.broadcast_parameters()            # (also syncs the targets to the eval networks)
    det_init(ag.policy.target_rnn, salt=0.5)
    assert ag.policy.dist
    shard = {k: v[rank * 3:(rank + 1) * 3] for k, v in _batch(slice(0, 6)).items()}
    grads = None
    for step in range(2):
        ag.policy.learn({k: v.clone() for k, v in shard.items()}, 40, step)
        grads = grads or _grads(ag)
    torch.save({'sd': _state(ag), 'grads': grads, 'norm': float(ag.policy.last_grad_norm)}, os.path.join(out_dir, 'rank%d.pt' % rank))
    torch.distributed.destroy_process_group()


def test_qmix_sharded_learn_equals_big_batch(tmp_path):
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(os.path.join(tmp_path, 'rank0.pt'))
    r1 = torch.load(os.path.join(tmp_path, 'rank1.pt'))
    for k in r0['sd']:
        assert torch.equal(r0['sd'][k], r1['sd'][k]), 'ranks diverged on %s' % k
    ag = _agents(dist=False)
    full = _batch(slice(0, 6))
    grads = None
    for step in range(2):
        ag.policy.learn({k: v.clone() for k, v in full.items()}, 40, step)
        grads = grads or _grads(ag)
    assert abs(float(ag.policy.last_grad_norm) - r0['norm']) <= 2e-4 * r0['norm']
    for k, g in grads.items():
        np.testing.assert_allclose(r0['grads'][k].numpy(), g.numpy(), rtol=1e-4, atol=1e-5 * float(g.abs().max()), err_msg=k)
    # Adam moves an element by up to ~lr (5e-4) per step whatever its gradient's size, so an element whose gradient is at rounding
    # level (the sharded and the whole-batch sums round differently) may land up to 2 x 2 x lr away after two steps
    for k, v in _state(ag).items():
        assert np.abs(r0['sd'][k].numpy() - v.numpy()).max() <= 4 * 5e-4 + 1e-6, k
