"""Generate the QMIX golden vectors by RUNNING THE REFERENCE (container-only; imports it at run time, copies nothing).

  tests/golden/globalobs_<golden>.npz  RoutingTaskManager.getglobalobs() (dmfb.py:368-391) of the reference, evaluated on
        the droplet positions / goals / blocks the reference recorded in the DMFB goldens (tests/golden/dmfb_*.npz): after the
        task injection (restart) of every episode ('gobs0', per episode) and after every step ('gobs', per record).
  tests/golden/qmix_net_ref_{2,1}l.pkl + qmix_net_ref.npz  state dicts of the reference's QMixNet under det_init weights
        (two_hyper_layers True / False) and its forward on fixed inputs.
  tests/golden/qmix_learn_<tag>.npz  two consecutive learns of the reference's QMIX (policy/qmix.py:79-128) on the batch of
        vdn_learn_<tag>.npz plus a global state, with the agent network swapped for the reference's CRNN and VDN's inputs
        (observation + last action, policy/vdn.py:134-165), stored without the batch keys vdn_learn_<tag>.npz holds: loss, grad
        norms, sampled CRNN gradients / weights (as the VDN goldens), and the mixer's gradients (weights) in full for tensors up to
        MIXER_FULL_GRAD (MIXER_FULL_W) elements, at 2048 sampled elements ('midx/') above that: the 4-droplet golden keeps every
        mixer gradient in full; a 20x20 state makes the first layers 32 x 1200, which in full would make the file 1.8 MB.  The state is synthetic but shaped like getglobalobs(): per
        episode one droplet layout per step (values 1..n in layers 0 / 1, a few block cells in layer 2), with
        s_next[t] == s[t + 1] on valid steps and zeros on padded ones.

Run: python tools/oracle/gen_qmix_golden.py
"""
import os
import sys
import types

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402

ref_shim.install()
from env.DMFB.dmfb import Block, DMFBenv, Droplet  # noqa: E402
from network.base_net import CRNN  # noqa: E402
from network.qmix_net import QMixNet  # noqa: E402
from policy.qmix import QMIX  # noqa: E402
from policy.vdn import VDN  # noqa: E402

from gen_vdn_golden import det_init, sample_idx  # noqa: E402

MIXER_FULL_GRAD, MIXER_FULL_W = 16384, 4096
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'tests', 'golden')


def gen_globalobs(name):
    g = np.load(os.path.join(OUT, name + '.npz'))
    W, L, n = [int(v) for v in g['cfg'][:3]]
    env = DMFBenv(W, L, n, 0, fov=5)
    rm = env.routing_manager
    ep_len = g['ep_len'].astype(int)
    first = np.concatenate([[0], np.cumsum(ep_len)[:-1]])
    blocks = g['blocks'] if 'blocks' in g else np.zeros((len(ep_len), 0, 4), np.int32)

    def state(e, pos):
        rm.blocks = [Block(*[int(v) for v in b]) for b in blocks[e]]
        rm.droplets = [Droplet(int(pos[i][0]), int(pos[i][1]), int(g['ends'][e][i][0]), int(g['ends'][e][i][1])) for i in range(n)]
        rm.n_droplets = n
        return rm.getglobalobs().astype(np.int8)
    gobs0 = np.stack([state(e, g['starts'][e]) for e in range(len(ep_len))])
    gobs = np.zeros((int(ep_len.sum()), 3, W, L), np.int8)
    for e in range(len(ep_len)):
        for t in range(ep_len[e]):
            gobs[first[e] + t] = state(e, g['pos'][first[e] + t])
    path = os.path.join(OUT, 'globalobs_%s.npz' % name.replace('dmfb_', ''))
    np.savez_compressed(path, gobs0=gobs0, gobs=gobs, source=np.array(name))
    print(os.path.basename(path), gobs.shape, os.path.getsize(path))


def net_args(two, n=4, S=300, hh=24):
    return types.SimpleNamespace(state_shape=S, hyper_hidden_dim=hh, qmix_hidden_dim=32, n_agents=n, two_hyper_layers=two)


def gen_net():
    rng = np.random.default_rng(7)
    out = {}
    q = rng.normal(0, 1, (3, 5, 4)).astype(np.float32)
    s = (rng.random((3, 5, 300)) < 0.05).astype(np.float32) * rng.integers(1, 5, (3, 5, 300))
    out['q'], out['s'] = q, s.astype(np.float32)
    for two in (True, False):
        torch.manual_seed(0)
        net = QMixNet(net_args(two))
        det_init(net, salt=0.3)
        tag = '2l' if two else '1l'
        torch.save(net.state_dict(), os.path.join(OUT, 'qmix_net_ref_%s.pkl' % tag))
        with torch.no_grad():
            out['q_tot_' + tag] = net(torch.as_tensor(q), torch.as_tensor(out['s'])).numpy()
    np.savez_compressed(os.path.join(OUT, 'qmix_net_ref.npz'), **out)
    print('qmix_net_ref', {k: v.shape for k, v in out.items()})


def synth_states(rng, padded, W, L, n):
    """(s, s_next) int8 (B, T, 3WL): one random layout per step, s_next[t] = s[t + 1] on valid steps, zeros on padded ones."""
    B, T = padded.shape
    S = 3 * W * L
    lay = np.zeros((B, T + 1, 3, W, L), np.int8)
    for b in range(B):
        blk = [(int(rng.integers(0, W - 1)), int(rng.integers(0, L - 1))) for _ in range(2)]
        gx, gy = rng.integers(0, W, n), rng.integers(0, L, n)
        for t in range(T + 1):
            for x, y in blk:
                lay[b, t, 2, x:x + 2, y:y + 2] = 1
            px, py = rng.integers(0, W, n), rng.integers(0, L, n)
            for i in range(n):
                lay[b, t, 0, px[i], py[i]] = i + 1
                lay[b, t, 1, gx[i], gy[i]] = i + 1
    lay = lay.reshape(B, T + 1, S)
    valid = ~padded.astype(bool)
    s = lay[:, :T] * valid[:, :, None]
    s_next = lay[:, 1:] * valid[:, :, None]
    return s.astype(np.int8), s_next.astype(np.int8)


def gen_learn(tag):
    g = dict(np.load(os.path.join(OUT, 'vdn_learn_%s.npz' % tag)))
    W, L, n, fov, hh, clip = [int(v) for v in g['cfg'][:6]]
    with open('/root/reference/data-dmfb/TrainParas/{}d.yaml'.format(n)) as f:
        net, train = yaml.safe_load_all(f.read())
    env = DMFBenv(W, L, n, 0, fov=fov)
    a = types.SimpleNamespace(alg='qmix', net='crnn', last_action=True, reuse_network=True, cuda=False, optimizer='ADAM', gamma=0.99,
                              model_dir='/tmp/model', load_model=False, load_model_name='', ith_run=0, fov=fov, width=W, length=L,
                              chip_size=W, drop_num=n, block_num=0, stall=True)
    a.__dict__.update(net)
    a.__dict__.update(train)
    a.__dict__.update(env.get_env_info())
    a.state_shape = 3 * W * L
    rng = np.random.default_rng(11)
    s, s_next = synth_states(rng, g['padded'][:, :, 0], W, L, n)
    torch.manual_seed(0)
    pol = QMIX(a)
    # the project's QMIX agent network: the reference CRNN with VDN's inputs (no agent-id one-hot)
    pol.eval_rnn, pol.target_rnn = CRNN(a), CRNN(a)
    det_init(pol.eval_rnn)
    det_init(pol.target_rnn, salt=0.5)
    det_init(pol.eval_qmix_net, salt=0.3)
    pol.target_qmix_net.load_state_dict(pol.eval_qmix_net.state_dict())
    pol._get_inputs = types.MethodType(VDN._get_inputs, pol)
    pol.get_q_values = types.MethodType(VDN.get_q_values, pol)
    pol.eval_parameters = list(pol.eval_qmix_net.parameters()) + list(pol.eval_rnn.parameters())
    pol.optimizer = torch.optim.Adam(pol.eval_parameters, lr=a.lr, betas=(0.9, 0.99))
    keys = ['o', 'u', 'r', 'o_next', 'avail_u', 'avail_u_next', 'u_onehot', 'padded', 'terminated']
    batch = {k: g[k] for k in keys}
    batch['s'], batch['s_next'] = s, s_next
    out = {'s': s, 's_next': s_next, 'source': np.array('vdn_learn_%s.npz' % tag)}   # the rest of the batch: that golden's
    norms, losses = [], []
    orig_clip = torch.nn.utils.clip_grad_norm_

    def clip_fn(params, max_norm, *x, **k):
        v = orig_clip(params, max_norm, *x, **k)
        norms.append(float(v))
        return v
    torch.nn.utils.clip_grad_norm_ = clip_fn
    orig_backward = torch.Tensor.backward

    def backward(self, *x, **k):
        losses.append(float(self.detach()))
        return orig_backward(self, *x, **k)
    torch.Tensor.backward = backward
    T = g['padded'].shape[1]
    lens = (1 - g['padded'][:, :, 0].astype(int)).sum(1)
    term = g['terminated'][:, :, 0] == 1
    T_b = int(max(np.argmax(term[b]) if term[b].any() else -1 for b in range(term.shape[0]))) + 1   # agent/agent.py:51-61
    for step in range(2):
        bt = {k: v[:, :T_b].copy() for k, v in batch.items()}
        pol.learn(bt, T_b, step)
        for nm, p in pol.eval_rnn.named_parameters():
            idx = sample_idx(p.numel())
            out['idx/%s' % nm] = idx
            out['grad%d/%s' % (step, nm)] = p.grad.detach().reshape(-1)[idx].numpy().copy()
            out['w%d/%s' % (step, nm)] = p.detach().reshape(-1)[idx].numpy().copy()
        for nm, p in pol.eval_qmix_net.named_parameters():
            # mixer gradients in full up to MIXER_FULL_GRAD elements, weights up to MIXER_FULL_W; larger tensors at 2048 sampled
            # elements ('midx/'), so that a 20x20 state (first layers of 32 x 1200) keeps the file small
            grad, w = p.grad.detach().numpy().copy(), p.detach().numpy().copy()
            if p.numel() > MIXER_FULL_W:
                idx = sample_idx(p.numel(), 2048)
                out['midx/%s' % nm] = idx
                w = w.reshape(-1)[idx]
                if p.numel() > MIXER_FULL_GRAD:
                    grad = grad.reshape(-1)[idx]
            out['mgrad%d/%s' % (step, nm)] = grad
            out['mw%d/%s' % (step, nm)] = w
    torch.nn.utils.clip_grad_norm_ = orig_clip
    torch.Tensor.backward = orig_backward
    out['loss'] = np.array(losses)
    out['grad_norm'] = np.array(norms)
    out['names'] = np.array([nm for nm, _ in pol.eval_rnn.named_parameters()])
    out['mixer_names'] = np.array([nm for nm, _ in pol.eval_qmix_net.named_parameters()])
    out['cfg'] = np.array([W, L, n, fov, hh, clip, T, T_b])
    path = os.path.join(OUT, 'qmix_learn_%s.npz' % tag)
    np.savez_compressed(path, **out)
    print(os.path.basename(path), 'lens', lens.tolist(), 'T_b', T_b, 'loss', losses, 'norms', norms, os.path.getsize(path))


if __name__ == '__main__':
    for name in ('dmfb_A_12x9_3d_fov7', 'dmfb_F_20x20_10d_fov9_12blocks', 'dmfb_D_50x50_10d_fov9'):
        gen_globalobs(name)
    gen_net()
    gen_learn('4d_od24')
    gen_learn('10d_od32')
