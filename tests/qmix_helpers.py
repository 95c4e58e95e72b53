"""Shared by the QMIX tests: args / Agents for a golden configuration and the learn-golden check against
tests/golden/qmix_learn_*.npz (tools/oracle/gen_qmix_golden.py)."""
import os

import numpy as np
import torch

from vdn_helpers import det_init

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KEYS = ['o', 'u', 'r', 'o_next', 'avail_u', 'avail_u_next', 'u_onehot', 'padded', 'terminated']


def qmix_agents(W, L, n, fov, device, **kw):
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    args = make_args(drop_num=n, width=W, length=L, fov=fov, alg='qmix', cuda=(device != 'cpu'), device=device, n_actions=5,
                     n_agents=n, obs_shape=(3, fov, fov, 2, 3 * fov * fov + 2), episode_limit=2 * (W + L), state_shape=3 * W * L,
                     **kw)
    return Agents(args)


def load_learn_golden(path):
    q = np.load(path)
    g = dict(np.load(os.path.join(GOLDEN, str(q['source']))))
    g.update({k: q[k] for k in q.files})
    return g


def replay_batch(g, device, ring_layout):
    """The golden batch as ReplayBuffer.sample hands it over (int8 / float32 / bool).  ring_layout: s / s_next as the two views of
    one (B, T + 1, S) tensor, as the ring stores them (slot 0 = s[0], slot t + 1 = s_next[t])."""
    b = {k: torch.as_tensor(g[k]).to(device) for k in KEYS}
    b['padded'], b['terminated'] = b['padded'].bool(), b['terminated'].bool()
    b['r'] = b['r'].float()
    for k in ('u', 'avail_u', 'avail_u_next', 'u_onehot', 'o', 'o_next'):
        b[k] = b[k].to(torch.int8)
    s, s_next = torch.as_tensor(g['s']).to(device), torch.as_tensor(g['s_next']).to(device)
    if ring_layout:
        T = s.shape[1]
        st = torch.cat([s[:, :1], s_next], dim=1)
        b['s'], b['s_next'] = st[:, :T], st[:, 1:]
    else:
        b['s'], b['s_next'] = s, s_next
    return b


def qmix_learn_golden_check(path, device, rtol=1e-5, atol=1e-5, fused=None, ring_layout=True):
    g = load_learn_golden(path)
    W, L, n, fov, hh, clip, T, T_b = [int(v) for v in g['cfg']]
    agents = qmix_agents(W, L, n, fov, device)
    pol = agents.policy
    assert pol.args.hyper_hidden_dim == hh and pol.args.grad_norm_clip == clip
    det_init(pol.eval_rnn)
    det_init(pol.target_rnn, salt=0.5)
    det_init(pol.eval_qmix_net, salt=0.3)
    pol.target_qmix_net.load_state_dict(pol.eval_qmix_net.state_dict())
    assert [str(x) for x in g['names']] == [k for k, _ in pol.eval_rnn.named_parameters()]
    assert [str(x) for x in g['mixer_names']] == [k for k, _ in pol.eval_qmix_net.named_parameters()]
    for step in range(2):
        batch = replay_batch(g, device, ring_layout)
        if fused is not None:
            assert pol._mix_fused_ok(batch) == fused
        agents.train(batch, step)
        np.testing.assert_allclose(float(pol.last_loss), g['loss'][step], rtol=rtol)
        np.testing.assert_allclose(float(pol.last_grad_norm), g['grad_norm'][step], rtol=rtol)
        for name, p in pol.eval_rnn.named_parameters():
            idx = torch.as_tensor(g['idx/' + name])
            ref_g = g['grad%d/%s' % (step, name)]
            np.testing.assert_allclose(p.grad.detach().reshape(-1).cpu()[idx].numpy(), ref_g, rtol=rtol,
                                       atol=atol * (np.abs(ref_g).max() + 1e-12), err_msg='grad %s step %d' % (name, step))
            np.testing.assert_allclose(p.detach().reshape(-1).cpu()[idx].numpy(), g['w%d/%s' % (step, name)], rtol=rtol, atol=2e-6)
        for name, p in pol.eval_qmix_net.named_parameters():
            # large first-layer tensors are stored at sampled elements ('midx/'), the rest in full (tools/oracle/gen_qmix_golden.py)
            grad, w = p.grad.detach().cpu().numpy(), p.detach().cpu().numpy()
            ref_g, ref_w = g['mgrad%d/%s' % (step, name)], g['mw%d/%s' % (step, name)]
            if ref_g.shape != grad.shape:
                grad = grad.reshape(-1)[g['midx/' + name]]
            if ref_w.shape != w.shape:
                w = w.reshape(-1)[g['midx/' + name]]
            np.testing.assert_allclose(grad, ref_g, rtol=rtol, atol=atol * (np.abs(ref_g).max() + 1e-12),
                                       err_msg='mixer grad %s step %d' % (name, step))
            # 1e-5 (2 % of lr) rather than the CRNN weights' 2e-6: Adam moves an element by ~lr whatever its gradient's size, and the
            # first hypernetwork layers hold elements whose gradient (a rarely non-zero state entry) is at rounding level
            np.testing.assert_allclose(w, ref_w, rtol=rtol, atol=1e-5, err_msg='mixer w %s step %d' % (name, step))
    return agents
