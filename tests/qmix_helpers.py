"""Shared by the QMIX tests: args / Agents for a golden configuration (DMFB or MEDA), the learn-golden check against
tests/golden/qmix_learn_*.npz (tools/oracle/gen_qmix_golden.py) with its rule as one function on tensors (`qmix_check_sampled`),
and the cases and learn paths of the full-tensor check against the float64 learn (F64_PATHS, F64_CASES, `f64_case_agents`,
`f64_case_learn`: tests/test_gpu_qmix_learn_f64.py, tools/diag_learn_f64.py qmix)."""
import os

import numpy as np
import torch

from vdn_helpers import det_init

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
KEYS = ['o', 'u', 'r', 'o_next', 'avail_u', 'avail_u_next', 'u_onehot', 'padded', 'terminated']


def qmix_agents(W, L, n, fov, device, **kw):
    """Agents with a QMIX learner.  DMFB (5 actions, state 3 W L, episode limit 2 (W + L)) unless `kw` says otherwise; MEDA takes
    name='meda', meda_state=True, n_actions=9, state_shape=2 W L and its episode_limit."""
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    over = dict(n_actions=5, episode_limit=2 * (W + L), state_shape=3 * W * L)
    over.update(kw)
    args = make_args(name=over.pop('name', 'dmfb'), drop_num=n, width=W, length=L, fov=fov, alg='qmix', cuda=(device != 'cpu'),
                     device=device, n_agents=n, obs_shape=(3, fov, fov, 2, 3 * fov * fov + 2), **over)
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


def qmix_check_sampled(g, step, loss, grad_norm, crnn, mixer, rtol=1e-5, atol=1e-5):
    """The rule of the QMIX learn goldens for one learn, on tensors: `crnn` and `mixer` yield (name, whole gradient, whole weight
    tensor) of the agent network and of the mixer.  Loss and gradient norm, the CRNN tensors at the elements the golden sampled
    (g['idx/<name>']), the mixer tensors in full or at g['midx/<name>'] are held to the reference's numbers."""
    np.testing.assert_allclose(float(loss), g['loss'][step], rtol=rtol)
    np.testing.assert_allclose(float(grad_norm), g['grad_norm'][step], rtol=rtol)
    for name, grad, w in crnn:
        idx = torch.as_tensor(g['idx/' + name])
        ref_g = g['grad%d/%s' % (step, name)]
        np.testing.assert_allclose(grad.detach().reshape(-1).cpu()[idx].numpy(), ref_g, rtol=rtol,
                                   atol=atol * (np.abs(ref_g).max() + 1e-12), err_msg='grad %s step %d' % (name, step))
        np.testing.assert_allclose(w.detach().reshape(-1).cpu()[idx].numpy(), g['w%d/%s' % (step, name)], rtol=rtol, atol=2e-6)
    for name, grad, w in mixer:
        # large first-layer tensors are stored at sampled elements ('midx/'), the rest in full (tools/oracle/gen_qmix_golden.py)
        grad, w = grad.detach().cpu().numpy(), w.detach().cpu().numpy()
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
        qmix_check_sampled(g, step, pol.last_loss, pol.last_grad_norm, [(k, p.grad, p) for k, p in pol.eval_rnn.named_parameters()],
                           [(k, p.grad, p) for k, p in pol.eval_qmix_net.named_parameters()], rtol, atol)
    return agents


# -------------------------------------------------------------------------- the learn paths of tests/test_gpu_qmix_learn_f64.py
# path -> (ring_layout of replay_batch, extra args, value of MARL_DMFB_GRU_PAIR or None)
F64_PATHS = {'fused_ring': (True, {}, None),
             'fused_two_tensors': (False, {}, None),
             'torch_ops': (True, {'fused_mix': False}, None),
             'packed': (True, {'qmix_packed': True}, '1'),            # pair recurrence on the matrix cores: the default
             'packed_valu': (True, {'qmix_packed': True}, '0')}       # the 8-row VALU recurrence kernels
# (batch of tests/qmix_learn_f64.py: SPECS, path): the two reference goldens through all five, MEDA and the other fovs through some
F64_CASES = [(spec, path) for spec in ('qmix_learn_4d_od24', 'qmix_learn_10d_od32') for path in F64_PATHS] + \
            [('meda_4d_od32', path) for path in ('fused_ring', 'torch_ops', 'packed')] + \
            [(spec, path) for spec in ('fov5_4d_od24', 'fov13_3d_od32') for path in ('fused_ring', 'packed')]


def f64_case_agents(g, config, path, device):
    """Agents for one batch of tests/qmix_learn_f64.py (`load_spec`, `spec_config`) and one path of F64_PATHS, with the
    deterministic weights the float64 restatement starts from."""
    kind, W, L, n, fov, hh, clip, A, S = config
    kw = dict(F64_PATHS[path][1])
    if kind == 'meda':
        kw.update(name='meda', meda_state=True, n_actions=A, state_shape=S, episode_limit=int(g['cfg'][7]))
    agents = qmix_agents(W, L, n, fov, device, **kw)
    pol = agents.policy
    assert pol.args.hyper_hidden_dim == hh and pol.args.grad_norm_clip == clip and pol.args.state_shape == S and pol.n_actions == A
    det_init(pol.eval_rnn)
    det_init(pol.target_rnn, salt=0.5)
    det_init(pol.eval_qmix_net, salt=0.3)
    pol.target_qmix_net.load_state_dict(pol.eval_qmix_net.state_dict())
    assert [str(x) for x in g['names']] == [k for k, _ in pol.eval_rnn.named_parameters()]
    return agents


def f64_case_learn(g, agents, path, device, step):
    """One learn (train_step = step) of the batch through the path, by the public Agents.train / QMIX.learn_packed; the path's
    precondition is asserted first."""
    pol = agents.policy
    batch = replay_batch(g, device, F64_PATHS[path][0])
    if path.startswith('packed'):
        assert pol.packed_ok(batch) is True, 'the packed learn must apply to this batch'
        lens = (~batch['padded'][:, :, 0]).sum(1).cpu().numpy()
        order = np.argsort(-lens, kind='stable')                       # the draw of test_gpu_qmix_packed_learn._draw
        assert int(lens.sum()) < batch['o'].shape[0] * batch['o'].shape[1], 'the batch must have padded steps to leave out'
        pol.learn_packed(batch, order, lens[order], step)
    else:
        assert pol._mix_fused_ok(batch) is (path != 'torch_ops'), 'the path under test must be the one the learn takes'
        agents.train(batch, step)
