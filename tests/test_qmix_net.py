"""QMixNet (network/qmix_net.py) against the reference's module: state_dict keys, a reference-written state dict loads with
weights_only=True, the forward reproduces the reference's output (tests/golden/qmix_net_ref*, tools/oracle/gen_qmix_golden.py);
Agents builds QMIX and refuses MEDA."""
import os
import types

import numpy as np
import pytest
import torch

from marl_dmfb_amd.network.qmix_net import QMixNet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _args(two):
    return types.SimpleNamespace(state_shape=300, hyper_hidden_dim=24, qmix_hidden_dim=32, n_agents=4, two_hyper_layers=two)


@pytest.mark.parametrize('two', [True, False], ids=['two_hyper_layers', 'one_hyper_layer'])
def test_state_dict_keys_load_and_forward(two):
    tag = '2l' if two else '1l'
    ref = torch.load(os.path.join(GOLDEN, 'qmix_net_ref_%s.pkl' % tag), map_location='cpu', weights_only=True)
    net = QMixNet(_args(two))
    assert list(net.state_dict().keys()) == list(ref.keys())
    net.load_state_dict(ref)
    g = np.load(os.path.join(GOLDEN, 'qmix_net_ref.npz'))
    with torch.no_grad():
        out = net(torch.as_tensor(g['q']), torch.as_tensor(g['s'])).numpy()
    assert out.shape == (3, 5, 1)
    np.testing.assert_allclose(out, g['q_tot_' + tag], rtol=1e-6, atol=1e-6)


def test_agents_builds_qmix_and_needs_state_shape():
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    kw = dict(alg='qmix', cuda=False, device='cpu', n_actions=5, n_agents=4, obs_shape=(3, 9, 9, 2, 245), episode_limit=40)
    ag = Agents(make_args(state_shape=300, **kw))
    pol = ag.policy
    assert type(pol).__name__ == 'QMIX' and pol.needs_state
    assert isinstance(pol.eval_qmix_net, QMixNet) and isinstance(pol.target_qmix_net, QMixNet)
    assert len(pol.eval_parameters) <= 32
    assert not pol.packed_ok({})
    with pytest.raises(ValueError, match='state_shape'):
        Agents(make_args(**kw))


def test_meda_qmix_raises():
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    args = make_args(name='meda', drop_num=4, width=30, length=30, fov=19, alg='qmix', cuda=False, device='cpu', n_actions=9,
                     n_agents=4, obs_shape=(3, 19, 19, 2, 3 * 19 * 19 + 2), episode_limit=120, state_shape=2700)
    with pytest.raises(ValueError, match='MEDA'):
        Agents(args)


def test_alg_flag_choices():
    from marl_dmfb_amd.common.arguments import get_train_args
    assert get_train_args(['dmfb', '--alg', 'qmix']).alg == 'qmix'
    with pytest.raises(SystemExit):
        get_train_args(['dmfb', '--alg', 'coma'])


def test_replay_buffer_state_views():
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.common.replay_buffer import ReplayBuffer
    kw = dict(cuda=False, device='cpu', n_actions=5, n_agents=2, obs_shape=(3, 9, 9, 2, 245), episode_limit=6, buffer_size=4)
    assert 's' not in ReplayBuffer(make_args(**kw)).buffers
    buf = ReplayBuffer(make_args(alg='qmix', state_shape=12, **kw))
    E, T = 3, 6
    ep = {k: torch.zeros(v.shape[1:], dtype=v.dtype).expand(E, *v.shape[1:]).clone() for k, v in buf.buffers.items()}
    ep['s'] = torch.arange(E * T * 12, dtype=torch.int64).remainder(100).to(torch.int8).view(E, T, 12)
    ep['s_next'] = torch.roll(ep['s'], -1, dims=1)
    ep['padded'][:] = False
    buf.store_episode(ep)
    b = buf.sample(5)
    assert b['s'].shape == (5, T, 12) and b['s_next'].data_ptr() == b['s'].data_ptr() + 12
    assert torch.equal(buf.buffers['s'][:E, 0], ep['s'][:, 0]) and torch.equal(buf.buffers['s_next'][:E], ep['s_next'])
