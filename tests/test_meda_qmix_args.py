"""args.meda_state (--meda_state on the train and evaluate parsers): QMIX on MEDA mixes on the project's own MEDA global state
(include/meda_vec.h), so it is opt-in; without the flag QMIX refuses MEDA as before, and DMFB and VDN ignore it."""
import pytest
import torch

from marl_dmfb_amd.common.arguments import get_evaluate_args, get_train_args, make_args

W = L = 30
KW = dict(name='meda', drop_num=4, width=W, length=L, fov=19, alg='qmix', cuda=False, device='cpu', n_actions=9, n_agents=4,
          obs_shape=(3, 19, 19, 2, 3 * 19 * 19 + 2), episode_limit=W + L)


def test_meda_state_parses_and_defaults_off():
    assert get_train_args([]).meda_state is False
    assert get_evaluate_args([]).meda_state is False
    assert make_args().meda_state is False and make_args(name='meda').meda_state is False
    a = get_train_args(['meda', '--alg', 'qmix', '--meda_state', '--stream_state'])
    assert a.meda_state is True and a.stream_state is True and a.alg == 'qmix' and a.name == 'meda'
    assert get_evaluate_args(['meda', '--alg', 'qmix', '--meda_state']).meda_state is True


def test_qmix_builds_on_meda_with_the_flag():
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.network.qmix_net import QMixNet
    torch.manual_seed(0)
    ag = Agents(make_args(state_shape=2 * W * L, meda_state=True, **KW))
    pol = ag.policy
    assert type(pol).__name__ == 'QMIX' and pol.needs_state
    assert isinstance(pol.eval_qmix_net, QMixNet)
    assert pol.eval_qmix_net.hyper_w1[0].in_features == 2 * W * L
    # one forward of the mixer on the CPU torch-op path, states as the ring stores them (int8)
    B, T = 3, 5
    s = torch.zeros((B, T, 2 * W * L), dtype=torch.int8)
    s[:, :, 100:125] = 1
    q = torch.randn((B, T, 4))
    assert pol.eval_qmix_net(q, s.float()).shape == (B, T, 1)


def test_qmix_on_meda_without_the_flag_raises():
    from marl_dmfb_amd.agent.agent import Agents
    with pytest.raises(ValueError, match='MEDA') as ei:
        Agents(make_args(state_shape=2 * W * L, **KW))
    assert 'meda_state' in str(ei.value)
    with pytest.raises(ValueError, match='state_shape'):
        Agents(make_args(meda_state=True, **KW))


def test_dmfb_and_vdn_ignore_the_flag():
    from marl_dmfb_amd.agent.agent import Agents
    kw = dict(cuda=False, device='cpu', n_actions=5, n_agents=4, obs_shape=(3, 9, 9, 2, 245), episode_limit=40)
    torch.manual_seed(1)
    a = Agents(make_args(alg='qmix', state_shape=300, meda_state=True, **kw)).policy
    torch.manual_seed(1)
    b = Agents(make_args(alg='qmix', state_shape=300, **kw)).policy
    for k, v in a.eval_qmix_net.state_dict().items():
        assert torch.equal(v, b.eval_qmix_net.state_dict()[k])
    v = Agents(make_args(**dict(KW, alg='vdn'), meda_state=True)).policy
    assert type(v).__name__ == 'VDN'
