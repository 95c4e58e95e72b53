"""QMIX end to end on the GPU: the Trainer (episode mode, global state in the ring, fused mixing / TD block) improves the greedy
policy by the criteria of tests/test_gpu_training_learns.py, and a checkpoint written and reloaded gives the same greedy actions."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _trainer(E=512, rounds=60, **kw):
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.train import Trainer
    env = VecDMFB(10, 10, 4, fov=9, n_envs=E, seed=7, device='cuda:0')
    args = make_args(alg='qmix', device='cuda:0', n_envs=E, batch_size=256, train_time=4, buffer_size=8 * E,
                     anneal_steps=E * 40 * rounds * 0.6, **kw, **env.get_env_info())
    return Trainer(env, args)


def test_qmix_short_training_run_improves_greedy_policy():
    torch.manual_seed(0)
    rounds = 60
    tr = _trainer(rounds=rounds)
    assert not tr.stream and tr.args.state_shape == 300
    r0, _, c0, _ = tr.rolloutWorker.evaluate(2)
    for _ in range(rounds):
        tr.collect_and_learn()
    r1, _, c1, _ = tr.rolloutWorker.evaluate(2)
    print('qmix greedy reward %.2f -> %.2f, constraints %.2f -> %.2f' % (r0, r1, c0, c1))
    assert torch.isfinite(tr.agents.policy.last_loss)
    assert r1 > r0 + 40.0, (r0, r1)
    assert c1 < 0.2 * c0 + 1.0, (c0, c1)


def test_stream_mode_refused_for_qmix():
    with pytest.raises(ValueError, match='VDN-only'):
        _trainer(E=64, stream=True)


def test_checkpoint_roundtrip_same_greedy_actions(tmp_path):
    from marl_dmfb_amd.agent.agent import Agents
    torch.manual_seed(1)
    tr = _trainer(E=128, model_dir=str(tmp_path))
    for _ in range(3):
        tr.collect_and_learn()
    tr.agents.policy.save_model(5)
    import os
    d = str(tmp_path) + '/qmix/fov9/'
    assert sorted(os.listdir(d)) == ['0_5_qmix_net_params.pkl', '0_5_rnn_net_params.pkl']
    args = copy.copy(tr.args)
    args.load_model, args.load_model_name = True, '0_5_'
    ag = Agents(args)
    for k, v in tr.agents.policy.eval_qmix_net.state_dict().items():
        assert torch.equal(v, ag.policy.eval_qmix_net.state_dict()[k])
    obs = tr.env.reset()
    E, n = obs.shape[:2]
    la = torch.zeros((E, n, 5), dtype=torch.int8, device='cuda:0')
    h = torch.zeros((E * n, 128), device='cuda:0')
    a1, _ = tr.agents.choose_actions(obs, la, h, 0.0, evaluate=True)
    a2, _ = ag.choose_actions(obs, la, h, 0.0, evaluate=True)
    assert torch.equal(a1, a2)
