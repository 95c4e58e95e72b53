"""The training loop at fov 11 (4 droplets on 14x14) and fov 13 (3 droplets on 16x16) on the HIP front end of
include/crnn_wide.h: the learn against the reference's own numbers, the continuous rollout against the CPU oracle, graph replay
against eager play, and a short training run."""
import os

import numpy as np
import pytest
import torch

from vdn_helpers import learn_golden_check

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# the goldens' shapes (tools/oracle/gen_fov_wide_golden.py), the one-droplet chips of the early-end rollouts, the training shapes
SHAPES = {11: dict(W=14, n=4), 13: dict(W=16, n=3)}
ONE_DROPLET = {11: 12, 13: 14}
TRAIN = {11: dict(W=14, n=3), 13: dict(W=16, n=3)}


def make_trainer(fov, E, seed=7, W=None, n=None, **kw):
    """A GPU Trainer on a W x W chip with n droplets (default: the golden's shape for this fov)."""
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.train import Trainer
    W, n = W or SHAPES[fov]['W'], n or SHAPES[fov]['n']
    env = VecDMFB(W, W, n, fov=fov, n_envs=E, seed=seed, device='cuda:0')
    args = make_args(device='cuda:0', n_envs=E, drop_num=n if n in (2, 3, 4, 5, 10) else 2, width=W, length=W, fov=fov, **kw,
                     **env.get_env_info())
    args.drop_num = n
    return Trainer(env, args)


def stream_replays_through_oracle(tr, fov, seed, K, early_ends):
    """small_fov_helpers.stream_replays_through_oracle for these shapes: K lock-steps of the continuous rollout at epsilon 1 (two
    calls: episodes straddle the boundary), the recorded actions replayed through the CPU oracle, every closed episode in the ring
    compared bit for bit.  The episode limits here (48 .. 64 steps) exceed K / 2, so a chip that never ends early closes ONE episode
    in K = 100 lock-steps: at least one closed episode per chip is required (the helper's `> E` holds with early ends only)."""
    from test_gpu_rollout_stream import _compare_ring, _oracle_episodes
    worker, buf, env, args = tr.rolloutWorker, tr.buffer, tr.env, tr.args
    E, n = env.n_envs, args.n_agents
    worker.epsilon = torch.tensor(1.0, device='cuda:0')
    worker.anneal_epsilon, worker.min_epsilon = 0.0, 0.0
    steps = []
    worker.stream_step_hook = lambda s, a, term: steps.append((a.cpu().numpy().copy(), term.cpu().numpy().copy()))
    acc = np.zeros(4, np.int64)
    for chunk in (K // 2, K - K // 2):
        acc += np.asarray(buf.sync_host(worker.generate_steps(buf, chunk)))
    cfg = dict(width=env.width, length=env.length, n_agents=n, fov=fov)
    want = _oracle_episodes(cfg, E, seed, steps, args.episode_limit, n, env.obs_len)
    print('fov %d %dx%d n %d: %d closed episodes on %d chips, limit %d' % (fov, env.width, env.length, n, len(want), E, args.episode_limit))
    assert len(want) == buf.host_closed == buf.current_size == acc[0]
    assert (acc[0] > E) if early_ends else (acc[0] >= E)
    lens = np.array([d['len'] for d in want])
    if early_ends:   # the case does exercise episodes that end before the step limit
        assert (lens < args.episode_limit).sum() >= 3 and len(set(lens.tolist())) >= 3, lens
    _compare_ring(buf, want)
    assert acc[1] == sum(d['stats'][1] for d in want) and acc[2] == sum(1 for d in want if d['stats'][3])


@pytest.mark.parametrize('name,fov', [('fovlearn_4d_od24_fov11.npz', 11), ('fovlearn_3d_od32_fov13.npz', 13)])
def test_packed_learn_matches_reference(name, fov, monkeypatch):
    """VDN.learn_packed on the HIP front end (forward and backward) against the reference's VDN.learn (tools/oracle/gen_vdn_golden.py:
    gen_learn), at the tolerances of the fov-9 packed test.  The eval network must go through the wide front end's autograd node."""
    from marl_dmfb_amd.network import base_net
    calls = []
    real = base_net._FrontWideTrain.apply
    monkeypatch.setattr(base_net._FrontWideTrain, 'apply', lambda *a: calls.append(a[2]) or real(*a))
    learn_golden_check(os.path.join(GOLDEN, name), 'cuda:0', rtol=1e-5, atol=1e-5, replay_dtypes=True, packed=True)
    assert calls and set(calls) == {fov}


@pytest.mark.parametrize('fov', [11, 13])
def test_dispatch_takes_the_hip_paths(fov):
    tr = make_trainer(fov, 64, batch_size=16, buffer_size=256)
    net = tr.agents.policy.eval_rnn
    probe = torch.zeros((1, tr.env.obs_len), dtype=torch.int8, device='cuda:0')
    assert net._hip_front() == fov and net._hip_geometry() is None
    with torch.enable_grad():
        assert net._hip_train_ok(probe)
    with torch.no_grad():
        assert net._hip_conv_ok(probe) and net.act_ok(probe)
    assert tr.stream and tr.rolloutWorker.stream_ok()


@pytest.mark.parametrize('fov', [11, 13])
@pytest.mark.parametrize('shape', ['one-droplet', 'golden'])
def test_stream_episodes_replay_through_the_oracle(fov, shape):
    """Uniform random play, 48 chips and 100 lock-steps: ONE droplet on a small chip (most episodes end early, at many lengths)
    and the golden's shape."""
    W, n = (ONE_DROPLET[fov], 1) if shape == 'one-droplet' else (SHAPES[fov]['W'], SHAPES[fov]['n'])
    tr = make_trainer(fov, 48, seed=11, W=W, n=n, buffer_size=1024)
    assert tr.stream
    stream_replays_through_oracle(tr, fov, 11, 100, early_ends=n == 1)


@pytest.mark.parametrize('fov', [11, 13])
def test_graph_rollout_equals_eager_rollout(fov):
    torch.manual_seed(5)
    a = make_trainer(fov, 128, seed=11, use_graph=False, batch_size=32, buffer_size=512, anneal_steps=20000)
    torch.manual_seed(5)
    b = make_trainer(fov, 128, seed=11, use_graph=True, batch_size=32, buffer_size=512, anneal_steps=20000)
    assert b.rolloutWorker.use_graph and not a.rolloutWorker.use_graph
    b.agents.policy.eval_rnn.load_state_dict(a.agents.policy.eval_rnn.state_dict())
    b.agents.policy.target_rnn.load_state_dict(a.agents.policy.target_rnn.state_dict())
    a.agents.policy.init_hidden(1)
    a.rolloutWorker._play(a.rolloutWorker.epsilon.clone(), False, True)   # the graph side's warm-up episode
    for rnd in range(2):
        ra = a.rolloutWorker.generate_episode()
        rb = b.rolloutWorker.generate_episode()
        for k in range(4):
            assert torch.equal(ra[k], rb[k]), ('stat', k, rnd)
        for key in ra[4]:
            assert torch.equal(ra[4][key], rb[4][key]), (key, rnd)
    a.agents.policy.init_hidden(1)
    a.rolloutWorker._play(0.0, True, False)
    ea = a.rolloutWorker._generate_episode()
    eb = b.rolloutWorker._generate_episode()
    for k in range(4):
        assert torch.equal(ea[k], eb[k]), ('eval stat', k)


@pytest.mark.parametrize('fov', [11, 13])
def test_short_training_run_improves_greedy_policy(fov):
    """512 chips, 60 rounds.  Direction only, no margin.  Measured on one MI355X: fov 11 (14x14) greedy reward -92.6 -> -7.3,
    constraint violations 110.1 -> 0.3; fov 13 (16x16) -104.2 -> -2.2, 120.9 -> 0.8."""
    E, rounds = 512, 60
    torch.manual_seed(0)
    W, n = TRAIN[fov]['W'], TRAIN[fov]['n']
    tr = make_trainer(fov, E, W=W, n=n, batch_size=256, train_time=4, buffer_size=8 * E, anneal_steps=E * 4 * W * rounds * 0.6)
    assert tr.stream
    r0, _, c0, _ = tr.rolloutWorker.evaluate(2)
    for _ in range(rounds):
        tr.collect_and_learn()
    r1, _, c1, _ = tr.rolloutWorker.evaluate(2)
    print('fov %d greedy reward %.1f -> %.1f, constraints %.1f -> %.1f' % (fov, r0, r1, c0, c1))
    assert torch.isfinite(tr.agents.policy.last_loss)
    assert r1 > r0, (r0, r1)
    assert c1 < c0, (c0, c1)
