"""The training loop at fov 7 (3 droplets) and fov 5 (4 droplets), the reference's field-of-view sweep (multiTrain.py), on the
HIP front end of include/crnn_fov.h: the learn against the reference's own numbers, the continuous rollout against the CPU
oracle, graph replay against eager play, and a short training run."""
import os

import pytest
import torch

from small_fov_helpers import make_trainer, stream_replays_through_oracle
from vdn_helpers import learn_golden_check

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.mark.parametrize('name,fov', [('fovlearn_3d_od32_fov7.npz', 7), ('fovlearn_4d_od24_fov5.npz', 5)])
def test_packed_learn_matches_reference(name, fov, monkeypatch):
    """VDN.learn_packed on the HIP front end (forward and backward) against the reference's VDN.learn (tools/oracle/gen_vdn_golden.py:
    gen_learn), at the tolerances of the fov-9 packed test.  The eval network must go through the HIP front end's autograd node."""
    from marl_dmfb_amd.network import base_net
    calls = []
    real = base_net._FrontFovTrain.apply
    monkeypatch.setattr(base_net._FrontFovTrain, 'apply', lambda *a: calls.append(a[2]) or real(*a))
    learn_golden_check(os.path.join(GOLDEN, name), 'cuda:0', rtol=1e-5, atol=1e-5, replay_dtypes=True, packed=True)
    assert calls and set(calls) == {fov}


@pytest.mark.parametrize('fov', [7, 5])
def test_dispatch_takes_the_hip_paths(fov):
    tr = make_trainer(fov, 64, batch_size=16, buffer_size=256)
    net = tr.agents.policy.eval_rnn
    probe = torch.zeros((1, tr.env.obs_len), dtype=torch.int8, device='cuda:0')
    assert net._hip_geometry() == fov
    with torch.enable_grad():
        assert net._hip_train_ok(probe)
    with torch.no_grad():
        assert net._hip_conv_ok(probe) and net.act_ok(probe)
    assert tr.stream and tr.rolloutWorker.stream_ok()


@pytest.mark.parametrize('fov', [7, 5])
@pytest.mark.parametrize('W,n', [(8, 1), (10, None)])
def test_stream_episodes_replay_through_the_oracle(fov, W, n):
    """Uniform random play: ONE droplet on an 8x8 chip (most episodes end early, at many lengths) and the sweep's shape (most run
    to the step limit)."""
    tr = make_trainer(fov, 48, seed=11, W=W, n=n, buffer_size=1024)
    assert tr.stream
    stream_replays_through_oracle(tr, fov, 11, 100, early_ends=n == 1)


@pytest.mark.parametrize('fov', [7, 5])
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


@pytest.mark.parametrize('fov', [7, 5])
def test_short_training_run_improves_greedy_policy(fov):
    E, rounds = 512, 60
    torch.manual_seed(0)
    tr = make_trainer(fov, E, batch_size=256, train_time=4, buffer_size=8 * E, anneal_steps=E * 40 * rounds * 0.6)
    assert tr.stream
    r0, _, c0, _ = tr.rolloutWorker.evaluate(2)
    for _ in range(rounds):
        tr.collect_and_learn()
    r1, _, c1, _ = tr.rolloutWorker.evaluate(2)
    print('fov %d greedy reward %.1f -> %.1f, constraints %.1f -> %.1f' % (fov, r0, r1, c0, c1))
    assert torch.isfinite(tr.agents.policy.last_loss)
    # the untrained greedy policy collides less at fov 5 (reward around -35 against -100 at fov 7 and 9): a smaller margin
    assert r1 > r0 + (40.0 if fov == 7 else 20.0), (r0, r1)
    assert c1 < 0.2 * c0 + 1.0, (c0, c1)
