"""QMIX on MEDA with the project's MEDA global state (args.meda_state, include/meda_vec.h): the Trainer, episode mode (graph replay
against eager play, padding included), the continuous rollout (args.stream_state: every closed episode's states against the
restatement along the CPU oracle's replay of it; graph replay against eager play across an evaluation), the fused mixing / TD block
at MEDA shapes, a short training run and a checkpoint round trip."""
import copy
import os

import numpy as np
import pytest
import torch

from test_gpu_meda_global_obs import numpy_meda_state
from test_gpu_qmix_ops import GRAD_TOL, _case, _fused, _reference64, _rel

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _trainer(E=256, W=30, L=30, n=4, seed=7, meda_state=True, **kw):
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.meda import VecMEDA
    from marl_dmfb_amd.train import Trainer
    env = VecMEDA(W, L, n, fov=19, n_envs=E, seed=seed, device=DEV, version=2)
    over = dict(batch_size=64, train_time=2, buffer_size=4 * E, anneal_steps=20000)
    over.update(kw)
    args = make_args(name='meda', drop_num=n, width=W, length=L, fov=19, alg='qmix', device=DEV, n_envs=E, meda_state=meda_state,
                     **over, **env.get_env_info())
    return Trainer(env, args)


# ---------------------------------------------------------------------------------------------------------- 1. setup
def test_trainer_builds_with_the_flag_and_refuses_without():
    tr = _trainer(E=64)
    S = 2 * 30 * 30
    assert tr.args.state_shape == S == tr.env.state_shape
    assert tr.buffer.states.shape == (tr.buffer.size, 61, S) and tr.buffer.states.dtype == torch.int8
    assert not tr.stream
    assert _trainer(E=64, W=45, L=30, n=4).buffer.states.shape[2] == 2 * 45 * 30
    with pytest.raises(ValueError, match='MEDA'):
        _trainer(E=64, meda_state=False)


# ---------------------------------------------------------------------------------------------------------- 2. episode mode
def test_episode_graphed_equals_eager_and_padding():
    torch.manual_seed(5)
    a = _trainer(use_graph=False)
    torch.manual_seed(5)
    b = _trainer(use_graph=True)
    assert not a.stream and not b.stream
    for k in ('eval_rnn', 'target_rnn', 'eval_qmix_net', 'target_qmix_net'):
        getattr(b.agents.policy, k).load_state_dict(getattr(a.agents.policy, k).state_dict())
    a.agents.policy.init_hidden(1)
    a.rolloutWorker._play(a.rolloutWorker.epsilon.clone(), False, True)   # the graph's warm-up episode
    for rnd in range(2):
        ea = a.rolloutWorker.generate_episode()[4]
        eb = b.rolloutWorker.generate_episode()[4]
        for k in ea:
            assert torch.equal(ea[k], eb[k]), (rnd, k)
        s, sn, pad = ea['s'], ea['s_next'], ea['padded'][:, :, 0]
        assert s.shape == (256, 60, 1800) and s.dtype == torch.int8
        assert bool((sn[pad] == 0).all()) and int((s[:, 1:][pad[:, :-1] | ea['terminated'][:, :-1, 0]]).abs().sum()) == 0
        valid_next = ~pad[:, 1:]
        assert torch.equal(sn[:, :-1][valid_next], s[:, 1:][valid_next])
        assert bool((s[:, 0].abs().sum(1) > 0).all())
        for tr, ep in ((a, ea), (b, eb)):
            tr.buffer.store_episode(ep)
            tr.buffer.generator = torch.Generator(device=DEV).manual_seed(rnd)
            tr.agents.train(tr.buffer.sample(64), rnd)


# ---------------------------------------------------------------------------------------------------------- 3. stream mode
def _stream(W, n, E, seed, buffer_size, L=None):
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.common.replay_buffer import ReplayBuffer
    from marl_dmfb_amd.common.rollout import RolloutWorker
    from marl_dmfb_amd.env.meda import VecMEDA
    L = L or W
    env = VecMEDA(W, L, n, fov=19, n_envs=E, seed=seed, device=DEV, version=2)
    args = make_args(name='meda', drop_num=n, width=W, length=L, fov=19, alg='qmix', device=DEV, n_envs=E, buffer_size=buffer_size,
                     state_shape=env.state_shape, meda_state=True, stream_state=True, **env.get_env_info())
    torch.manual_seed(seed)
    agents = Agents(args)
    worker = RolloutWorker(env, agents, args)
    return env, args, agents, worker, ReplayBuffer(args, device=DEV)


def _oracle_states(cfg, E, seed, steps, T):
    """The recorded (actions, terminated) of every lock-step replayed through the CPU oracle: (length, int8 (T + 1, S) state rows
    as the ring stores them) of every closed episode, in closing order (lock-step, then chip)."""
    from oracle.meda_oracle import MedaOracle  # the checker
    ora = MedaOracle(n_envs=E, seed=seed, **cfg)
    W, L = cfg['width'], cfg['length']

    def state():
        return numpy_meda_state(W, L, ora.get_state()['pos'], ora.get_task()[1]).reshape(E, -1)
    ora.reset()
    cur = state()
    rows = [[cur[e]] for e in range(E)]
    closed, overlaps = [], 0
    for acts, term_gpu in steps:
        _, dones, _, _ = ora.step(acts)
        cur = state()
        term = dones.all(axis=1)
        np.testing.assert_array_equal(term, term_gpu.astype(bool))
        pos = ora.get_state()['pos']
        d = np.abs(pos[:, :, None, :] - pos[:, None, :, :]).max(-1) + 99 * np.eye(pos.shape[1], dtype=np.int64)
        overlaps += int((d <= 4).any(axis=(1, 2)).sum())
        for e in range(E):
            rows[e].append(cur[e])
            if term[e]:
                st = np.zeros((T + 1, cur.shape[1]), np.int8)
                st[:len(rows[e])] = np.stack(rows[e])
                closed.append((len(rows[e]) - 1, st))
        if term.any():
            ora.reset(mask=term.astype(np.uint8))
            cur = state()
            for e in np.nonzero(term)[0]:
                rows[e] = [cur[e]]
    return closed, overlaps


@pytest.mark.parametrize('W,L,n,E,Ks', [(30, 30, 4, 48, (70, 61)), (45, 30, 4, 32, (80, 71))], ids=['30x30_4d', '45x30_4d'])
def test_stream_replays_through_the_meda_oracle(W, L, n, E, Ks):
    seed = 13
    env, args, agents, worker, buf = _stream(W, n, E, seed, buffer_size=8 * E, L=L)
    assert worker.stream_ok() and not worker._stream_state(buf).fused_reset
    worker.epsilon = torch.tensor(1.0, device=DEV)
    worker.anneal_epsilon, worker.min_epsilon = 0.0, 0.0
    T = args.episode_limit
    steps = []
    worker.stream_step_hook = lambda s, a, term: steps.append((a.cpu().numpy().copy(), term.cpu().numpy().copy()))
    acc = np.zeros(4, np.int64)
    for K in Ks:
        acc += np.asarray(buf.sync_host(worker.generate_steps(buf, K)))
    want, overlaps = _oracle_states(dict(width=W, length=L, n_agents=n, fov=19, version=2), E, seed, steps, T)
    assert len(want) == buf.host_closed == acc[0] >= 2 * E and len(want) <= buf.size
    assert overlaps > 0
    states = buf.states[:len(want)].cpu().numpy()
    lens = np.array([w[0] for w in want])
    np.testing.assert_array_equal(buf.host_len[:len(want)], lens)
    for k, (ln, st) in enumerate(want):
        np.testing.assert_array_equal(states[k], st, err_msg='states of slot %d (len %d)' % (k, ln))


def test_stream_graph_replay_equals_eager_play_across_an_evaluation():
    W, n, E, seed = 30, 4, 64, 9
    outs = []
    for graph in (False, True):
        env, args, agents, worker, buf = _stream(W, n, E, seed, buffer_size=4096)
        worker.use_graph = graph
        worker.epsilon = torch.tensor(0.3, device=DEV)
        worker.anneal_epsilon, worker.min_epsilon = 1e-5, 0.05
        accs = [buf.sync_host(worker.generate_steps(buf, K)) for K in (59, 60, 61)]
        worker.use_graph = False
        ev = worker.evaluate(1)
        worker.use_graph = graph
        accs += [buf.sync_host(worker.generate_steps(buf, K)) for K in (61, 59, 60)]
        if graph:
            assert sorted(worker._stream.graphs) == [59, 60, 61]
        outs.append((accs, ev, buf.states.clone(), {k: v.clone() for k, v in buf.buffers.items()}, buf.ring_len.clone(),
                     buf.ring_state.clone(), buf.ring_stats.clone(), worker._stream.s_stage.clone(), worker._stream.t_ep.clone()))
    a, b = outs
    assert a[0] == b[0] and a[1] == b[1], (a[0], b[0])
    closed = int(a[5][2])
    assert E * 4 <= closed < 4096
    assert torch.equal(a[2][:closed], b[2][:closed])
    assert bool((a[2][:closed, 0].abs().sum(1) > 0).all())
    for k in a[3]:
        assert torch.equal(a[3][k][:closed], b[3][k][:closed]), k
    assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]) and torch.equal(a[6].view(torch.int64), b[6].view(torch.int64))
    assert torch.equal(a[7], b[7]) and torch.equal(a[8], b[8])


# ---------------------------------------------------------------------------------------------------------- 4. fused mixer
@pytest.mark.parametrize('n,S,B,T', [(4, 1800, 256, 60), (10, 12800, 64, 40)], ids=['n4_S1800', 'n10_S12800'])
def test_fused_mix_td_at_meda_shapes(n, S, B, T):
    """The fused block (include/qmix_ops.h) at MEDA's shapes (9 actions, hyper_hidden_dim 32, 2 W L state entries) against float64
    autograd of QMixNet and the TD rule, with test_gpu_qmix_ops.py's tolerances."""
    args, ev, tg, st, batch, q_e, q_t = _case(n, 32, B, T, seed=n * 7 + 1, A=9, S=S)
    num64, gq64, g64 = _reference64(args, ev, tg, st, batch, q_e, q_t, T)
    num, gq, gw, bad = _fused(args, ev, tg, st, batch, q_e, q_t, T)
    assert abs(float(num) - float(num64)) <= 1e-5 * abs(float(num64))
    assert _rel(gq.cpu(), gq64) < GRAD_TOL, _rel(gq.cpu(), gq64)
    for k, ref in g64.items():
        assert _rel(gw[k].cpu(), ref) < GRAD_TOL, (k, _rel(gw[k].cpu(), ref))
    assert int(bad.item()) == 0


def test_one_learn_fused_against_torch_op_path():
    """One QMIX learn on a MEDA replay batch (30x30, 4 droplets: S = 1800) through the fused path and, from identical weights and
    the same batch, through the torch-op QMixNet path: the same loss (1e-5 relative, as test_gpu_qmix_ops.py) and the same Adam
    step.  The first Adam step is about lr * sign(gradient) per weight, so the two updates are compared at 1e-2 relative L2 (a
    gradient near zero may flip sign between two float32 summation orders); the gradients themselves are held to GRAD_TOL by
    test_fused_mix_td_at_meda_shapes."""
    torch.manual_seed(3)
    a = _trainer(E=256, use_graph=False)
    torch.manual_seed(3)
    b = _trainer(E=256, use_graph=False)
    pa, pb = a.agents.policy, b.agents.policy
    for k in ('eval_rnn', 'target_rnn', 'eval_qmix_net', 'target_qmix_net'):
        sa, sb = getattr(pa, k).state_dict(), getattr(pb, k).state_dict()
        assert all(torch.equal(sa[n_], sb[n_]) for n_ in sa), k
    for _ in range(2):
        a.buffer.store_episode(a.rolloutWorker.generate_episode()[4])
    a.buffer.generator = torch.Generator(device=DEV).manual_seed(0)
    batch = a.buffer.sample(128)
    T = int(batch['padded'].shape[1])
    assert pa._mix_fused_ok(batch)
    w0 = [p.detach().clone() for p in pa.eval_parameters]
    loss_f = float(pa.learn(batch, T, 1))
    pb._mix_fused_ok = lambda _b: False
    loss_t = float(pb.learn(batch, T, 1))
    assert abs(loss_f - loss_t) <= 1e-5 * abs(loss_t), (loss_f, loss_t)
    du_f = torch.cat([(p.detach() - q).flatten() for p, q in zip(pa.eval_parameters, w0)])
    du_t = torch.cat([(p.detach() - q).flatten() for p, q in zip(pb.eval_parameters, w0)])
    assert float(du_f.norm()) > 0
    assert _rel(du_t, du_f) < 1e-2, _rel(du_t, du_f)


# ---------------------------------------------------------------------------------------------------------- 5. training
def test_short_training_run_improves_greedy_policy():
    """30x30 / 4 droplets, 2048 chips, 120 rounds of 4 learns of 512 episodes, QMIX in the continuous rollout.  Observed on one
    MI355X: greedy reward -21.00 -> -6.33 (+14.7), constraints -42.96 -> -3.45 (+39.5), success 0.09.  The margins below are
    at most half of the observed improvement."""
    torch.manual_seed(0)
    rounds, E = 120, 2048
    tr = _trainer(E=E, batch_size=512, train_time=4, buffer_size=4 * E, anneal_steps=E * 60 * rounds * 0.5, stream_state=True)
    assert tr.stream
    r0, _, c0, _ = tr.rolloutWorker.evaluate(1)
    for _ in range(rounds):
        tr.collect_and_learn()
    r1, _, c1, ok = tr.rolloutWorker.evaluate(1)
    print('meda qmix greedy reward %.2f -> %.2f, constraints %.2f -> %.2f, success %.3f' % (r0, r1, c0, c1, ok))
    assert torch.isfinite(tr.agents.policy.last_loss)
    assert r1 > r0 + 7.0, (r0, r1)
    assert c1 > c0 + 19.0, (c0, c1)


def test_checkpoint_roundtrip_same_greedy_actions(tmp_path):
    from marl_dmfb_amd.agent.agent import Agents
    torch.manual_seed(1)
    tr = _trainer(E=128, model_dir=str(tmp_path))
    for _ in range(2):
        tr.collect_and_learn()
    tr.agents.policy.save_model(5)
    d = str(tmp_path) + '/qmix/fov19/'
    assert sorted(os.listdir(d)) == ['0_5_qmix_net_params.pkl', '0_5_rnn_net_params.pkl']
    args = copy.copy(tr.args)
    args.load_model, args.load_model_name = True, '0_5_'
    ag = Agents(args)
    for k, v in tr.agents.policy.eval_qmix_net.state_dict().items():
        assert torch.equal(v, ag.policy.eval_qmix_net.state_dict()[k])
    obs = tr.env.reset()
    E, n = obs.shape[:2]
    la = torch.zeros((E, n, 9), dtype=torch.int8, device=DEV)
    h = torch.zeros((E * n, 128), device=DEV)
    a1, _ = tr.agents.choose_actions(obs, la, h, 0.0, evaluate=True)
    a2, _ = ag.choose_actions(obs, la, h, 0.0, evaluate=True)
    assert torch.equal(a1, a2)
