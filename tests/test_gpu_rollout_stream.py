"""Continuous rollout (RolloutWorker.generate_steps; include/rollout_ops.h "stream" entry points): every chip plays on its own
clock, a finished episode is written into the replay ring on the device and the chip starts its next episode in the following
lock-step.

Each episode in the ring must be what the reference's generate_episode returns for that chip's task, actions and draws
(common/rollout.py:101-150 incl. the padding of :131-141): the test replays the recorded actions of every lock-step through the
CPU oracle (same Philox contract: same tasks, same move draws), closes and pads the episodes with the reference's rules on the
host, and compares every tensor of every ring slot bit for bit -- plus generate_episode's return values (reward, steps with the
failure inflation, constraints, success) and the trainer-facing counters."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CKPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'r04', 'degre', 'model')
CKPT_4D = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'r04', 'train_4d', '0_rnn_net_params.pkl')
KEYS = ['o', 'u', 'r', 'o_next', 'avail_u', 'avail_u_next', 'u_onehot', 'padded', 'terminated']


def _make(W, n, E, seed, buffer_size, trained=False, b_degrade=False, **over):
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.common.replay_buffer import ReplayBuffer
    from marl_dmfb_amd.common.rollout import RolloutWorker
    from marl_dmfb_amd.env.dmfb import VecDMFB
    kw = dict(b_degrade=True, per_degrade=1.0) if b_degrade else {}
    env = VecDMFB(W, W, n, fov=9, n_envs=E, seed=seed, device='cuda:0', **kw)
    args = make_args(drop_num=n if n in (2, 3, 4, 5, 10) else 2, width=W, length=W, fov=9, device='cuda:0', n_envs=E, buffer_size=buffer_size,
                     load_model=trained, load_model_name='0_', model_dir=CKPT, **env.get_env_info())
    args.__dict__.update(over)
    args.drop_num = n
    torch.manual_seed(seed)
    agents = Agents(args)
    worker = RolloutWorker(env, agents, args)
    return env, args, agents, worker, ReplayBuffer(args, device='cuda:0')


def _load_4d(agents):
    """The 10x10 / 4-droplet policy of profiles/r04/train_4d (97 % success, ~13 steps): episodes of many lengths."""
    sd = torch.load(CKPT_4D, map_location='cuda:0', weights_only=True)
    agents.policy.eval_rnn.load_state_dict(sd)


class _ChipOracles:
    """One DmfbOracle per chip (env_id0 = chip: the same draws as chip e of a batch) so that a step can leave chips out, as
    VecDMFB.step(active=...) does: a frozen chip is not stepped and reports terminated."""

    def __init__(self, E, seed, **cfg):
        from oracle.dmfb_oracle import DmfbOracle  # the checker
        self.o = [DmfbOracle(n_envs=1, seed=seed, env_id0=e, **cfg) for e in range(E)]
        self.n = cfg['n_agents']

    def reset(self, mask=None, new=False):
        for e, o in enumerate(self.o):
            if mask is None or mask[e]:
                o.reset(new=new)

    def restart(self, mask=None):
        for e, o in enumerate(self.o):
            if mask is None or mask[e]:
                o.restart()

    def step(self, acts, active=None, record=True):
        E, n = len(self.o), self.n
        rew, dones = np.zeros((E, n)), np.ones((E, n), np.uint8)
        cons, succ = np.zeros(E, np.int32), np.zeros(E, np.uint8)
        for e, o in enumerate(self.o):
            if active is None or active[e]:
                r, d, c, s_ = o.step(acts[e:e + 1], record=record)
                rew[e], dones[e], cons[e], succ[e] = r[0], d[0], c[0], s_[0]
        return rew, dones, cons, succ

    def observe(self):
        return np.concatenate([o.observe() for o in self.o])


def _logged(env, calls):
    """Wrap the env instance's reset / restart / step: their arguments (and step's terminated flags) go into `calls`."""
    host = lambda t: None if t is None else t.cpu().numpy().copy()
    cls = type(env)

    def reset(mask=None, new=False, obs=None):
        calls.append(('reset', host(mask), bool(new)))
        return cls.reset(env, mask=mask, new=new, obs=obs)

    def restart(mask=None, obs=None):
        calls.append(('restart', host(mask)))
        return cls.restart(env, mask=mask, obs=obs)

    def step(actions, uniforms=None, record=True, autoreset=False, active=None, out=None):
        assert uniforms is None and not autoreset and out is None
        res = cls.step(env, actions, record=record, active=active)
        calls.append(('step', host(actions), host(active), bool(record), host(res[3]['terminated'])))
        return res
    env.reset, env.restart, env.step = reset, restart, step


def _oracle_episodes(cfg, E, seed, steps, T, n, O, A=5, meda=False, ora=None):
    """Replay the recorded (lock-step -> actions) through the CPU oracle; returns the closed episodes in closing order
    (lock-step, then chip) as padded dicts + generate_episode's return values.  An entry {'calls': [...]} of `steps` is what
    something else (an evaluation) did with the env between two stream segments (_logged); it is replayed, then the stream
    restarts: every chip reset, the episodes in flight dropped."""
    if ora is not None:
        pass
    elif meda:
        from oracle.meda_oracle import MedaOracle  # the checker
        ora = MedaOracle(n_envs=E, seed=seed, **cfg)
    else:
        from oracle.dmfb_oracle import DmfbOracle  # the checker
        ora = DmfbOracle(n_envs=E, seed=seed, **cfg)
    ora.reset()
    obs = ora.observe()
    open_eps = [dict(o=[], u=[], r=[], o_next=[], cons=0, succ=0) for _ in range(E)]
    closed = []
    for item in steps:
        if isinstance(item, dict):
            for c in item['calls']:
                if c[0] == 'reset':
                    ora.reset(mask=c[1], new=c[2])
                elif c[0] == 'restart':
                    ora.restart(mask=c[1])
                else:
                    _, acts, active, record, term_gpu = c
                    _, dones, _, _ = ora.step(acts, active=active, record=record)
                    np.testing.assert_array_equal(dones.all(axis=1), term_gpu.astype(bool))
            ora.reset()
            obs = ora.observe()
            open_eps = [dict(o=[], u=[], r=[], o_next=[], cons=0, succ=0) for _ in range(E)]
            continue
        acts, term_gpu = item
        rew, dones, cons, succ = ora.step(acts)
        nxt = ora.observe()
        term = dones.all(axis=1)
        np.testing.assert_array_equal(term, term_gpu.astype(bool))
        for e in range(E):
            ep = open_eps[e]
            ep['o'].append(obs[e].copy()); ep['o_next'].append(nxt[e].copy()); ep['u'].append(acts[e].copy())
            ep['r'].append(np.sum(rew[e]) / n)           # rollout.py:33 (numpy's summation order)
            ep['cons'] += (float(cons[e]) if meda else int(cons[e])); ep['succ'] += int(succ[e])   # MEDA: the (float) sum of punishments
            if term[e]:
                ln = len(ep['r'])
                d = {'o': np.zeros((T, n, O), np.int8), 'o_next': np.zeros((T, n, O), np.int8), 'u': np.zeros((T, n, 1), np.int8),
                     'r': np.zeros((T, 1), np.float32), 'avail_u': np.zeros((T, n, A), np.int8), 'avail_u_next': np.zeros((T, n, A), np.int8),
                     'u_onehot': np.zeros((T, n, A), np.int8), 'padded': np.ones((T, 1), bool), 'terminated': np.ones((T, 1), bool)}
                d['o'][:ln], d['o_next'][:ln] = np.stack(ep['o']), np.stack(ep['o_next'])
                d['u'][:ln, :, 0] = np.stack(ep['u'])
                d['u_onehot'][:ln] = np.eye(A, dtype=np.int8)[np.stack(ep['u'])]
                d['r'][:ln, 0] = np.asarray(ep['r'], np.float64).astype(np.float32)
                d['avail_u'][:ln] = 1; d['avail_u_next'][:ln] = 1
                d['padded'][:ln] = False; d['terminated'][:ln - 1] = False
                total = 0.0
                for v in ep['r']:
                    total += v                              # reward += experience.r[0] (rollout.py:122)
                d['stats'] = (total, ln if ep['succ'] else T, ep['cons'], ep['succ'])
                d['len'] = ln
                closed.append(d)
                open_eps[e] = dict(o=[], u=[], r=[], o_next=[], cons=0, succ=0)
        if term.any():
            ora.reset(mask=term.astype(np.uint8))
            obs = ora.observe()
        else:
            obs = nxt
    return closed


@pytest.mark.parametrize('case', ['random_1d', 'trained_10d', 'trained_10d_degrade', 'bench_4d', 'bench_4d_unfused', 'bench_4d_split'])
def test_stream_episodes_replay_through_the_oracle(case, monkeypatch):
    if case == 'random_1d':      # uniform random play of ONE droplet on a small chip (a 245-byte row: the byte path of the close
        W, n, E, K, trained, eps, deg = 9, 1, 40, 150, False, 1.0, False     # kernel): most episodes time out, some end early
    elif case.startswith('bench'):   # the BENCH shape (10x10, 4 droplets, fov 9: 980-byte rows, 40 x 245 words -> the per-chip
        W, n, E, K, trained, eps, deg = 10, 4, 64, 100, False, 0.05, False   # dword form of the close) under the 4-droplet policy
    else:                        # the 20x20 / 10-droplet policy of profiles/r04/degre (73 % success): lengths 10..80
        W, n, E, K, trained, eps, deg = 20, 10, 24, 170, True, 0.05, case.endswith('degrade')
    if case == 'bench_4d_split':     # the env's split launches (every DMFB run at E >= split_min): no terminal-observation
        monkeypatch.setenv('DMFB_VEC_SPLIT_MIN_ENVS', '1')               # output, the reset follows the stream step
    seed = 11
    env, args, agents, worker, buf = _make(W, n, E, seed, buffer_size=1024, trained=trained, b_degrade=deg)
    if case.startswith('bench'):
        _load_4d(agents)
    if case == 'bench_4d_unfused':
        worker.stream_fused_reset = False
    if case.startswith('bench'):
        assert worker._stream_state(buf).fused_reset == (case == 'bench_4d')
    worker.epsilon = torch.tensor(eps, device='cuda:0')
    worker.anneal_epsilon, worker.min_epsilon = 0.0, 0.0
    T, O = args.episode_limit, env.obs_len
    steps = []
    worker.stream_step_hook = lambda s, a, term: steps.append((a.cpu().numpy().copy(), term.cpu().numpy().copy()))
    acc = np.zeros(4, np.int64)
    for chunk in (K // 2, K - K // 2):      # two calls: episodes straddle the call boundary
        acc += np.asarray(buf.sync_host(worker.generate_steps(buf, chunk)))
    cfg = dict(width=W, length=W, n_agents=n, fov=9)
    if deg:
        cfg.update(b_degrade=True, per_degrade=1.0)
    want = _oracle_episodes(cfg, E, seed, steps, T, n, O)
    assert len(want) == buf.host_closed == buf.current_size == acc[0] > E
    lens = np.array([d['len'] for d in want])
    assert (lens < T).sum() >= 3 and len(set(lens.tolist())) >= 3, lens     # the case does exercise early ends
    _compare_ring(buf, want)
    assert acc[1] == sum(d['stats'][1] for d in want) and acc[2] == sum(1 for d in want if d['stats'][3]) and acc[3] == E * K


def _compare_ring(buf, want):
    """Slots 0 .. len(want) - 1 of the ring against the oracle's episodes, every tensor and the statistics bit for bit."""
    lens = np.array([d['len'] for d in want])
    np.testing.assert_array_equal(buf.host_len[:len(want)], lens)
    got = {k: buf.buffers[k][:len(want)].cpu().numpy() for k in KEYS}
    stats = buf.ring_stats[:len(want)].cpu().numpy()
    for k, d in enumerate(want):
        for key in KEYS:
            np.testing.assert_array_equal(got[key][k].reshape(d[key].shape), d[key], err_msg='slot %d key %s (len %d)' % (k, key, d['len']))
        np.testing.assert_array_equal(stats[k].view(np.int64), np.asarray(d['stats'], np.float64).view(np.int64), err_msg='stats of slot %d' % k)


def test_stream_restart_after_an_evaluation_replays_through_the_oracle():
    """A greedy evaluation between two stream segments (eager: the step hook keeps graphs off): everything the evaluation did
    with the env is logged and replayed through per-chip oracles, then the stream restarts from a reset of every chip.  The
    episodes closed before and after the restart must be the reference's, bit for bit."""
    W, n, E, seed = 10, 4, 48, 21
    env, args, agents, worker, buf = _make(W, n, E, seed, buffer_size=1024)
    _load_4d(agents)
    worker.epsilon = torch.tensor(0.05, device='cuda:0')
    worker.anneal_epsilon, worker.min_epsilon = 0.0, 0.0
    T, O = args.episode_limit, env.obs_len
    steps = []
    worker.stream_step_hook = lambda s, a, term: steps.append((a.cpu().numpy().copy(), term.cpu().numpy().copy()))
    acc = np.zeros(4, np.int64)
    for K in (30, 25):
        acc += np.asarray(buf.sync_host(worker.generate_steps(buf, K)))
    before = int(acc[0])
    calls = []
    _logged(env, calls)
    worker.evaluate(1)
    del env.reset, env.restart, env.step
    assert [c[0] for c in calls[:2]] == ['reset', 'step'] and len(calls) > 10
    assert any(c[2] is not None and not c[2].all() for c in calls if c[0] == 'step')   # chips froze after finishing early
    steps.append({'calls': calls})
    for K in (45, 20):
        acc += np.asarray(buf.sync_host(worker.generate_steps(buf, K)))
    want = _oracle_episodes(dict(width=W, length=W, n_agents=n, fov=9), E, seed, steps, T, n, O, ora=_ChipOracles(E, seed, width=W, length=W, n_agents=n, fov=9))
    assert len(want) == buf.host_closed == acc[0] and len(want) - before >= E     # every chip closed after the restart
    assert acc[3] == E * (30 + 25 + 45 + 20)
    _compare_ring(buf, want)
    assert acc[1] == sum(d['stats'][1] for d in want) and acc[2] == sum(1 for d in want if d['stats'][3])


def test_stream_graph_replay_equals_eager_play_across_an_evaluation():
    """The restart after an evaluation happens under graph replay too: rounds of 39, 40 and 41 lock-steps (three cached graphs,
    the odd ones with the copy-back of the double buffers), a greedy evaluation, then the same cached graphs again.  Ring,
    statistics, counters and epsilon equal the eager play bit for bit.  The evaluation itself is played eagerly in both runs:
    the first graphed evaluation plays an extra warm-up episode before its capture, which would move the env on."""
    W, n, E, seed = 10, 4, 64, 9
    outs = []
    for graph in (False, True):
        env, args, agents, worker, buf = _make(W, n, E, seed, buffer_size=4096)
        _load_4d(agents)
        worker.use_graph = graph
        worker.epsilon = torch.tensor(0.3, device='cuda:0')
        worker.anneal_epsilon, worker.min_epsilon = 1e-5, 0.05
        accs = [buf.sync_host(worker.generate_steps(buf, K)) for K in (39, 40, 41)]
        worker.use_graph = False
        ev = worker.evaluate(1)
        worker.use_graph = graph
        accs += [buf.sync_host(worker.generate_steps(buf, K)) for K in (41, 39, 40, 41)]
        if graph:
            assert sorted(worker._stream.graphs) == [39, 40, 41]
        outs.append((accs, ev, {k: v.clone() for k, v in buf.buffers.items()}, buf.ring_len.clone(), buf.ring_state.clone(),
                     buf.ring_stats.clone(), float(worker.epsilon), worker._stream.t_ep.clone(), worker._stream.started))
    a, b = outs
    assert a[0] == b[0] and a[1] == b[1], (a[0], b[0])
    closed = int(a[4][2])
    assert E * 6 < closed < 4096                    # nothing overwritten: every episode of both runs is compared
    for k in a[2]:                                  # (the slots behind them were never written: torch.empty)
        assert torch.equal(a[2][k][:closed], b[2][k][:closed]), k
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and torch.equal(a[5].view(torch.int64), b[5].view(torch.int64))
    assert a[6] == b[6] and torch.equal(a[7], b[7]) and a[8] and b[8]


def test_stream_refuses_a_ring_smaller_than_the_batch():
    """Every chip may close in the same lock-step (after a restart every chip that does not finish times out together): a ring of
    fewer slots than chips would map two closes onto one slot.  The episode path raises for the same case."""
    env, args, agents, worker, buf = _make(10, 4, 64, 1, buffer_size=63)
    with pytest.raises(ValueError, match='smaller than the batch'):
        worker.generate_steps(buf, 1)
    env, args, agents, worker, buf = _make(10, 4, 64, 1, buffer_size=64)   # S == n_envs is the smallest legal ring
    assert buf.sync_host(worker.generate_steps(buf, 40))[3] == 64 * 40


def test_trainer_above_the_stream_limit_plays_episodes():
    """Past ROLLOUT_STREAM_MAX_ENVS chips the continuous rollout does not apply: the Trainer keeps the episode-per-round form."""
    from marl_dmfb_amd import _lib
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.train import Trainer
    E = _lib.ROLLOUT_STREAM_MAX_ENVS + 1
    torch.manual_seed(0)
    env = VecDMFB(10, 10, 4, fov=9, n_envs=E, seed=3, device='cuda:0')
    args = make_args(device='cuda:0', n_envs=E, batch_size=64, train_time=1, buffer_size=E, **env.get_env_info())
    tr = Trainer(env, args)
    assert tr.rolloutWorker.use_graph and not tr.rolloutWorker.stream_ok() and not tr.stream
    played = tr.collect_and_learn()
    assert E <= played <= E * 40 and tr.buffer.current_size == E and tr.trained_times == 1


def test_stream_graph_replay_equals_eager_play():
    """The captured graph of a round and the eager launches write the same ring, bit for bit, over several rounds with the ring
    wrapping around; epsilon anneals alike."""
    W, n, E, seed = 10, 4, 64, 5
    outs = []
    for graph in (False, True):
        env, args, agents, worker, buf = _make(W, n, E, seed, buffer_size=160)
        worker.use_graph = graph
        worker.epsilon = torch.tensor(0.9, device='cuda:0')
        worker.anneal_epsilon, worker.min_epsilon = 1e-5, 0.05
        accs = [buf.sync_host(worker.generate_steps(buf, 40)) for _ in range(4)]
        outs.append((accs, {k: v.clone() for k, v in buf.buffers.items()}, buf.ring_len.clone(), buf.ring_state.clone(),
                     buf.ring_stats.clone(), float(worker.epsilon)))
    a, b = outs
    assert a[0] == b[0] and a[0][0][0] >= E          # every chip closed at least one episode per round of episode_limit lock-steps
    assert int(a[3][2]) > 160                        # the ring wrapped
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and a[5] == b[5]
    assert abs(a[5] - (0.9 - 1e-5 * E * 160)) < 1e-4


def test_trainer_in_stream_mode_learns_and_counts():
    """Trainer.collect_and_learn in continuous mode: a round is episode_limit lock-steps with every chip playing, the learns get
    their exact length from the host-side draw, time_steps follows the failure-inflated count, and the loop does learn."""
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.train import Trainer
    E = 1024
    torch.manual_seed(0)
    env = VecDMFB(10, 10, 4, fov=9, n_envs=E, seed=7, device='cuda:0')
    rounds = 120
    args = make_args(device='cuda:0', n_envs=E, batch_size=256, train_time=4, buffer_size=8 * E, anneal_steps=E * 40 * rounds * 0.6,
                     **env.get_env_info())
    tr = Trainer(env, args)
    assert tr.stream
    r0, s0, c0, ok0 = tr.rolloutWorker.evaluate(1)
    seen = 0
    for k in range(rounds):
        played = tr.collect_and_learn()
        assert played == E * 40
        assert tr.last_round['episodes'] >= E
        seen += tr.last_round['steps_inflated']
    assert tr.time_steps == seen and tr.trained_times == 4 * rounds
    r1, s1, c1, ok1 = tr.rolloutWorker.evaluate(1)
    assert r1 > r0 + 30 and c1 < c0 * 0.2, (r0, c0, r1, c1)
    assert tr.buffer.current_size == 8 * E and int(tr.buffer.ring_state[2]) == tr.buffer.host_closed
    resets = []                 # the observation every full reset leaves (the stream's restart is one)

    def reset(mask=None, new=False, obs=None):
        out = type(env).reset(env, mask=mask, new=new, obs=obs)
        if mask is None:
            resets.append(out.clone())
        return out
    env.reset = reset
    cursor0, closed0 = (int(v) for v in tr.buffer.ring_state[[0, 2]])
    tr.collect_and_learn()   # the evaluation reset every chip: the stream restarts cleanly
    del env.reset
    assert tr.last_round['played'] == E * 40
    # The round after the restart: every chip started its first episode in its first lock-step, so the episodes closed in the round
    # plus the steps of the ones in flight are exactly E x 40 lock-steps (an episode carried over from before the evaluation would
    # add its earlier steps), and each chip's first episode begins with the observation of the reset.
    assert len(resets) == 1, 'the stream did not reset the chips after the evaluation'
    n_new = int(tr.buffer.ring_state[2]) - closed0
    assert n_new == tr.last_round['episodes'] and E <= n_new <= tr.buffer.size
    slots = (cursor0 + torch.arange(n_new, device='cuda:0')) % tr.buffer.size
    st = tr.rolloutWorker._stream
    assert int(tr.buffer.ring_len[slots].sum()) + int(st.t_ep[0].sum()) == E * 40
    w = torch.randint(1, 1 << 20, (4 * env.obs_len,), device='cuda:0', dtype=torch.int64)
    first = (tr.buffer.buffers['o'][slots, 0].reshape(n_new, -1).to(torch.int64) * w).sum(1)
    reset_rows = (resets[0].reshape(E, -1).to(torch.int64) * w).sum(1)
    assert bool(torch.isin(reset_rows, first).all()), 'an episode of the round does not start from the reset'


def test_stream_episodes_replay_through_the_meda_oracle():
    """The same for MEDA (30x30, 4 droplets, v0_2 observation, fov-19 network: 4 340-byte rows, episodes of 60 steps closed by all
    workgroups together; the env has no terminal-observation output, so the reset follows the stream step as its own call)."""
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.common.replay_buffer import ReplayBuffer
    from marl_dmfb_amd.common.rollout import RolloutWorker
    from marl_dmfb_amd.env.meda import VecMEDA
    W, n, E, K, seed = 30, 4, 20, 150, 3
    env = VecMEDA(W, W, n, fov=19, n_envs=E, seed=seed, device='cuda:0', version=2)
    args = make_args(name='meda', drop_num=n, width=W, length=W, fov=19, device='cuda:0', n_envs=E, buffer_size=256, **env.get_env_info())
    torch.manual_seed(seed)
    worker = RolloutWorker(env, Agents(args), args)
    buf = ReplayBuffer(args, device='cuda:0')
    assert worker.stream_ok()
    worker.epsilon = torch.tensor(1.0, device='cuda:0')
    worker.anneal_epsilon, worker.min_epsilon = 0.0, 0.0
    T, O, A = args.episode_limit, env.obs_len, args.n_actions
    steps = []
    worker.stream_step_hook = lambda s, a, term: steps.append((a.cpu().numpy().copy(), term.cpu().numpy().copy()))
    acc = np.zeros(4, np.int64)
    for chunk in (K // 2, K - K // 2):
        acc += np.asarray(buf.sync_host(worker.generate_steps(buf, chunk)))
    want = _oracle_episodes(dict(width=W, length=W, n_agents=n, fov=19, version=2), E, seed, steps, T, n, O, A=A, meda=True)
    assert len(want) == buf.host_closed == acc[0] >= 2 * E
    lens = np.array([d['len'] for d in want])
    assert (lens < T).sum() >= 1, lens
    np.testing.assert_array_equal(buf.host_len[:len(want)], lens)
    got = {k: buf.buffers[k][:len(want)].cpu().numpy() for k in KEYS}
    stats = buf.ring_stats[:len(want)].cpu().numpy()
    for k, d in enumerate(want):
        for key in KEYS:
            np.testing.assert_array_equal(got[key][k].reshape(d[key].shape), d[key], err_msg='slot %d key %s (len %d)' % (k, key, d['len']))
        np.testing.assert_array_equal(stats[k].view(np.int64), np.asarray(d['stats'], np.float64).view(np.int64), err_msg='stats of slot %d' % k)
