"""QMIX in the continuous rollout (args.stream_state): the env stages every chip's global state while its episode runs and copies
it into the replay ring's state tensor when the episode closes (include/dmfb_vec.h: dmfb_vec_global_obs_stage_first / _close).

  * the two entry points against a numpy restatement of the header contract, bit for bit, over batch sizes, state lengths,
    closing patterns and the argument checks;
  * eager stream rounds replayed through the CPU oracle: every ring slot, the state included, is the reference's episode;
  * graph replay equals eager play across an evaluation and restart;
  * the Trainer picks stream mode with the flag (and learns), and nothing changes without it or for VDN."""
import os

import numpy as np
import pytest
import torch

from test_gpu_dmfb_global_obs import numpy_state

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CKPT_4D = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'r04', 'train_4d', '0_rnn_net_params.pkl')
KEYS = ['o', 'u', 'r', 'o_next', 'avail_u', 'avail_u_next', 'u_onehot', 'padded', 'terminated']


def _env_state(env):
    pos = env.get_state()['pos'].cpu().numpy()
    ends = env.get_task()[1].cpu().numpy()
    blocks = env.get_blocks().cpu().numpy() if env.n_blocks else np.zeros((env.n_envs, 0, 4), np.int32)
    return numpy_state(env.width, env.length, pos, ends, blocks).reshape(env.n_envs, -1)


def _rand_bytes(shape, gen):
    return torch.randint(-128, 128, shape, dtype=torch.int8, device=DEV, generator=gen)


# ---------------------------------------------------------------------------------------------------------- 1. the kernels
@pytest.mark.parametrize('E', [1, 63, 64, 65, 4096, 32768])
@pytest.mark.parametrize('W,n,nb,T', [(5, 2, 0, 6), (10, 4, 0, 5), (12, 3, 2, 3)])
def test_stage_and_close_against_restatement(E, W, n, nb, T):
    """stage_first with a random mask, one random step, then stage_close with synthetic step indices (t = T - 1 included) and
    three closing patterns: a sparse random set, none, and every chip at once into a ring of exactly E slots about to wrap.
    S = 75 (not a multiple of 4), 300, 432; stage / slot rows of 525, 1800, 1728 bytes: 16-byte, 4-byte and byte copies."""
    from marl_dmfb_amd.env.dmfb import VecDMFB
    env = VecDMFB(W, W, n, nb, fov=3, n_envs=E, seed=E + W, device=DEV)
    env.reset(new=True)
    S = env.state_shape
    gen = torch.Generator(device=DEV).manual_seed(E * 7 + W)
    stage = _rand_bytes((E, T + 1, S), gen)
    mask = (torch.rand(E, device=DEV, generator=gen) < 0.5).to(torch.uint8)
    want = stage.cpu().numpy()
    st0 = _env_state(env)
    env.global_obs_stage_first(mask, stage)
    m = mask.cpu().numpy().astype(bool)
    want[m, 0] = st0[m]
    np.testing.assert_array_equal(stage.cpu().numpy(), want)
    env.step(torch.randint(0, 5, (E, n), device=DEV, generator=gen, dtype=torch.int32))
    st1 = _env_state(env)
    for pattern in ('sparse', 'none', 'all_wrap'):
        slots = E if pattern == 'all_wrap' else E + 5
        ring = _rand_bytes((slots, T + 1, S), gen)
        t_ep = torch.randint(0, T, (E,), device=DEV, generator=gen, dtype=torch.int32)
        t_ep[::3] = T - 1                                      # episodes of length T
        if pattern == 'sparse':
            close = torch.full((E,), -1, dtype=torch.int32, device=DEV)
            pick = torch.rand(E, device=DEV, generator=gen) < 0.2
            pick[-1] = True
            close[pick] = torch.randperm(slots, device=DEV, generator=gen)[:int(pick.sum())].to(torch.int32)
        elif pattern == 'none':
            close = torch.full((E,), -1, dtype=torch.int32, device=DEV)
        else:
            close = ((E - 3 + torch.arange(E, device=DEV)) % E).to(torch.int32)
        want_st, want_ring = stage.cpu().numpy(), ring.cpu().numpy()
        te, cs = t_ep.cpu().numpy(), close.cpu().numpy()
        want_st[np.arange(E), te + 1] = st1
        for e in np.nonzero(cs >= 0)[0]:
            want_ring[cs[e], :te[e] + 2] = want_st[e, :te[e] + 2]
            want_ring[cs[e], te[e] + 2:] = 0
        env.global_obs_stage_close(t_ep, close, stage, ring)
        np.testing.assert_array_equal(stage.cpu().numpy(), want_st, err_msg=pattern)
        np.testing.assert_array_equal(ring.cpu().numpy(), want_ring, err_msg=pattern)


def test_close_multi_chunk_misaligned_and_out_of_range():
    """A 35 100-byte row (three grid work items per chip), a ring one byte off 4-byte alignment (the byte path), and device-side
    values outside the contract: step indices -1 / T and slots >= slots are skipped, nothing else is written."""
    from marl_dmfb_amd.env.dmfb import VecDMFB
    E, W, n, T = 65, 30, 4, 12
    env = VecDMFB(W, W, n, fov=9, n_envs=E, seed=4, device=DEV)
    env.reset(new=True)
    S = env.state_shape
    gen = torch.Generator(device=DEV).manual_seed(3)
    for offset in (0, 1):
        slots = E + 2
        stage = _rand_bytes((E, T + 1, S), gen)
        flat = _rand_bytes((slots * (T + 1) * S + 16,), gen)
        ring = flat[offset:offset + slots * (T + 1) * S].view(slots, T + 1, S)
        t_ep = torch.randint(0, T, (E,), device=DEV, generator=gen, dtype=torch.int32)
        close = torch.randperm(slots, device=DEV, generator=gen)[:E].to(torch.int32)
        t_ep[0], t_ep[1], close[2], close[3], close[4] = -1, T, slots, 1 << 30, -7
        want_st, want_flat = stage.cpu().numpy(), flat.cpu().numpy()
        want_ring = want_flat[offset:offset + slots * (T + 1) * S].reshape(slots, T + 1, S)
        te, cs, st = t_ep.cpu().numpy(), close.cpu().numpy(), _env_state(env)
        for e in range(E):
            if 0 <= te[e] < T:
                want_st[e, te[e] + 1] = st[e]
                if 0 <= cs[e] < slots:
                    want_ring[cs[e], :te[e] + 2] = want_st[e, :te[e] + 2]
                    want_ring[cs[e], te[e] + 2:] = 0
        env.global_obs_stage_close(t_ep, close, stage, ring)
        np.testing.assert_array_equal(stage.cpu().numpy(), want_st)
        np.testing.assert_array_equal(flat.cpu().numpy(), want_flat, err_msg='offset %d' % offset)


def test_bad_arguments_are_refused_before_any_launch():
    from marl_dmfb_amd.env.dmfb import VecDMFB
    E, T = 8, 4
    env = VecDMFB(10, 10, 2, fov=3, n_envs=E, seed=1, device=DEV)
    S = env.state_shape
    stage = torch.full((E, T + 1, S), 5, dtype=torch.int8, device=DEV)
    ring = torch.full((E, T + 1, S), 6, dtype=torch.int8, device=DEV)
    t_ep = torch.zeros(E, dtype=torch.int32, device=DEV)
    close = torch.zeros(E, dtype=torch.int32, device=DEV)
    lib, h, null = env.lib, env.h, None
    p = lambda t: t.data_ptr()
    first = [(h, null, 0, p(stage), null), (h, null, -1, p(stage), null), (h, null, T, null, null), (null, null, T, p(stage), null)]
    close_ = [(h, null, p(close), T, p(stage), p(ring), E, null), (h, p(t_ep), null, T, p(stage), p(ring), E, null),
              (h, p(t_ep), p(close), T, null, p(ring), E, null), (h, p(t_ep), p(close), T, p(stage), null, E, null),
              (null, p(t_ep), p(close), T, p(stage), p(ring), E, null), (h, p(t_ep), p(close), 0, p(stage), p(ring), E, null),
              (h, p(t_ep), p(close), T, p(stage), p(ring), E - 1, null)]
    for a in first:
        with pytest.raises(ValueError):
            lib.dmfb_vec_global_obs_stage_first(*a)
    for a in close_:
        with pytest.raises(ValueError):
            lib.dmfb_vec_global_obs_stage_close(*a)
    big = VecDMFB(150, 150, 2, fov=3, n_envs=1, seed=1, device=DEV)   # 67 500-byte state rows: over the 64 KiB limit
    with pytest.raises(ValueError):
        big.global_obs_stage_first(None, stage[:1])
    with pytest.raises(ValueError):
        big.global_obs_stage_close(t_ep[:1], close[:1], stage[:1], ring[:1])
    torch.cuda.synchronize()
    assert bool((stage == 5).all()) and bool((ring == 6).all())
    one = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    one[3] = 2
    lib.dmfb_vec_global_obs_stage_close(h, p(t_ep), p(one), T, p(stage), p(ring), E, null)   # a legal call does write
    torch.cuda.synchronize()
    assert not bool((ring == 6).all())


# ---------------------------------------------------------------------------------------------------------- 2. oracle replay
def _make(W, n, E, seed, buffer_size, nb=0, alg='qmix', **over):
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.common.replay_buffer import ReplayBuffer
    from marl_dmfb_amd.common.rollout import RolloutWorker
    from marl_dmfb_amd.env.dmfb import VecDMFB
    env = VecDMFB(W, W, n, nb, fov=9, n_envs=E, seed=seed, device=DEV)
    args = make_args(drop_num=n, width=W, length=W, fov=9, alg=alg, device=DEV, n_envs=E, buffer_size=buffer_size, block_num=nb,
                     state_shape=env.state_shape, stream_state=True, **env.get_env_info())
    args.__dict__.update(over)
    torch.manual_seed(seed)
    agents = Agents(args)
    worker = RolloutWorker(env, agents, args)
    return env, args, agents, worker, ReplayBuffer(args, device=DEV)


def _load_4d(agents):
    agents.policy.eval_rnn.load_state_dict(torch.load(CKPT_4D, map_location=DEV, weights_only=True))


def _oracle_state(ora):
    return numpy_state(ora.W, ora.L, ora.get_state()['pos'], ora.get_task()[1], ora.get_blocks()).reshape(ora.E, -1)


def _oracle_episodes(cfg, E, seed, steps, T, n, O, A=5):
    """The recorded (actions, terminated) of every lock-step replayed through the CPU oracle: the closed episodes in closing order
    (lock-step, then chip), padded by the reference's rules, with their global state as the ring stores it (T + 1 rows)."""
    from oracle.dmfb_oracle import DmfbOracle  # the checker
    ora = DmfbOracle(n_envs=E, seed=seed, **cfg)
    ora.reset()
    obs, state = ora.observe(), _oracle_state(ora)
    new = lambda e: dict(o=[], u=[], r=[], o_next=[], s=[state[e].copy()], cons=0, succ=0)
    open_eps = [new(e) for e in range(E)]
    closed = []
    for acts, term_gpu in steps:
        rew, dones, cons, succ = ora.step(acts)
        nxt, state = ora.observe(), _oracle_state(ora)
        term = dones.all(axis=1)
        np.testing.assert_array_equal(term, term_gpu.astype(bool))
        for e in range(E):
            ep = open_eps[e]
            ep['o'].append(obs[e].copy()); ep['o_next'].append(nxt[e].copy()); ep['u'].append(acts[e].copy())
            ep['s'].append(state[e].copy())
            ep['r'].append(np.sum(rew[e]) / n)
            ep['cons'] += int(cons[e]); ep['succ'] += int(succ[e])
            if term[e]:
                ln = len(ep['r'])
                d = {'o': np.zeros((T, n, O), np.int8), 'o_next': np.zeros((T, n, O), np.int8), 'u': np.zeros((T, n, 1), np.int8),
                     'r': np.zeros((T, 1), np.float32), 'avail_u': np.zeros((T, n, A), np.int8), 'avail_u_next': np.zeros((T, n, A), np.int8),
                     'u_onehot': np.zeros((T, n, A), np.int8), 'padded': np.ones((T, 1), bool), 'terminated': np.ones((T, 1), bool),
                     'states': np.zeros((T + 1, len(ep['s'][0])), np.int8)}
                d['o'][:ln], d['o_next'][:ln] = np.stack(ep['o']), np.stack(ep['o_next'])
                d['u'][:ln, :, 0] = np.stack(ep['u'])
                d['u_onehot'][:ln] = np.eye(A, dtype=np.int8)[np.stack(ep['u'])]
                d['r'][:ln, 0] = np.asarray(ep['r'], np.float64).astype(np.float32)
                d['avail_u'][:ln] = 1; d['avail_u_next'][:ln] = 1
                d['padded'][:ln] = False; d['terminated'][:ln - 1] = False
                d['states'][:ln + 1] = np.stack(ep['s'])          # slot 0 = s[0], slot t + 1 = s_next[t]
                total = 0.0
                for v in ep['r']:
                    total += v
                d['stats'] = (total, ln if ep['succ'] else T, ep['cons'], ep['succ'])
                d['len'] = ln
                closed.append(d)
        if term.any():
            ora.reset(mask=term.astype(np.uint8))
            obs, state = ora.observe(), _oracle_state(ora)
            for e in np.nonzero(term)[0]:
                open_eps[e] = new(e)
        else:
            obs = nxt
    return closed


def _compare_ring(buf, want):
    """The episodes still in the ring (the last `size` closed, episode k in slot k % size) against the oracle's, bit for bit."""
    size = buf.size
    states = buf.states.cpu().numpy()
    got = {k: buf.buffers[k].cpu().numpy() for k in KEYS}
    stats = buf.ring_stats.cpu().numpy()
    for k in range(max(0, len(want) - size), len(want)):
        d, slot = want[k], k % size
        assert buf.host_len[slot] == d['len'], (k, slot)
        np.testing.assert_array_equal(states[slot], d['states'], err_msg='states of slot %d (len %d)' % (slot, d['len']))
        for key in KEYS:
            np.testing.assert_array_equal(got[key][slot].reshape(d[key].shape), d[key], err_msg='slot %d key %s' % (slot, key))
        np.testing.assert_array_equal(stats[slot].view(np.int64), np.asarray(d['stats'], np.float64).view(np.int64))


@pytest.mark.parametrize('case', ['random_4d', 'trained_4d_odd_k', 'random_10d', 'blocks'])
def test_qmix_stream_replays_through_the_oracle(case):
    if case == 'random_10d':
        W, n, nb, E, Ks, eps = 20, 10, 0, 64, (85, 85), 1.0
    elif case == 'blocks':
        W, n, nb, E, Ks, eps = 12, 3, 3, 96, (50, 50), 0.3
    else:
        W, n, nb, E, Ks, eps = 10, 4, 0, 256, ((37, 37, 37) if case.endswith('odd_k') else (50, 50)), (0.05 if 'trained' in case else 1.0)
    seed = 17
    env, args, agents, worker, buf = _make(W, n, E, seed, buffer_size=E + E // 2, nb=nb)
    assert worker.stream_ok() and not worker._stream_state(buf).fused_reset
    if 'trained' in case:
        _load_4d(agents)
    worker.epsilon = torch.tensor(eps, device=DEV)
    worker.anneal_epsilon, worker.min_epsilon = 0.0, 0.0
    T, O = args.episode_limit, env.obs_len
    steps = []
    worker.stream_step_hook = lambda s, a, term: steps.append((a.cpu().numpy().copy(), term.cpu().numpy().copy()))
    acc = np.zeros(4, np.int64)
    for K in Ks:
        acc += np.asarray(buf.sync_host(worker.generate_steps(buf, K)))
    want = _oracle_episodes(dict(width=W, length=W, n_agents=n, n_blocks=nb, fov=9), E, seed, steps, T, n, O)
    assert len(want) == buf.host_closed == acc[0] > buf.size            # the ring wrapped
    if 'trained' in case:
        lens = np.array([d['len'] for d in want])
        assert (lens < T).sum() >= 3 and len(set(lens.tolist())) >= 3, lens
    if nb:
        assert int(np.abs(want[-1]['states'][0].reshape(3, W, W)[2]).sum()) > 0   # the block layer is there
    _compare_ring(buf, want)


# ---------------------------------------------------------------------------------------------------------- 3. graph == eager
def test_qmix_stream_graph_replay_equals_eager_play_across_an_evaluation():
    W, n, E, seed = 10, 4, 64, 9
    outs = []
    for graph in (False, True):
        env, args, agents, worker, buf = _make(W, n, E, seed, buffer_size=4096)
        _load_4d(agents)
        worker.use_graph = graph
        worker.epsilon = torch.tensor(0.3, device=DEV)
        worker.anneal_epsilon, worker.min_epsilon = 1e-5, 0.05
        accs = [buf.sync_host(worker.generate_steps(buf, K)) for K in (39, 40, 41)]
        worker.use_graph = False
        ev = worker.evaluate(1)
        worker.use_graph = graph
        accs += [buf.sync_host(worker.generate_steps(buf, K)) for K in (41, 39, 40)]
        if graph:
            assert sorted(worker._stream.graphs) == [39, 40, 41]
        outs.append((accs, ev, buf.states.clone(), {k: v.clone() for k, v in buf.buffers.items()}, buf.ring_len.clone(),
                     buf.ring_state.clone(), buf.ring_stats.clone(), worker._stream.s_stage.clone(), worker._stream.t_ep.clone()))
    a, b = outs
    assert a[0] == b[0] and a[1] == b[1], (a[0], b[0])
    closed = int(a[5][2])
    assert E * 5 < closed < 4096
    assert torch.equal(a[2][:closed], b[2][:closed])
    assert bool((a[2][:closed, 0].abs().sum(1) > 0).all())
    for k in a[3]:
        assert torch.equal(a[3][k][:closed], b[3][k][:closed]), k
    assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]) and torch.equal(a[6].view(torch.int64), b[6].view(torch.int64))
    assert torch.equal(a[7], b[7]) and torch.equal(a[8], b[8])


# ---------------------------------------------------------------------------------------------------------- 4. the Trainer
def _trainer(E=512, rounds=60, alg='qmix', **kw):
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.train import Trainer
    env = VecDMFB(10, 10, 4, fov=9, n_envs=E, seed=7, device=DEV)
    args = make_args(alg=alg, device=DEV, n_envs=E, batch_size=256, train_time=4, buffer_size=8 * E,
                     anneal_steps=E * 40 * rounds * 0.6, **kw, **env.get_env_info())
    return Trainer(env, args)


def test_qmix_trainer_with_stream_state_learns():
    torch.manual_seed(0)
    rounds = 60
    tr = _trainer(rounds=rounds, stream_state=True)
    assert tr.stream
    r0, _, c0, _ = tr.rolloutWorker.evaluate(2)
    seen = []
    orig = tr.agents.train

    def train(batch, step, **kw):
        seen.append(int(batch['s'][:, 0].abs().sum(1).min()))
        return orig(batch, step, **kw)
    tr.agents.train = train
    for _ in range(rounds):
        assert tr.collect_and_learn() == 512 * 40
        assert tr.last_round['episodes'] >= 512
    r1, _, c1, _ = tr.rolloutWorker.evaluate(2)
    print('qmix stream greedy reward %.2f -> %.2f, constraints %.2f -> %.2f' % (r0, r1, c0, c1))
    assert len(seen) == 4 * rounds and min(seen) > 0   # every learned episode starts from a real state
    assert tr._packed is False                         # QMIX learns on the gathered padded batch
    assert torch.isfinite(tr.agents.policy.last_loss)
    assert r1 > r0 + 40.0, (r0, r1)
    assert c1 < 0.2 * c0 + 1.0, (c0, c1)


def test_qmix_stream_true_accepted_with_the_flag_only():
    assert _trainer(E=64, stream=True, stream_state=True).stream
    tr = _trainer(E=64)
    assert not tr.stream and not tr.rolloutWorker.stream_ok()
    tr.rolloutWorker.use_graph = True
    assert not tr.rolloutWorker.stream_ok()


def test_stream_state_checks_the_replay_buffer():
    env, args, agents, worker, buf = _make(10, 4, 64, 1, buffer_size=64)
    buf.states, buf.state_shape = None, None
    with pytest.raises(ValueError, match='global state'):
        worker.generate_steps(buf, 1)


def test_vdn_ignores_the_flag():
    """VDN with stream_state set: no stage, no state launch, the same ring bit for bit as without the flag."""
    outs = []
    for flag in (False, True):
        env, args, agents, worker, buf = _make(10, 4, 64, 5, buffer_size=160, alg='vdn', stream_state=flag)
        called = []
        env.global_obs_stage_first = lambda *a: called.append('first')
        env.global_obs_stage_close = lambda *a: called.append('close')
        worker.epsilon = torch.tensor(0.9, device=DEV)
        accs = [buf.sync_host(worker.generate_steps(buf, 40)) for _ in range(3)]
        assert not called and worker._stream.s_stage is None and buf.states is None and worker._stream.fused_reset
        outs.append((accs, {k: v.clone() for k, v in buf.buffers.items()}, buf.ring_stats.clone()))
    a, b = outs
    assert a[0] == b[0]
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert torch.equal(a[2].view(torch.int64), b[2].view(torch.int64))
