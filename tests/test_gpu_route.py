"""Routing given tasks on the GPU: the route append kernels against get_state, recorded routes replayed through the CPU oracles
bit for bit, the best-of-K select kernel against its numpy rule, Router against the greedy Evaluator, and the evaluate CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from vdn_helpers import det_init

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _agents(env, alg='vdn', salt=0.25, **over):
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    name = 'meda' if env.__class__.__name__ == 'VecMEDA' else 'dmfb'
    args = make_args(name=name, drop_num=env.n_agents, width=env.width, length=env.length, fov=env.fov, device=DEV, alg=alg,
                     **dict(env.get_env_info(), **over))
    if alg == 'qmix':
        args.state_shape = env.state_shape
    agents = Agents(args)
    det_init(agents.policy.eval_rnn, salt=salt)
    return agents


def _tasks(name, E, seed, **cfg):
    """Valid random tasks (and blocks) as the env generates them."""
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.env.meda import VecMEDA
    env = (VecDMFB if name == 'dmfb' else VecMEDA)(n_envs=E, seed=seed, device=DEV, **cfg)
    env.reset()
    s, g = env.get_task()
    b = env.get_blocks().cpu().numpy() if name == 'dmfb' and cfg.get('n_blocks', 0) else None
    return s.cpu().numpy(), g.cpu().numpy(), b


# ---------------------------------------------------------------------------------------------------- 1. route append
@pytest.mark.parametrize('name,cfg', [
    ('dmfb', dict(width=10, length=10, n_agents=4, fov=9)),
    ('dmfb', dict(width=20, length=20, n_agents=10, fov=9, n_blocks=3)),
    ('meda', dict(width=30, length=30, n_agents=4, fov=19, version=0)),
    ('meda', dict(width=30, length=30, n_agents=4, fov=19, version=2)),
])
def test_route_append_equals_get_state(name, cfg):
    from marl_dmfb_amd import _lib
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.env.meda import VecMEDA
    E, n = 200, cfg['n_agents']
    env = (VecDMFB if name == 'dmfb' else VecMEDA)(n_envs=E, seed=7, device=DEV, **cfg)
    T = env.max_step
    A = 5 if name == 'dmfb' else 9
    route = torch.full((E, T + 1, n, 2), 255, dtype=torch.uint8, device=DEV)
    env.reset()
    env.route_append(-1, T, route)
    active = torch.ones(E, dtype=torch.uint8, device=DEV)
    active[::3] = 0                                    # frozen from the start
    rng = np.random.default_rng(1)
    for t in range(T):
        if t == T // 2:
            active[1::5] = 0                           # frozen on the way
        env.step(torch.as_tensor(rng.integers(0, A, (E, n)), dtype=torch.int32, device=DEV), active=active)
        env.route_append(t, T, route)
        pos = env.get_state()['pos'].cpu().numpy()
        np.testing.assert_array_equal(route[:, t + 1].cpu().numpy(), pos, err_msg='slot %d' % (t + 1))
    r = route.cpu().numpy()
    assert (r[::3] == r[::3, :1]).all()                # a chip frozen from the start never moves
    assert (r[1::15, T // 2:] == r[1::15, T // 2:T // 2 + 1]).all()
    assert (r[:, 1:] != r[:, :-1]).any()               # the others do move
    # bad arguments come back before any launch
    raw = getattr(_lib, name + '_vec')()
    fn = getattr(raw, name + '_vec_route_append')
    p = route.data_ptr()
    assert fn(env.h, -2, T, p, None) == -1 and fn(env.h, T, T, p, None) == -1 and fn(env.h, 0, 0, p, None) == -1
    assert fn(env.h, 0, T, None, None) == -1 and fn(env.h, 0, T, p + 1, None) == -1
    torch.cuda.synchronize()


def test_evaluator_route_mode_eager_equals_graph_replay():
    """The route round of Evaluator in eager mode and through a captured graph (replayed twice) records the same routes; the
    existing graph keys stay untouched by route mode."""
    from marl_dmfb_amd.common.rollout import Evaluator
    from marl_dmfb_amd.env.dmfb import VecDMFB
    E = 256
    s, g, b = _tasks('dmfb', E, 3, width=20, length=20, n_agents=10, fov=9, n_blocks=2)
    out = []
    for graph in (False, True, True):
        env = VecDMFB(20, 20, 10, 2, fov=9, n_envs=E, seed=0, device=DEV)
        env.set_task(s, g)
        env.set_blocks(b)
        ev = Evaluator(env, _agents(env), env.max_step)
        ev.use_graph = graph
        ev.reset_fn = env.restart
        ev.route_active = torch.ones(E, dtype=torch.uint8, device=DEV)
        ev.route_active[::4] = 0
        play = ev._play_graphed if graph else ev._play
        for _ in range(2 if graph else 1):
            r = play(0.0, evaluate=True, record=False, route=True)
        assert all(k[0] == 'route' for k in ev._graphs)
        ep = r[4]
        out.append((ep['route'].cpu().numpy(), ep['u'].cpu().numpy(), ep['steps'].cpu().numpy(), r[3].cpu().numpy()))
        # slot t + 1 of every chip equals its final position after the episode
        pos = env.get_state()['pos'].cpu().numpy()
        np.testing.assert_array_equal(ep['route'][:, -1].cpu().numpy(), pos)
    for o in out[1:]:
        for a, b_ in zip(out[0], o):
            np.testing.assert_array_equal(a, b_)
    assert (out[0][2][::4] == 0).all() and (out[0][2][1::4] > 0).all()


# ---------------------------------------------------------------------------------------------------- 2. oracle replay
def _replay_dmfb(res, s, g, b, health, draws, cfg):
    from oracle.dmfb_oracle import DmfbOracle
    B, T = res.steps.shape[0], res.actions.shape[1]
    n = s.shape[1]
    ora = DmfbOracle(n_envs=B, seed=0, with_maps=health is not None, n_blocks=0 if b is None else b.shape[1], **cfg)
    if health is not None:
        ora.set_map('health', health)
    if b is not None:
        ora.set_blocks(b)
    ora.set_task(s, g)
    ora.restart()
    np.testing.assert_array_equal(ora.get_state()['pos'], res.positions[:, 0])
    cons = np.zeros(B, np.int64)
    succ = np.zeros(B, bool)
    for t in range(T):
        live = t < res.steps
        if not live.any():
            break
        a = np.where(live[:, None], res.actions[:, t], 0).astype(np.int32)
        assert (a >= 0).all()
        u = np.full((B, n), 2.0) if draws is None else np.where(live[:, None], draws[t], 2.0)
        _, dones, c, sc = ora.step(a, u if health is not None else None)
        cons += np.where(live, c, 0)
        succ |= live & (sc > 0)
        pos = ora.get_state()['pos']
        np.testing.assert_array_equal(res.positions[live, t + 1], pos[live], err_msg='t=%d' % t)
        ended = live & dones.all(axis=1).astype(bool)
        assert not (ended & (res.steps != t + 1)).any(), 'episode ends t=%d' % t
    # after the end the last position holds
    for k in range(B):
        assert (res.positions[k, res.steps[k]:] == res.positions[k, res.steps[k]]).all()
        assert (res.actions[k, res.steps[k]:] == -1).all()
    np.testing.assert_array_equal(cons, res.constraints)
    np.testing.assert_array_equal(succ, res.success)


@pytest.mark.parametrize('tries,with_health', [(1, True), (3, False)])
def test_dmfb_routes_replay_through_the_oracle(tries, with_health):
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.route import Router
    cfg = dict(width=20, length=20, n_agents=10, fov=9)
    B = 96
    s, g, b = _tasks('dmfb', B, 11, n_blocks=3, **cfg)
    health = None
    if with_health:
        rng = np.random.default_rng(4)
        health = np.where(rng.random((B, 20, 20)) < 0.3, rng.uniform(0.2, 0.9, (B, 20, 20)), 1.0)
    probe = VecDMFB(n_envs=1, device=DEV, **cfg)
    router = Router(_agents(probe, salt=0.5), name='dmfb', n_blocks=3, use_graph=True, device=DEV, **cfg)
    res = router.route(s, g, blocks=b, health=health, tries=tries, epsilon=0.3, seed=9)
    assert res.positions.shape == (B, 81, 10, 2) and res.actions.shape == (B, 80, 10)
    draws = None
    if with_health:   # one round (tries=1): the draws of that round, chip = task
        draws = next(iter(router._slots.values()))['draws'].cpu().numpy()
    if tries > 1:
        assert (res.try_index > 0).any()
    _replay_dmfb(res, s, g, b, health, draws, dict(width=20, length=20, n_agents=10, fov=9))


@pytest.mark.parametrize('version', [0, 2])
def test_meda_routes_replay_through_the_oracle(version):
    from marl_dmfb_amd.env.meda import VecMEDA
    from marl_dmfb_amd.route import Router
    from oracle.meda_oracle import MedaOracle
    cfg = dict(width=30, length=30, n_agents=4, fov=19)
    B = 64
    s, g, _ = _tasks('meda', B, 5, version=version, **cfg)
    probe = VecMEDA(n_envs=1, device=DEV, version=version, **cfg)
    router = Router(_agents(probe, salt=0.1), name='meda', version=version, device=DEV, **cfg)
    res = router.route(s, g, tries=2, epsilon=0.5, seed=1)
    assert res.constraints.dtype == np.float64
    ora = MedaOracle(n_envs=B, seed=0, version=version, **cfg)
    ora.set_task(s, g)
    ora.restart()
    np.testing.assert_array_equal(ora.get_state()['pos'], res.positions[:, 0])
    fail = np.zeros(B)
    succ = np.zeros(B, bool)
    for t in range(res.actions.shape[1]):
        live = t < res.steps
        if not live.any():
            break
        _, dones, f, sc = ora.step(np.where(live[:, None], res.actions[:, t], 0).astype(np.int32))
        fail = fail + np.where(live, f, 0.0)
        succ |= live & (sc > 0)
        np.testing.assert_array_equal(res.positions[live, t + 1], ora.get_state()['pos'][live], err_msg='t=%d' % t)
        assert not (live & dones.all(axis=1).astype(bool) & (res.steps != t + 1)).any(), 't=%d' % t
    np.testing.assert_array_equal(_bits(fail), _bits(res.constraints))
    np.testing.assert_array_equal(succ, res.success)


# ---------------------------------------------------------------------------------------------------- 3. select kernel
@pytest.mark.parametrize('K,f64', [(1, False), (3, True), (8, False), (8, True), (70, True)])
def test_route_select_kernel_equals_the_numpy_rule(K, f64):
    from marl_dmfb_amd import _lib
    from marl_dmfb_amd.route import select_reference
    rng = np.random.default_rng(K + 100 * f64)
    B, n, T = 203, 3, 13
    steps = rng.integers(1, 4, B * K)
    success = rng.integers(0, 2, B * K) * rng.integers(1, 3, B * K)
    success[: 5 * K] = 0                                   # tasks whose tries all fail
    cons = rng.integers(0, 3, B * K)
    cons = cons.astype(np.float64) * 0.5 if f64 else cons.astype(np.int32)
    route = rng.integers(0, 256, (B * K, T + 1, n, 2)).astype(np.uint8)
    u = rng.integers(-1, 9, (B * K, T, n)).astype(np.int8)
    d = lambda a: torch.as_tensor(a, device=DEV)
    st, su, co, ro, uu = d(steps.astype(np.int64)), d(success.astype(np.int64)), d(cons), d(route), d(u)
    ro_out = torch.zeros((B, T + 1, n, 2), dtype=torch.uint8, device=DEV)
    u_out = torch.zeros((B, T, n), dtype=torch.int8, device=DEV)
    choice = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    lib = _lib.checked('rollout_route')
    lib.rollout_route_select(B, K, n, T, st.data_ptr(), su.data_ptr(), co.data_ptr(), int(f64), ro.data_ptr(), uu.data_ptr(),
                             ro_out.data_ptr(), u_out.data_ptr(), choice.data_ptr(), torch.cuda.current_stream().cuda_stream)
    want = select_reference(steps, success, cons, K)
    got = choice.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    chip = np.arange(B) * K + want
    np.testing.assert_array_equal(ro_out.cpu().numpy(), route[chip])
    np.testing.assert_array_equal(u_out.cpu().numpy(), u[chip])
    # the choice alone (no rows)
    choice.fill_(-1)
    lib.rollout_route_select(B, K, n, T, st.data_ptr(), su.data_ptr(), co.data_ptr(), int(f64), None, None, None, None,
                             choice.data_ptr(), torch.cuda.current_stream().cuda_stream)
    np.testing.assert_array_equal(choice.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------- 4. / 5. Router
def _greedy_evaluator(s, g, agents, **cfg):
    from marl_dmfb_amd.common.rollout import Evaluator
    from marl_dmfb_amd.env.dmfb import VecDMFB
    env = VecDMFB(n_envs=s.shape[0], seed=0, device=DEV, **cfg)
    env.set_task(s, g)
    ev = Evaluator(env, agents, env.max_step)
    ev.reset_fn = env.restart
    _, steps, _, success, _, _ = ev._play(0.0, evaluate=True, record=False)
    return steps.cpu().numpy(), success.cpu().numpy() > 0


def test_tries_1_is_the_greedy_evaluator_and_tries_8_is_never_worse():
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.route import Router
    cfg = dict(width=10, length=10, n_agents=4, fov=9)
    B = 300
    s, g, _ = _tasks('dmfb', B, 21, **cfg)
    agents = _agents(VecDMFB(n_envs=1, device=DEV, **cfg), salt=0.7)
    steps_ev, succ_ev = _greedy_evaluator(s, g, agents, **cfg)
    router = Router(agents, name='dmfb', device=DEV, **cfg)
    r1 = router.route(s, g, tries=1)
    assert router.rounds == 1
    np.testing.assert_array_equal(r1.success, succ_ev)
    np.testing.assert_array_equal(np.where(r1.success, r1.steps, 40), steps_ev)
    assert (r1.try_index == 0).all()
    # chunks: the same tasks through handles of 64 chips (5 chunks, the last one padded)
    small = Router(agents, name='dmfb', device=DEV, max_chips=64, use_graph=False, **cfg)
    rc = small.route(s, g, tries=1)
    assert small.rounds == 5
    for k in ('positions', 'actions', 'steps', 'success', 'constraints'):
        np.testing.assert_array_equal(getattr(rc, k), getattr(r1, k), err_msg=k)
    r8 = router.route(s, g, tries=8, epsilon=0.2, seed=3)
    assert (r8.success >= r1.success).all()
    both = r8.success & r1.success
    assert (r8.steps[both] <= r1.steps[both]).all()
    greedy_best = r8.try_index == 0
    np.testing.assert_array_equal(r8.steps[greedy_best], r1.steps[greedy_best])
    np.testing.assert_array_equal(r8.positions[greedy_best], r1.positions[greedy_best])
    assert (~greedy_best).any()
    again = router.route(s, g, tries=8, epsilon=0.2, seed=3)
    for k in ('positions', 'actions', 'steps', 'success', 'constraints', 'try_index'):
        np.testing.assert_array_equal(getattr(again, k), getattr(r8, k), err_msg=k)


def _fields(r):
    return ('positions', 'actions', 'steps', 'success', 'constraints', 'try_index')


def _same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in _fields(a))


def test_seed_is_honoured_across_calls_and_chunks_under_graph_replay():
    """One Router with its graphs captured routes the same tasks with seed 1, seed 2, seed 1: the two seed-1 results are equal and
    equal a fresh Router's, eager and graph alike, and seed 2 picks differently.  The same holds for a batch in four chunks."""
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.route import Router
    cfg = dict(width=10, length=10, n_agents=4, fov=9)
    B = 256
    s, g, _ = _tasks('dmfb', B, 31, **cfg)
    agents = _agents(VecDMFB(n_envs=1, device=DEV, **cfg), salt=0.7)
    for max_chips in (32768, 512):   # one chunk; four chunks of 64 tasks x 8 tries
        router = Router(agents, name='dmfb', device=DEV, max_chips=max_chips, **cfg)
        a1 = router.route(s, g, tries=8, epsilon=0.3, seed=1)
        b = router.route(s, g, tries=8, epsilon=0.3, seed=2)
        a2 = router.route(s, g, tries=8, epsilon=0.3, seed=1)
        assert _same(a1, a2)
        assert not _same(a1, b)
        assert (a1.try_index > 0).any() and (b.try_index > 0).any()
        fresh = Router(agents, name='dmfb', device=DEV, max_chips=max_chips, **cfg).route(s, g, tries=8, epsilon=0.3, seed=1)
        eager = Router(agents, name='dmfb', device=DEV, max_chips=max_chips, use_graph=False, **cfg).route(
            s, g, tries=8, epsilon=0.3, seed=1)
        assert _same(a1, fresh) and _same(a1, eager)
        # the first chunk and the others draw from different counter ranges: the same tasks in every chunk do not pick alike
        if max_chips == 512:
            t0, t1 = np.tile(s[:64], (4, 1, 1)), np.tile(g[:64], (4, 1, 1))
            r = router.route(t0, t1, tries=8, epsilon=0.3, seed=5)
            assert not all(np.array_equal(r.actions[:64], r.actions[64 * k:64 * (k + 1)]) for k in range(1, 4))


def test_one_router_with_changing_block_counts_replays_through_the_oracle():
    """Calls with 0, 3, 1 and again 0 blocks per task on ONE Router (graph replay): every result replays through DmfbOracle with
    the blocks of its own call, and equals a fresh Router's."""
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.route import Router
    cfg = dict(width=20, length=20, n_agents=10, fov=9)
    B = 64
    s0, g0, _ = _tasks('dmfb', B, 41, **cfg)
    s1, g1, b3 = _tasks('dmfb', B, 42, n_blocks=3, **cfg)
    agents = _agents(VecDMFB(n_envs=1, device=DEV, **cfg), salt=0.4)
    router = Router(agents, name='dmfb', device=DEV, n_blocks=3, **cfg)   # one Router that takes up to three blocks per task
    calls = [(s0, g0, None), (s1, g1, b3), (s1, g1, b3[:, :1].copy()), (s0, g0, None), (s1, g1, b3)]
    for k, (s, g, b) in enumerate(calls):
        res = router.route(s, g, blocks=b, tries=2, epsilon=0.3, seed=k)
        _replay_dmfb(res, s, g, b, None, None, cfg)
        fresh = Router(agents, name='dmfb', device=DEV, **cfg).route(s, g, blocks=b, tries=2, epsilon=0.3, seed=k)
        assert _same(res, fresh), 'call %d' % k


def test_qmix_checkpoint_routes_with_its_agent_network():
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.route import Router
    cfg = dict(width=10, length=10, n_agents=4, fov=9)
    s, g, _ = _tasks('dmfb', 32, 2, **cfg)
    env = VecDMFB(n_envs=1, device=DEV, **cfg)
    vdn, qmix = _agents(env, salt=0.3), _agents(env, alg='qmix', salt=0.3)
    a = Router(vdn, name='dmfb', device=DEV, **cfg).route(s, g, tries=2, seed=4)
    b = Router(qmix, name='dmfb', device=DEV, **cfg).route(s, g, tries=2, seed=4)
    np.testing.assert_array_equal(a.positions, b.positions)


# ---------------------------------------------------------------------------------------------------- 6. CLI
def test_evaluate_cli(tmp_path):
    from marl_dmfb_amd.env.dmfb import VecDMFB
    env = VecDMFB(20, 20, 4, fov=9, n_envs=1, device=DEV)
    agents = _agents(VecDMFB(10, 10, 4, fov=9, n_envs=1, device=DEV), salt=0.9)   # trained on 10 x 10, evaluated on 20 x 20
    d = tmp_path / 'model' / 'vdn' / 'fov9'
    d.mkdir(parents=True)
    torch.save(agents.policy.eval_rnn.state_dict(), str(d / 'rnn_net_params.pkl'))
    torch.save(agents.policy.eval_mixer.state_dict(), str(d / 'vdn_net_params.pkl'))
    base = [sys.executable, '-m', 'marl_dmfb_amd.evaluate', 'dmfb', '--fov', '9', '--chip_size', '20', '--model_dir',
            str(tmp_path / 'model')]
    run = lambda extra: subprocess.run(base + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
    out = run(['--evaluate_task', '64', '--routes', str(tmp_path / 'r.npz')])
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    assert any(l.startswith('time:') for l in lines)
    assert any(l.startswith('The average total_rewards of vdn is  ') for l in lines)
    steps_line = [l for l in lines if l.startswith('The average total_steps is: ')]
    rate_line = [l for l in lines if l.startswith('The successful rate is: ')]
    assert steps_line and rate_line
    with np.load(tmp_path / 'r.npz') as f:
        assert sorted(f.files) == sorted(['positions', 'actions', 'steps', 'success', 'constraints', 'starts', 'goals', 'cfg'])
        assert f['positions'].shape == (64, 81, 4, 2) and f['actions'].shape == (64, 80, 4) and f['starts'].shape == (64, 4, 2)
        steps, success = f['steps'], f['success']
        assert float(steps_line[0].split(': ')[1]) == pytest.approx(np.where(success, steps, 80).mean())
        assert float(rate_line[0].split(': ')[1]) == pytest.approx(success.mean())
        assert (f['positions'][np.arange(64), steps] == f['positions'][:, -1]).all()
        tasks = {'starts': f['starts'][:16], 'goals': f['goals'][:16]}
    np.savez(tmp_path / 'tasks.npz', **tasks)
    out = run(['--tasks', str(tmp_path / 'tasks.npz'), '--tries', '4', '--routes', str(tmp_path / 't.npz')])
    assert out.returncode == 0, out.stderr[-3000:]
    with np.load(tmp_path / 't.npz') as f:
        assert f['positions'].shape == (16, 81, 4, 2) and f['try_index'].shape == (16,)
        np.testing.assert_array_equal(f['positions'][:, 0], tasks['starts'])
    del env
