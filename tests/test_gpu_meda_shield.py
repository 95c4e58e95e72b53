"""The MEDA action shield on the GPU (include/meda_vec.h: meda_vec_shield): the kernel against
marl_dmfb_amd.shield.meda_shield_reference on states reached through set_task and a step, its staging and argument guards, a
closed loop with a random-init policy on degraded chips, the continuous rollout ring, Router and the switch.  Every comparison
is exact.

The env, like the reference, admits (width // 15) * (length // 15) droplets at the most (meda.py:151-154), so a 12x12 chip cannot
be created at all and a 30x60 chip holds 8 droplets: the kernel cases take, per droplet count, the smallest chip the env admits
(15x15, 15x30, 60x60: the clamps of every side are in reach of most droplets), 30x60 where the count fits, and 128x128.  The rule
on a 12x12 chip is checked on the CPU (tests/test_meda_shield_host.py)."""
import os

import numpy as np
import pytest
import torch

from meda_round_helpers import CFG, agents as _agents, health as _health, switch_off_round
from meda_shield_helpers import kernel_case_rounds, kernel_case_task

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 0x55
A = 9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'shield_off_meda_round.npz')


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _onehot(actions):
    """int8 (..., 9): the one-hot row of every action, all zero for an action outside [0, 9)."""
    a = np.asarray(actions)
    return (a[..., None] == np.arange(A)).astype(np.int8)


def _state(env):
    st = env.get_state()
    return st['pos'].cpu().numpy(), env.get_task()[1].cpu().numpy(), st['status'].cpu().numpy()


SMALLEST = {1: (15, 15), 2: (15, 30), 15: (60, 60), 16: (60, 60)}
KERNEL_CASES = [(E, n, W, L) for E in (1, 5, 67) for n in (1, 2, 15, 16)
                for W, L in (SMALLEST[n], (30, 60), (128, 128)) if n <= (W // 15) * (L // 15)]


def test_the_env_refuses_the_chips_the_cases_leave_out():
    from marl_dmfb_amd.env.meda import VecMEDA
    for W, L, n in ((12, 12, 1), (30, 60, 15)):
        with pytest.raises(RuntimeError, match='Too many droplets'):
            VecMEDA(W, L, n, fov=19, n_envs=1, device=DEV)


@pytest.mark.parametrize('E,n,W,L', KERNEL_CASES)
def test_kernel_equals_reference(E, n, W, L):
    from marl_dmfb_amd.env.meda import VecMEDA
    from marl_dmfb_amd.shield import meda_anchors, meda_shield_reference
    rng = np.random.default_rng(E * 1000 + n * 10 + W)
    T = 5
    env = VecMEDA(W, L, n, fov=19, n_envs=E, seed=3, device=DEV)
    starts, goals, first = kernel_case_task(rng, E, n, W, L)
    env.set_task(starts, goals)
    env.step(_dev(first))                           # healthy electrodes: every move happens
    pos, goals, done = _state(env)                  # read back: what the kernel sees
    forced, _ = meda_anchors(pos, goals, done)
    if E * n >= 60:
        assert done.any() and (forced & (done == 0)).any() and (~forced).any()
    if W == 128 and E > 1:
        assert pos.max() == 125                     # a centre on the last valid column or row of the byte range
    seen_unsafe = seen_override = 0
    for rnd, q, picks, active in kernel_case_rounds(rng, E, n):
        over0 = rng.integers(0, 1000, E).astype(np.int32)
        want, want_over, want_unsafe = meda_shield_reference(W, L, pos, goals, done, q, picks, active)
        # round 0: no staging; round 1: the common slot 3; round 2: every chip its own slot, some out of range
        t_ep = rng.integers(0, T, E).astype(np.int32)
        t_ep[::3] = rng.choice([-1, T, 100, -2 ** 31, 2 ** 31 - 1], len(t_ep[::3]))
        slots = (None, np.full(E, 3, np.int32), t_ep)[rnd]
        actions, onehot = _dev(picks.copy()), torch.full((E, n, A), SENTINEL, dtype=torch.int8, device=DEV)
        ep_u = torch.full((E, T, n, 1), SENTINEL, dtype=torch.int8, device=DEV)
        ep_oh = torch.full((E, T, n, A), SENTINEL, dtype=torch.int8, device=DEV)
        over, unsafe = _dev(over0.copy()), torch.zeros(E, dtype=torch.uint8, device=DEV)
        env.shield(_dev(q), actions, onehot, ep_u if rnd else None, ep_oh if rnd else None, t=3 if rnd == 1 else 0,
                   t_ep=_dev(t_ep) if rnd == 2 else None, active=_dev(active) if rnd else None, overrides=over, unsafe=unsafe)
        want_u, want_oh = np.full((E, T, n, 1), SENTINEL, np.int8), np.full((E, T, n, A), SENTINEL, np.int8)
        for e in range(E):
            if rnd and active[e] and 0 <= slots[e] < T:
                want_u[e, slots[e], :, 0] = want[e]
                want_oh[e, slots[e]] = _onehot(want[e])
        np.testing.assert_array_equal(actions.cpu().numpy(), want, err_msg='round %d' % rnd)
        np.testing.assert_array_equal(onehot.cpu().numpy(), np.where(active[:, None, None] != 0, _onehot(want), np.int8(SENTINEL)))
        np.testing.assert_array_equal(ep_u.cpu().numpy(), want_u)
        np.testing.assert_array_equal(ep_oh.cpu().numpy(), want_oh)
        np.testing.assert_array_equal(over.cpu().numpy(), over0 + want_over)
        np.testing.assert_array_equal(unsafe.cpu().numpy(), want_unsafe)
        assert (want[forced & (active[:, None] != 0)] == picks[forced & (active[:, None] != 0)]).all()
        seen_unsafe += int(want_unsafe.sum())
        seen_override += int(want_over.sum())
    if E * n >= 60:
        assert seen_override > 0
    if E > 1 and n >= 15:
        assert seen_unsafe > 0, 'the case has no unsafe chip'
    np.testing.assert_array_equal(env.get_state()['pos'].cpu().numpy(), pos)         # the shield moves nothing


def test_argument_guards_return_bad_arg_and_launch_nothing():
    from marl_dmfb_amd import _lib
    from marl_dmfb_amd.env.meda import VecMEDA
    E, n, T = 8, 2, 5
    env = VecMEDA(30, 30, n, fov=19, n_envs=E, seed=0, device=DEV)
    env.reset()
    q = torch.zeros((E, n, A), device=DEV)
    q[..., 8] = 1.0                                     # a launch would turn every pick into STALL ...
    actions = torch.full((E, n), 11, dtype=torch.int32, device=DEV)   # ... for the picks are out of range
    onehot = torch.full((E, n, A), SENTINEL, dtype=torch.int8, device=DEV)
    ep_u = torch.full((E, T, n), SENTINEL, dtype=torch.int8, device=DEV)
    ep_oh = torch.full((E, T, n, A), SENTINEL, dtype=torch.int8, device=DEV)
    fn = _lib.meda_vec().meda_vec_shield
    h, pq, pa, po, pu, ph = env.h, q.data_ptr(), actions.data_ptr(), onehot.data_ptr(), ep_u.data_ptr(), ep_oh.data_ptr()
    bad = [(None, pq, None, pa, po, pu, ph, T, 0, None, None, None, None),
           (h, None, None, pa, po, pu, ph, T, 0, None, None, None, None),
           (h, pq, None, None, po, pu, ph, T, 0, None, None, None, None),
           (h, pq, None, pa, None, pu, ph, T, 0, None, None, None, None),
           (h, pq, None, pa, po, pu, None, T, 0, None, None, None, None),
           (h, pq, None, pa, po, None, ph, T, 0, None, None, None, None),
           (h, pq, None, pa, po, pu, ph, 0, 0, None, None, None, None),
           (h, pq, None, pa, po, pu, ph, T, -1, None, None, None, None),
           (h, pq, None, pa, po, pu, ph, T, T, None, None, None, None)]
    for k, args in enumerate(bad):
        assert fn(*args) == -1, 'case %d' % k           # MEDA_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (actions == 11).all() and (onehot == SENTINEL).all() and (ep_u == SENTINEL).all() and (ep_oh == SENTINEL).all()
    # t is not looked at when every chip brings its own slot, nor the episode limit without the pair
    t_ep = torch.zeros(E, dtype=torch.int32, device=DEV)
    assert fn(h, pq, None, pa, po, pu, ph, T, -1, t_ep.data_ptr(), None, None, None) == 0
    assert fn(h, pq, None, pa, po, None, None, 0, -1, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (actions == 8).all() and (ep_u[:, 0] == 8).all() and (ep_u[:, 1:] == SENTINEL).all()
    with pytest.raises(ValueError):
        env.shield(q, actions, onehot, ep_u=ep_u)
    with pytest.raises(TypeError):
        env.shield(q.double(), actions, onehot)
    with pytest.raises(TypeError):
        env.shield(q, actions.long(), onehot)


# ---------------------------------------------------------------------------------------------------- policy play
def _episode(shield, E=64, seed=31):
    from marl_dmfb_amd.common.rollout import RolloutWorker
    from marl_dmfb_amd.env.meda import VecMEDA
    env = VecMEDA(n_envs=E, seed=seed, with_maps=True, device=DEV, **CFG)
    env.set_map('health', _health(E, seed))
    agents, args = _agents(env, n_envs=E, meda_shield=shield)
    worker = RolloutWorker(env, agents, args)
    assert worker.meda_shield == shield and not worker.shield
    worker.epsilon = torch.tensor(0.3, device=DEV)
    worker.anneal_epsilon, worker.min_epsilon = 0.0, 0.0
    _, _, cons, success, ep = worker.generate_episode()
    return worker, cons.cpu().numpy(), success.cpu().numpy(), {k: v.cpu().numpy() for k, v in ep.items()}


def test_closed_loop_with_a_policy_on_degraded_chips():
    """64 chips, 30x30 / 4 droplets, random-init policy with epsilon 0.3, health uniform in [0.6, 1): no proximity penalty under
    meda_shield where the same seed without it has some, and the recorded u / u_onehot are the executed actions: the recorded
    observations replay through the CPU oracle from them."""
    from oracle.meda_oracle import MedaOracle
    E, seed = 64, 31
    _, plain_cons, _, _ = _episode(False)
    assert (plain_cons != 0).any() and plain_cons.sum() < 0          # `fail` sums -0.6 per droplet of a near pair
    worker, cons, success, ep = _episode(True)
    assert (cons == 0).all()
    assert int(worker.shield_overrides.sum()) > 0 and int(worker.shield_unsafe.sum()) == 0
    valid = ~ep['padded'][:, :, 0].astype(bool)
    u = ep['u'][..., 0]
    np.testing.assert_array_equal(ep['u_onehot'][valid], _onehot(u)[valid])
    ora = MedaOracle(n_envs=E, seed=seed, with_maps=True, **CFG)
    ora.set_map('health', _health(E, seed))
    ora.reset()
    np.testing.assert_array_equal(ora.observe(), ep['o'][:, 0])
    for t in range(int(valid.sum(1).max())):
        live = valid[:, t]
        _, _, fail, _ = ora.step(np.where(live[:, None], u[:, t], 8).astype(np.int32))
        assert (fail[live] == 0).all(), 't=%d' % t
        np.testing.assert_array_equal(ora.observe()[live], ep['o_next'][live, t], err_msg='t=%d' % t)


def _ring(graph, K=45, calls=3, E=48, seed=23):
    from marl_dmfb_amd.common.replay_buffer import ReplayBuffer
    from marl_dmfb_amd.common.rollout import RolloutWorker
    from marl_dmfb_amd.env.meda import VecMEDA
    env = VecMEDA(n_envs=E, seed=seed, with_maps=True, device=DEV, version=2, **CFG)   # the v0_2 observation: the HIP front end
    env.set_map('health', _health(E, seed))
    agents, args = _agents(env, n_envs=E, buffer_size=256, meda_shield=True)
    worker = RolloutWorker(env, agents, args)
    assert worker.meda_shield and worker.stream_ok()
    worker.use_graph = graph
    buf = ReplayBuffer(args, device=DEV)
    worker.epsilon = torch.tensor(0.3, device=DEV)
    worker.anneal_epsilon, worker.min_epsilon = 0.0, 0.0
    steps = []
    if not graph:   # the hook sees the actions handed to the env (eager play only)
        worker.stream_step_hook = lambda s, a, term: steps.append((a.cpu().numpy().copy(), term.cpu().numpy().astype(bool)))
    overrides = 0
    for _ in range(calls):
        buf.sync_host(worker.generate_steps(buf, K))
        overrides += int(worker.shield_overrides.sum().item())
        assert int(worker.shield_unsafe.sum().item()) == 0
    return worker, buf, args, steps, overrides


def test_continuous_rollout_ring_eager_and_graph():
    E, n = 48, 4
    worker, buf, args, steps, overrides = _ring(graph=False)
    assert overrides > 0
    # the episodes in closing order (lock-step, then chip), from the actions the hook saw
    open_u, closed = [[] for _ in range(E)], []
    for acts, term in steps:
        for e in range(E):
            open_u[e].append(acts[e])
            if term[e]:
                closed.append(np.stack(open_u[e]))
                open_u[e] = []
    assert len(closed) == buf.host_closed == buf.current_size >= E
    T = args.episode_limit
    u = buf.buffers['u'][:len(closed)].cpu().numpy().reshape(len(closed), T, n)
    oh = buf.buffers['u_onehot'][:len(closed)].cpu().numpy().reshape(len(closed), T, n, A)
    stats = buf.ring_stats[:len(closed)].cpu().numpy()
    assert (stats[:, 2] == 0).all()                                  # constraints of every closed episode
    for k, acts in enumerate(closed):
        ln = len(acts)
        assert buf.host_len[k] == ln
        np.testing.assert_array_equal(u[k, :ln], acts, err_msg='slot %d' % k)
        np.testing.assert_array_equal(oh[k, :ln], _onehot(acts), err_msg='slot %d' % k)
        assert (u[k, ln:] == 0).all() and (oh[k, ln:] == 0).all()
    # the captured graph stages the same, from graphs of its own mode
    gworker, gbuf, _, _, goverrides = _ring(graph=True)
    st = gworker._stream
    assert list(st.shield_graphs) == [45] and not st.graphs
    assert gbuf.host_closed == buf.host_closed
    for key in ('u', 'u_onehot', 'o', 'r', 'terminated', 'padded'):
        np.testing.assert_array_equal(gbuf.buffers[key][:len(closed)].cpu().numpy(), buf.buffers[key][:len(closed)].cpu().numpy(),
                                      err_msg=key)
    np.testing.assert_array_equal(gbuf.ring_stats[:len(closed)].cpu().numpy(), stats)
    # the last call's counter is the same; the first call of the graph worker counts its warm-up only
    assert int(gworker.shield_overrides.sum().item()) == int(worker.shield_overrides.sum().item())
    # with the switch off the same worker captures into the other set
    gworker.meda_shield = False
    gworker.generate_steps(gbuf, 45)
    assert list(st.graphs) == [45] and list(st.shield_graphs) == [45]


# ---------------------------------------------------------------------------------------------------- Router and the switch
def _tasks(B, seed=29):
    from marl_dmfb_amd.env.meda import VecMEDA
    env = VecMEDA(n_envs=B, seed=seed, device=DEV, **CFG)
    env.reset()
    s, g = (t.cpu().numpy() for t in env.get_task())
    return env, s, g


def test_router_under_the_meda_shield():
    from marl_dmfb_amd.route import Router
    B = 64
    env, s, g = _tasks(B)
    agents, _ = _agents(env, salt=0.7)
    health = _health(B, 2)
    plain = Router(agents, name='meda', device=DEV, **CFG).route(s, g, health=health, tries=4, epsilon=0.2, seed=3)
    assert plain.overrides is None and (plain.constraints != 0).any()
    router = Router(agents, name='meda', device=DEV, meda_shield=True, **CFG)
    r1 = router.route(s, g, health=health, tries=1, seed=3)
    r4 = router.route(s, g, health=health, tries=4, epsilon=0.2, seed=3)
    for r in (r1, r4):
        assert (r.constraints == 0).all()
        assert r.overrides.dtype == np.int32 and r.overrides.shape == (B,) and r.overrides.sum() > 0
    assert (r4.success >= r1.success).all()
    again = router.route(s, g, health=health, tries=4, epsilon=0.2, seed=3)
    for k in ('positions', 'actions', 'steps', 'success', 'constraints', 'try_index', 'overrides'):
        np.testing.assert_array_equal(getattr(again, k), getattr(r4, k), err_msg=k)


def test_the_switch_is_refused_for_dmfb():
    from marl_dmfb_amd.common.rollout import Evaluator
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.route import Router
    env = VecDMFB(10, 10, 4, fov=9, n_envs=2, device=DEV)
    ev = Evaluator(env, type('A', (), {'n_agents': 4, 'n_actions': 5})(), env.max_step)
    ev.meda_shield = True
    with pytest.raises(ValueError, match='meda_shield'):
        ev._shield_state()
    with pytest.raises(ValueError, match='meda_shield'):
        Router(None, name='dmfb', width=10, length=10, n_agents=4, fov=9, meda_shield=True)
    # the switch is part of every graph key
    ev.meda_shield = False
    keys = [ev.graph_key(True, False), ev.graph_key(False, True), ev.graph_key(True, False, route=True)]
    ev.meda_shield = True
    assert all(a != b for a, b in zip(keys, [ev.graph_key(True, False), ev.graph_key(False, True),
                                             ev.graph_key(True, False, route=True)]))


def test_a_round_with_the_switch_off_is_the_parents():
    """tests/golden/shield_off_meda_round.npz holds switch_off_round() as the commit before the MEDA shield played it (no switch
    existed there): the same seed gives the same bytes in every output."""
    want = np.load(GOLDEN)
    got = switch_off_round()
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert (got['constraints'] != 0).any()      # the round is one the shield would have changed


@pytest.mark.parametrize('mode', ['random', 'tasks'])
def test_evaluate_cli_under_the_meda_shield(tmp_path, mode):
    """`python -m marl_dmfb_amd.evaluate meda --meda_shield`, with random tasks and with given ones: the saved routes carry
    `overrides` and no proximity penalty."""
    import subprocess
    import sys
    from marl_dmfb_amd.env.meda import VecMEDA
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    agents, _ = _agents(VecMEDA(n_envs=1, device=DEV, version=2, **CFG), salt=0.9)   # the CLI's default observation: v0_2
    d = tmp_path / 'model' / 'vdn' / 'fov19'
    d.mkdir(parents=True)
    torch.save(agents.policy.eval_rnn.state_dict(), str(d / 'rnn_net_params.pkl'))
    torch.save(agents.policy.eval_mixer.state_dict(), str(d / 'vdn_net_params.pkl'))
    cmd = [sys.executable, '-m', 'marl_dmfb_amd.evaluate', 'meda', '--fov', '19', '--chip_size', '30', '--drop_num', '4',
           '--model_dir', str(tmp_path / 'model'), '--meda_shield', '--routes', str(tmp_path / 'r.npz')]
    if mode == 'random':
        cmd += ['--evaluate_task', '32']
    else:
        _, s, g = _tasks(8)
        np.savez(tmp_path / 'tasks.npz', starts=s, goals=g)
        cmd += ['--tasks', str(tmp_path / 'tasks.npz'), '--tries', '2']
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert 'The average constraints under the shield is: 0.0' in out.stdout
    with np.load(tmp_path / 'r.npz') as f:
        B = 32 if mode == 'random' else 8
        assert (f['constraints'] == 0).all() and f['overrides'].shape == (B,) and f['overrides'].sum() > 0
