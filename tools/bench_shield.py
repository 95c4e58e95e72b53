"""Measurements of the action shields (marl_dmfb_amd.shield; profiles/shield/NOTES.md).  One JSON line per result.  DMFB:

    rocprofv3 --kernel-trace --stats -- python tools/bench_shield.py kernel 4     # 300 launches of dmfb_vec_shield at 4096 chips,
    rocprofv3 --kernel-trace --stats -- python tools/bench_shield.py kernel 10    # 4 / 10 droplets: read k_shield off the trace
    python tools/bench_shield.py round [--shield]    # a training round: 40 lock-steps of the continuous rollout, 4096 chips
    python tools/bench_shield.py ckpt                # greedy success / steps / constraints of the recorded checkpoints, both ways

With --meda the same for the MEDA shield (meda_vec_shield, k_meda_shield) on 30x30 chips with 4 droplets (kernel 10: 60x60, 10
droplets), the v0_2 observation and the checkpoint of profiles/r04/train_meda; the round takes --meda_shield, and ckpt also plays
chips whose health is uniform in [0.6, 1).
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

DEV = 'cuda:0'


def kernel(n):
    from marl_dmfb_amd.env.dmfb import VecDMFB
    W, E = (10 if n <= 4 else 20), 4096
    env = VecDMFB(W, W, n, fov=9, n_envs=E, seed=1, device=DEV)
    env.reset()
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    q = torch.randn((E, n, 5), generator=g, device=DEV)
    picks = q.argmax(-1).to(torch.int32)
    last = torch.zeros((E, n, 5), dtype=torch.int8, device=DEV)
    over = torch.zeros(E, dtype=torch.int32, device=DEV)
    for _ in range(300):
        env.shield(q, picks.clone(), last, overrides=over)
    torch.cuda.synchronize()
    print(json.dumps({'what': 'kernel', 'chips': E, 'droplets': n, 'launches': 300,
                      'overrides_per_launch': round(float(over.sum()) / 300, 1)}), flush=True)


def meda_kernel(n):
    from marl_dmfb_amd.env.meda import VecMEDA
    W, E = (30 if n <= 4 else 60), 4096
    env = VecMEDA(W, W, n, fov=19, n_envs=E, seed=1, device=DEV, version=2)
    env.reset()
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    q = torch.randn((E, n, 9), generator=g, device=DEV)
    picks = q.argmax(-1).to(torch.int32)
    for _ in range(8):      # a few random steps: the droplets leave their starts, some reach their disc
        env.step(torch.randint(0, 9, (E, n), generator=g, device=DEV, dtype=torch.int32))
    last = torch.zeros((E, n, 9), dtype=torch.int8, device=DEV)
    over = torch.zeros(E, dtype=torch.int32, device=DEV)
    for _ in range(300):
        env.shield(q, picks.clone(), last, overrides=over)
    torch.cuda.synchronize()
    print(json.dumps({'what': 'kernel', 'env': 'meda', 'chips': E, 'droplets': n, 'launches': 300,
                      'overrides_per_launch': round(float(over.sum()) / 300, 1)}), flush=True)


MEDA_CKPT = 'profiles/r04/train_meda/0_rnn_net_params.pkl'


def _meda_worker(E, seed, health=False, **over):
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.meda import VecMEDA
    env = VecMEDA(30, 30, 4, fov=19, n_envs=E, seed=seed, device=DEV, version=2, with_maps=health)
    if health:
        g = torch.Generator(device=DEV)
        g.manual_seed(seed)
        env.set_map('health', torch.rand((E, 30, 30), generator=g, device=DEV, dtype=torch.float64) * 0.4 + 0.6)
    args = make_args(name='meda', drop_num=4, width=30, length=30, fov=19, device=DEV, n_envs=E, **dict(env.get_env_info(), **over))
    torch.manual_seed(0)
    agents = Agents(args)
    _load(agents, MEDA_CKPT)
    return env, agents, args


def meda_round_ms(shield):
    from marl_dmfb_amd.common.replay_buffer import ReplayBuffer
    from marl_dmfb_amd.common.rollout import RolloutWorker
    E = 4096
    over = dict(meda_shield=True) if shield else {}      # (a tree without the switch takes no such argument)
    env, agents, args = _meda_worker(E, 1, buffer_size=8192, **over)
    w = RolloutWorker(env, agents, args)
    w.use_graph = True
    buf = ReplayBuffer(args, device=DEV)
    for _ in range(3):
        w.generate_steps(buf, 40)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(10):
            w.generate_steps(buf, 40)
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / 10)
    print(json.dumps({'what': 'round', 'env': 'meda', 'shield': bool(shield), 'chips': E, 'ms_per_round_40_steps': round(best * 1e3, 3),
                      'us_per_lock_step': round(best * 1e6 / 40, 1)}), flush=True)


def meda_ckpt():
    from marl_dmfb_amd.common.rollout import Evaluator
    E = 1024
    for health in (False, True):
        for shield in (False, True):
            env, agents, _ = _meda_worker(E, 7, health=health)
            ev = Evaluator(env, agents, env.max_step)
            ev.use_graph, ev.meda_shield = True, shield
            r, s, c, ok = ev.evaluate(4)
            # the env's success already excludes every episode with a proximity event (success = in_time && all && !failed)
            out = {'what': 'ckpt', 'env': 'meda', 'name': 'train_meda', 'health': '[0.6, 1)' if health else '1', 'shield': shield,
                   'chips': E, 'episodes_per_chip': 4, 'reward': round(r, 3), 'steps': round(s, 3), 'constraints': round(c, 4),
                   'success': round(ok, 4)}
            if shield:
                out['overrides_last_episode'] = round(float(ev.shield_overrides.double().mean()), 3)
                out['unsafe_last_episode'] = int(ev.shield_unsafe.sum())
            print(json.dumps(out), flush=True)


def _worker_args(env, n, W, E, **over):
    from marl_dmfb_amd.common.arguments import make_args
    return make_args(drop_num=n, width=W, length=W, fov=9, device=DEV, n_envs=E, **dict(env.get_env_info(), **over))


def _load(agents, path):
    agents.policy.eval_rnn.load_state_dict(torch.load(os.path.join(ROOT, path), map_location=DEV, weights_only=True))


def round_ms(shield):
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.replay_buffer import ReplayBuffer
    from marl_dmfb_amd.common.rollout import RolloutWorker
    from marl_dmfb_amd.env.dmfb import VecDMFB
    E = 4096
    env = VecDMFB(10, 10, 4, fov=9, n_envs=E, seed=1, device=DEV)
    args = _worker_args(env, 4, 10, E, buffer_size=8192, shield=bool(shield))
    torch.manual_seed(0)
    agents = Agents(args)
    _load(agents, 'profiles/r04/train_4d/0_rnn_net_params.pkl')
    w = RolloutWorker(env, agents, args)
    w.use_graph = True
    buf = ReplayBuffer(args, device=DEV)
    for _ in range(3):
        w.generate_steps(buf, 40)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(10):
            w.generate_steps(buf, 40)
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / 10)
    print(json.dumps({'what': 'round', 'shield': bool(shield), 'chips': E, 'ms_per_round_40_steps': round(best * 1e3, 3),
                      'us_per_lock_step': round(best * 1e6 / 40, 1)}), flush=True)


def ckpt():
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.rollout import Evaluator
    from marl_dmfb_amd.env.dmfb import VecDMFB
    cases = [('train_4d', 10, 4, 'profiles/r04/train_4d/0_rnn_net_params.pkl', {}),
             ('train_50x50', 50, 10, 'profiles/r04/train_50x50/0_rnn_net_params.pkl', {}),
             ('degre', 20, 10, 'profiles/r04/degre/model/vdn/fov9/0_rnn_net_params.pkl', dict(b_degrade=True, per_degrade=1.0))]
    E = 1024
    for name, W, n, path, kw in cases:
        for shield in (False, True):
            env = VecDMFB(W, W, n, fov=9, n_envs=E, seed=7, device=DEV, **kw)
            agents = Agents(_worker_args(env, n, W, E))
            _load(agents, path)
            ev = Evaluator(env, agents, env.max_step)
            ev.use_graph, ev.shield = True, shield
            r, s, c, ok = ev.evaluate(4)
            out = {'what': 'ckpt', 'name': name, 'shield': shield, 'chips': E, 'episodes_per_chip': 4, 'reward': round(r, 3),
                   'steps': round(s, 3), 'constraints': round(c, 4), 'success': round(ok, 4)}
            if shield:
                out['overrides_last_episode'] = round(float(ev.shield_overrides.double().mean()), 3)
                out['unsafe_last_episode'] = int(ev.shield_unsafe.sum())
            print(json.dumps(out), flush=True)


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else ''
    meda = '--meda' in sys.argv[2:]
    if what == 'kernel':
        (meda_kernel if meda else kernel)(int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 4)
    elif what == 'round' and meda:
        meda_round_ms('--meda_shield' in sys.argv[2:])
    elif what == 'round':
        round_ms('--shield' in sys.argv[2:])
    elif what == 'ckpt':
        (meda_ckpt if meda else ckpt)()
    else:
        sys.exit(__doc__)
