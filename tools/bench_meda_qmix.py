"""QMIX on MEDA measurements on one MI355X (profiles/qmix/): python tools/bench_meda_qmix.py --out profiles/qmix/bench_meda.json

  writer      meda_vec_global_obs_append at 30x60 / 4096 chips (us per launch), and the dense meda_vec_global_obs at 30x60 / 131 072
              chips (472 MB written, over the 256 MiB Infinity Cache): bytes written / time against 8 TB/s.
  rounds      rounds of the training loop at 30x30 / 4 droplets / 4096 chips (v0_2, fov 19, 4 learns of 512 episodes), env steps/s:
              VDN in stream mode, QMIX in episode mode and QMIX in stream mode (--meda_state, + --stream_state), interleaved.
  learn       one QMIX learn against one VDN learn (padded, fused TD blocks) at 30x30 / 4 droplets, 512 episodes x 60 steps, and
              the two pieces of the QMIX learn that grow with the state: the int8 -> float32 state conversion and the first-layer
              GEMM of the four hypernetworks (eval and target).
  stage       QMIX stream rounds at 30x60 / 4 droplets or 80x80 / 10 droplets (--stage_cfg), 4096 chips, for a kernel trace of
              their own:  rocprofv3 --kernel-trace --stats -- python tools/bench_meda_qmix.py --only stage --stage_cfg 30x60
              (per lock-step: k_meda_global_obs twice, k_state_close once).
Every figure is a median over repeats, named in the JSON for what it is."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_qmix import timed  # noqa: E402

DEV = 'cuda:0'


def _env(W, L, n, E, seed=1):
    from marl_dmfb_amd.env.meda import VecMEDA
    return VecMEDA(W, L, n, fov=19, n_envs=E, seed=seed, device=DEV, version=2)


def bench_writer(reps=30):
    res = {}
    env = _env(30, 60, 4, 4096)
    env.reset()
    T, S, E = env.max_step, env.state_shape, 4096
    s = torch.zeros((E, T, S), dtype=torch.int8, device=DEV)
    sn = torch.zeros_like(s)
    alive = torch.ones(E, dtype=torch.uint8, device=DEV)
    term = torch.zeros(E, dtype=torch.uint8, device=DEV)
    for _ in range(3):
        env.global_obs_append(alive, term, 1, s, sn)
    ms = float(np.median(timed(lambda: env.global_obs_append(alive, term, 1, s, sn), reps)))
    res['append_30x60_4096'] = {'bytes_written': 2 * S * E, 'us_median': 1e3 * ms, 'share_of_8TBps': 2 * S * E / ms / 1e6 / 8000.0,
                                'timing': 'HIP events around one launch (includes launch overhead)'}
    del s, sn, env
    E = 131072
    env = _env(30, 60, 4, E)
    env.reset()
    out = torch.zeros((E, 2, 30, 60), dtype=torch.int8, device=DEV)
    for _ in range(3):
        env.global_obs(out=out)
    ms = float(np.median(timed(lambda: env.global_obs(out=out), reps)))
    byts = out.numel()
    res['dense_30x60_131072'] = {'bytes_written': byts, 'ms_median': ms, 'GBps': byts / ms / 1e6, 'share_of_8TBps': byts / ms / 1e6 / 8000.0,
                                 'timing': 'HIP events around one launch (includes launch overhead)'}
    return res


def _trainer(alg, stream, E, W=30, L=30, n=4):
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.train import Trainer
    torch.manual_seed(0)
    env = _env(W, L, n, E, seed=5)
    args = make_args(name='meda', drop_num=n, width=W, length=L, fov=19, alg=alg, device=DEV, n_envs=E, batch_size=512, train_time=4,
                     buffer_size=4 * E, stream=stream, stream_state=stream, meda_state=True, **env.get_env_info())
    tr = Trainer(env, args)
    assert tr.stream == stream
    return tr


def bench_rounds(rounds=6, E=4096, reps=3):
    res = {}
    modes = [('vdn', True), ('qmix', False), ('qmix', True)]
    trs = {m: _trainer(m[0], m[1], E) for m in modes}
    for tr in trs.values():
        for _ in range(2):
            tr.collect_and_learn()
    times = {m: [] for m in modes}
    played = {}
    for _ in range(reps):
        for m, tr in trs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            played[m] = sum(tr.collect_and_learn() for _ in range(rounds))
            torch.cuda.synchronize()
            times[m].append(time.perf_counter() - t0)
    for (alg, stream), ts in times.items():
        dt = float(np.median(ts))
        res[alg + ('_stream' if stream else '_episode')] = {'env_steps_per_s': played[(alg, stream)] / dt, 'ms_per_round': 1e3 * dt / rounds}
    res['config'] = ('MEDA 30x30, 4 droplets, v0_2, fov 19, %d chips, 4 learns x 512 episodes per round; median of %d interleaved runs '
                     'of %d rounds' % (E, reps, rounds))
    return res


def bench_learn(reps=20):
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.common.replay_buffer import ReplayBuffer
    from marl_dmfb_amd.common.rollout import RolloutWorker
    res = {}
    for alg in ('vdn', 'qmix'):
        env = _env(30, 30, 4, 512, seed=3)
        args = make_args(name='meda', drop_num=4, width=30, length=30, fov=19, alg=alg, device=DEV, n_envs=512, batch_size=512,
                         buffer_size=512, state_shape=env.state_shape, meda_state=True, **env.get_env_info())
        torch.manual_seed(0)
        ag = Agents(args)
        w = RolloutWorker(env, ag, args)
        buf = ReplayBuffer(args, device=DEV)
        buf.store_episode(w.generate_episode()[4])
        batch = buf.sample(512)
        T = args.episode_limit
        k = [0]

        def learn():
            ag.train({kk: v for kk, v in batch.items()}, k[0], max_len=T)
            k[0] += 1
        for _ in range(5):
            learn()
        res[alg + '_learn_ms_median'] = float(np.median(timed(learn, reps)))
        if alg == 'qmix':
            st = buf.states[:512]
            conv = float(np.median(timed(lambda: st.float(), reps)))
            x = st.float().view(-1, st.shape[-1])
            F_ = 4 * 32   # hyper_w1 / hyper_w2 (hyper_hidden_dim) + hyper_b1 / hyper_b2 (qmix_hidden_dim) first layers
            wt = torch.randn((st.shape[-1], F_), device=DEV)
            gemm = float(np.median(timed(lambda: x.mm(wt), reps)))
            res['state_to_float_ms_median'] = conv
            res['first_layer_gemm_ms_median'] = gemm
            res['first_layer_share_of_learn'] = (conv + 2 * gemm) / res['qmix_learn_ms_median']
    res['shape'] = '512 episodes x 60 steps, MEDA 30x30, 4 droplets, S = 1800; first_layer share = (conversion + 2 GEMMs) / learn'
    return res


def bench_stage(cfg, rounds=10, E=4096):
    W, L, n = {'30x60': (30, 60, 4), '80x80': (80, 80, 10)}[cfg]
    tr = _trainer('qmix', True, E, W=W, L=L, n=n)
    for _ in range(rounds):
        tr.collect_and_learn()
    torch.cuda.synchronize()
    return {'cfg': cfg, 'rounds': rounds, 'lock_steps': rounds * tr.args.episode_limit, 'chips': E,
            'note': 'run under rocprofv3 --kernel-trace --stats; per lock-step: 2 x k_meda_global_obs + 1 x k_state_close'}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    p.add_argument('--only', default='writer,learn,rounds')
    p.add_argument('--stage_cfg', default='30x60', choices=['30x60', '80x80'])
    a = p.parse_args()
    out = {}
    parts = a.only.split(',')
    if 'writer' in parts:
        out['writer'] = bench_writer()
    if 'learn' in parts:
        out['learn'] = bench_learn()
    if 'rounds' in parts:
        out['rounds'] = bench_rounds()
    if 'stage' in parts:
        out['stage'] = bench_stage(a.stage_cfg)
    out['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(out, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
