"""QMIX measurements on one MI355X (profiles/qmix/): python tools/bench_qmix.py --out profiles/qmix/bench.json

  mix_td      fused mixing / TD block (first-layer GEMMs + qmix_mix_td_forward / _backward + second-layer GEMMs) against the
              torch-op QMixNet path, forward + backward, 20 480 rows (512 episodes x 40 steps) at 4d and 10d shapes; HIP events,
              the two alternating after a warm-up.
  learn       one QMIX learn (fused path) against one padded VDN learn (fused TD block) at the bench learn shape
              (10x10, 4 droplets, 512 episodes x 40 steps).
  append      dmfb_vec_global_obs_append at 262 144 chips (10x10): bytes written / time against 8 TB/s.
  rounds      rounds of the training loop (HIP-graph rollout, 4 learns of 512 episodes) at the bench config, env steps/s: VDN and
              QMIX in episode mode (stream=False), VDN in stream mode and QMIX in stream mode (stream_state=True: the global state
              staged per chip and closed into the ring, include/dmfb_vec.h: dmfb_vec_global_obs_stage_first / _close).
  stage       QMIX stream rounds only, for a kernel trace of their own:
              rocprofv3 --kernel-trace --stats -- python tools/bench_qmix.py --only stage
              (k_global_obs runs twice and k_state_close once per lock-step; the round count is printed).
Every figure is a median over repeats, named in the JSON for what it is."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = 'cuda:0'


def timed(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def bench_mix(n, hh, W, reps=30):
    from marl_dmfb_amd.policy.qmix import QMIX
    from qmix_helpers import qmix_agents
    B, T, A = 512, 40, 5
    ag = qmix_agents(W, W, n, 9, DEV)
    pol = ag.policy
    assert pol.args.hyper_hidden_dim == hh
    g = torch.Generator(device=DEV).manual_seed(0)
    S = 3 * W * W
    st = (torch.rand((B, T + 1, S), device=DEV, generator=g) < 2.0 * n / S).to(torch.int8)
    batch = {'u': torch.randint(0, A, (B, T, n, 1), device=DEV, generator=g, dtype=torch.int8),
             'r': torch.randn((B, T, 1), device=DEV, generator=g),
             'avail_u_next': torch.ones((B, T, n, A), dtype=torch.int8, device=DEV),
             'terminated': torch.zeros((B, T, 1), dtype=torch.bool, device=DEV),
             'padded': torch.zeros((B, T, 1), dtype=torch.bool, device=DEV),
             's': st[:, :T], 's_next': st[:, 1:]}
    q_e = torch.randn((T, B * n, A), device=DEV, generator=g).requires_grad_(True)
    q_t = torch.randn((T, B * n, A), device=DEV, generator=g)

    def fused():
        num, _ = pol._mix_td_fused(q_e, q_t, batch, T)
        num.backward()

    def torch_ops():
        u = batch['u'].long()
        qe = q_e.view(T, B, n, A).permute(1, 0, 2, 3)
        qt = q_t.view(T, B, n, A).permute(1, 0, 2, 3)
        qg = torch.gather(qe, 3, u).squeeze(3)
        qm = qt.masked_fill(batch['avail_u_next'] == 0, -9999999).max(3)[0]
        tot_e = pol.eval_qmix_net(qg, batch['s'].float())
        with torch.no_grad():
            tot_t = pol.target_qmix_net(qm, batch['s_next'].float())
        targets = batch['r'] + 0.99 * tot_t * (1 - batch['terminated'].float())
        mask = 1 - batch['padded'].float()
        ((mask * (tot_e - targets.detach())) ** 2).sum().backward()
    for _ in range(5):
        fused(); torch_ops()
    tf, tt = [], []
    for _ in range(reps):   # alternating
        tf += timed(fused, 1)
        tt += timed(torch_ops, 1)
    assert isinstance(pol, QMIX)
    return {'rows': B * T, 'n': n, 'hyper_hidden': hh, 'state': S, 'fused_fwd_bwd_ms_median': float(np.median(tf)),
            'torch_ops_fwd_bwd_ms_median': float(np.median(tt)), 'speedup': float(np.median(tt) / np.median(tf))}


def bench_learn(reps=20):
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.common.replay_buffer import ReplayBuffer
    from marl_dmfb_amd.env.dmfb import VecDMFB
    res = {}
    for alg in ('vdn', 'qmix'):
        env = VecDMFB(10, 10, 4, fov=9, n_envs=512, seed=3, device=DEV)
        args = make_args(alg=alg, device=DEV, n_envs=512, batch_size=512, buffer_size=512, state_shape=env.state_shape,
                         **env.get_env_info())
        ag = Agents(args)
        from marl_dmfb_amd.common.rollout import RolloutWorker
        w = RolloutWorker(env, ag, args)
        buf = ReplayBuffer(args, device=DEV)
        buf.store_episode(w.generate_episode()[4])
        batch = buf.sample(512)
        T = 40
        k = [0]

        def learn():
            ag.train({kk: v for kk, v in batch.items()}, k[0], max_len=T)
            k[0] += 1
        for _ in range(5):
            learn()
        res[alg + '_learn_ms_median'] = float(np.median(timed(learn, reps)))
    res['shape'] = '512 episodes x 40 steps, 10x10, 4 droplets'
    return res


def bench_append(E=262144, reps=30):
    from marl_dmfb_amd.env.dmfb import VecDMFB
    env = VecDMFB(10, 10, 4, fov=9, n_envs=E, seed=1, device=DEV)
    env.reset()
    T, S = 4, env.state_shape
    s = torch.zeros((E, T, S), dtype=torch.int8, device=DEV)
    sn = torch.zeros_like(s)
    alive = torch.ones(E, dtype=torch.uint8, device=DEV)
    term = torch.zeros(E, dtype=torch.uint8, device=DEV)
    for _ in range(3):
        env.global_obs_append(alive, term, 1, s, sn)
    ms = float(np.median(timed(lambda: env.global_obs_append(alive, term, 1, s, sn), reps)))
    byts = 2 * S * E
    return {'chips': E, 'bytes_written': byts, 'ms_median': ms, 'GBps': byts / ms / 1e6, 'share_of_8TBps': byts / ms / 1e6 / 8000.0,
            'timing': 'HIP events around one launch (includes launch overhead)'}


def _round_trainer(alg, stream, E):
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.train import Trainer
    torch.manual_seed(0)
    env = VecDMFB(10, 10, 4, fov=9, n_envs=E, seed=5, device=DEV)
    args = make_args(alg=alg, device=DEV, n_envs=E, batch_size=512, train_time=4, buffer_size=4 * E, stream=stream,
                     stream_state=stream, **env.get_env_info())
    tr = Trainer(env, args)
    assert tr.stream == stream
    return tr


def bench_rounds(rounds=8, E=4096, reps=3):
    """Median over `reps` timed runs of `rounds` rounds per mode, the modes interleaved run by run."""
    res = {}
    modes = [('vdn', False), ('qmix', False), ('vdn', True), ('qmix', True)]
    trs = {m: _round_trainer(m[0], m[1], E) for m in modes}
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
        res[alg + ('_stream' if stream else '')] = {'env_steps_per_s': played[(alg, stream)] / dt, 'ms_per_round': 1e3 * dt / rounds}
    res['config'] = ('10x10, 4 droplets, fov 9, %d chips, 4 learns x 512 episodes per round; vdn / qmix: stream=False, '
                     'vdn_stream: stream=True, qmix_stream: stream=True + stream_state=True; median of %d runs of %d rounds' % (E, reps, rounds))
    return res


def bench_stage(rounds=20, E=4096):
    tr = _round_trainer('qmix', True, E)
    for _ in range(rounds):
        tr.collect_and_learn()
    torch.cuda.synchronize()
    return {'rounds': rounds, 'lock_steps': rounds * tr.args.episode_limit, 'chips': E,
            'note': 'run under rocprofv3 --kernel-trace --stats; per lock-step: 2 x k_global_obs + 1 x k_state_close'}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    p.add_argument('--only', default='mix,learn,append,rounds')
    a = p.parse_args()
    out = {}
    parts = a.only.split(',')
    if 'mix' in parts:
        out['mix_td'] = [bench_mix(4, 24, 10), bench_mix(10, 32, 20)]
    if 'learn' in parts:
        out['learn'] = bench_learn()
    if 'append' in parts:
        out['append'] = bench_append()
    if 'rounds' in parts:
        out['rounds'] = bench_rounds()
    if 'stage' in parts:
        out['stage'] = bench_stage()
    out['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(out, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
