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
  packed      the packed QMIX learn (args.qmix_packed; include/qmix_packed.h), written to profiles/qmix/bench_packed.json unless --out
              says otherwise: a QMIX stream run trained for 300 rounds in the script (10x10, 4 droplets, 4096 chips) so that
              episodes end early; from that state one learn, padded against packed, on the same draws, rounds with the flag off
              and on (three interleaved repeats), and the share of valid units; the mixer block forward + backward, padded
              against packed, on one draw of 512 episodes, and the two kernels alone on the same 20 480 rows; qmix_gather_states at 20 992 rows, S = 300 and 1800, beside the
              padded path's .float().contiguous() of 512 x 41 slots.
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


def bench_gather(S, n_rows=20992, slots=2048, T=40, reps=30):
    from marl_dmfb_amd import _lib
    lib = _lib.checked('qmix_packed')
    g = torch.Generator(device=DEV).manual_seed(S)
    ring = torch.randint(-1, 2, (slots, T + 1, S), device=DEV, generator=g, dtype=torch.int8)
    rows = torch.randint(0, slots * (T + 1), (n_rows,), device=DEV, generator=g).to(torch.int32)
    out = torch.empty((n_rows, S), dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def gather():
        lib.qmix_gather_states(ring.data_ptr(), slots * (T + 1), S, rows.data_ptr(), n_rows, out.data_ptr(), stream)
    batch = ring[:512]

    def convert():
        return batch.float().contiguous()
    for _ in range(5):
        gather(); convert()
    assert torch.equal(out, ring.view(-1, S)[rows.long()].float())
    tg, tc = [], []
    for _ in range(reps):
        tg += timed(gather, 1)
        tc += timed(convert, 1)
    ms, byts = float(np.median(tg)), 5.0 * n_rows * S
    cms, cbytes = float(np.median(tc)), 5.0 * 512 * (T + 1) * S
    return {'state_len': S, 'rows': n_rows, 'gather_us_median': 1e3 * ms, 'gather_GBps': byts / ms / 1e6,
            'padded_rows': 512 * (T + 1), 'padded_float_contiguous_us_median': 1e3 * cms, 'padded_GBps': cbytes / cms / 1e6,
            'timing': 'HIP events around one call (includes launch overhead); bytes = 1 read + 4 written per element'}


def bench_packed_mixer(pol, buffers, idx, lens, reps=30):
    """The mixer block (first-layer outputs given) forward + backward on one draw: _MixTD on the gathered (B, T) batch against
    _MixTDPacked on its valid units, random Q values and first-layer outputs."""
    from marl_dmfb_amd.policy.qmix import QMIX, _MixTD, _MixTDPacked
    a, n, A = pol.args, pol.n_agents, pol.n_actions
    H, M = a.hyper_hidden_dim, a.qmix_hidden_dim
    B, T, T_ring, Fc = len(idx), int(lens[0]), buffers['o'].shape[1], 2 * a.hyper_hidden_dim + 2 * a.qmix_hidden_dim
    g = torch.Generator(device=DEV).manual_seed(1)
    counts, units_np = pol.pack_units(idx, lens, T_ring)
    _, target_np = QMIX.pack_state_rows(idx, lens, counts, T_ring)
    U = len(units_np)
    units, target_row = torch.from_numpy(units_np).to(DEV), torch.from_numpy(target_np).to(DEV)
    it = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int64)).to(DEV)
    batch = {k: buffers[k][it][:, :T] for k in ('u', 'r', 'avail_u_next', 'terminated', 'padded')}
    tgt = tuple(t.detach() for t in pol.target_qmix_net.second_layers())
    second = pol.eval_qmix_net.second_layers()
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    Vp = -(-U * n // 64) * 64
    qe_p = torch.randn((Vp, A), device=DEV, generator=g).requires_grad_(True)
    qt_p = torch.randn((Vp, A), device=DEV, generator=g)
    pe_p = torch.randn((U, Fc), device=DEV, generator=g).requires_grad_(True)
    pt_p = torch.randn((U + B, Fc), device=DEV, generator=g)
    qe = torch.randn((T, B * n, A), device=DEV, generator=g).requires_grad_(True)
    qt = torch.randn((T, B * n, A), device=DEV, generator=g)
    pe = torch.randn((B * (T + 1), Fc), device=DEV, generator=g).requires_grad_(True)

    def padded():
        num, _ = _MixTD.apply(qe, pe, *second, qt, pe.detach(), tgt, batch['u'], batch['r'], batch['avail_u_next'], batch['terminated'],
                              batch['padded'], (B, T, n, A, H, M, T + 1, 0, T + 1, 1), a.gamma, bad)
        num.backward()

    def packed():
        num, _ = _MixTDPacked.apply(qe_p, pe_p, *second, qt_p, pt_p, tgt, units, U, target_row, buffers['u'], buffers['r'],
                                    buffers['avail_u_next'], buffers['terminated'], buffers['padded'], (n, A, H, M), a.gamma, bad)
        num.backward()
    for _ in range(5):
        padded(); packed()
    tp, tk = [], []
    for _ in range(reps):
        tp += timed(padded, 1)
        tk += timed(packed, 1)
    return {'episodes': B, 'padded_rows': B * T, 'units': U, 'padded_fwd_bwd_ms_median': float(np.median(tp)),
            'packed_fwd_bwd_ms_median': float(np.median(tk)), 'speedup': float(np.median(tp) / np.median(tk)),
            'what': 'qmix_mix_td_forward / _backward + the second-layer gradient GEMMs, first-layer outputs given'}


def bench_packed_kernels(n, H, A=5, B=512, T=40):
    """The two kernels alone through the C ABI, padded against packed on the SAME rows (every (b, t) row a unit, step-major)."""
    from marl_dmfb_amd import _lib
    M = 32
    g = torch.Generator(device=DEV).manual_seed(0)
    Fc, R = 2 * H + 2 * M, B * T
    rn = lambda *s: torch.randn(s, device=DEV, generator=g)
    mix = lambda: [rn(n * M, H) * .5, rn(n * M), rn(M, H) * .5, rn(M), rn(1, M), rn(1)]
    ev, tg = mix(), mix()
    me, mt = _lib.QmixMixer(*[t.data_ptr() for t in ev]), _lib.QmixMixer(*[t.data_ptr() for t in tg])
    u = torch.randint(0, A, (B, T, n, 1), device=DEV, generator=g, dtype=torch.int8)
    r = rn(B, T, 1)
    avail = torch.ones((B, T, n, A), dtype=torch.int8, device=DEV)
    term = torch.zeros((B, T, 1), dtype=torch.uint8, device=DEV)
    pad = torch.zeros((B, T, 1), dtype=torch.uint8, device=DEV)
    qe, qt = rn(T, B * n, A), rn(T, B * n, A)
    pe = rn(B * (T + 1), Fc)
    mtd, mask = torch.empty(R, device=DEV), torch.empty(R, device=DEV)
    gq, gp = torch.empty(R * n, A, device=DEV), torch.zeros_like(pe)
    z, x = torch.empty(R, n * M + M + 1, device=DEV), torch.empty(R, 2 * H + M + 3, device=DEV)
    g0 = torch.ones(1, device=DEV)
    # packed: step-major units over all rows
    t_idx = torch.arange(T, device=DEV).repeat_interleave(B)
    b_idx = torch.arange(B, device=DEV).repeat(T)
    units = (b_idx * T + t_idx).to(torch.int32)
    pe_p = pe.view(B, T + 1, Fc)[b_idx, t_idx].contiguous()
    trow = (b_idx * (T + 1) + t_idx + 1).to(torch.int32)
    gp_p = torch.empty_like(pe_p)
    mtd_p, mask_p = torch.empty(R, device=DEV), torch.empty(R, device=DEV)
    lo, lp = _lib.checked('qmix_ops'), _lib.checked('qmix_packed')
    p = lambda t: t.data_ptr()
    fwd = lambda: lo.qmix_mix_td_forward(p(qe), p(qt), p(u), p(r), p(avail), p(term), p(pad), B, T, T, n, A, p(pe), T + 1, 0, p(pe), T + 1, 1,
                                         H, M, me, mt, 0.99, p(mtd), p(mask), None, None)
    bwd = lambda: lo.qmix_mix_td_backward(p(mtd), p(mask), p(qe), p(u), B, T, T, n, A, p(pe), T + 1, 0, H, M, me, p(g0), p(gq), p(gp), p(z), p(x), None)
    fwd_p = lambda: lp.qmix_mix_td_forward_packed(p(qe), p(qt), p(units), R, p(u), p(r), p(avail), p(term), p(pad), n, A, p(pe_p), p(pe), p(trow),
                                                  H, M, me, mt, 0.99, p(mtd_p), p(mask_p), None, None)
    bwd_p = lambda: lp.qmix_mix_td_backward_packed(p(mtd_p), p(mask_p), p(qe), p(units), R, p(u), n, A, R * n, p(pe_p), H, M, me, p(g0), p(gq), p(gp_p),
                                                   p(z), p(x), None)
    for f in (fwd, fwd_p, bwd, bwd_p):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    assert torch.equal(mtd.view(B, T).t().reshape(-1), mtd_p)   # unit t * B + b is row b * T + t
    res = {'n': n, 'H': H, 'rows': R}
    for _ in range(2):
        for name, f in (('fwd_padded', fwd), ('fwd_packed', fwd_p), ('bwd_padded', bwd), ('bwd_packed', bwd_p)):
            res[name + '_us'] = 1e3 * float(np.median(timed(f, 30)))
    return res


def bench_packed(train_rounds=300, rounds=8, E=4096, reps=3, learn_reps=20):
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.train import Trainer
    res = {'gather': [bench_gather(300), bench_gather(1800)]}
    torch.manual_seed(0)
    env = VecDMFB(10, 10, 4, fov=9, n_envs=E, seed=5, device=DEV)
    args = make_args(alg='qmix', device=DEV, n_envs=E, batch_size=512, train_time=4, buffer_size=4 * E, stream=True, stream_state=True,
                     qmix_packed=True, anneal_steps=E * 40 * train_rounds * 0.6, **env.get_env_info())
    tr = Trainer(env, args)
    pol, buf = tr.agents.policy, tr.buffer
    t0 = time.perf_counter()
    for _ in range(train_rounds):
        tr.collect_and_learn()
    torch.cuda.synchronize()
    assert tr._packed is True
    pol.check_td_inputs()
    res['training'] = {'rounds': train_rounds, 'seconds': time.perf_counter() - t0, 'last_loss': float(pol.last_loss),
                       'epsilon': float(tr.rolloutWorker.epsilon), 'greedy_eval_reward_steps_constraints_success': [float(v) for v in tr.rolloutWorker.evaluate(2)],
                       'config': '10x10, 4 droplets, fov 9, %d chips, stream_state + qmix_packed, 4 learns x 512 episodes per round' % E}

    def set_flag(on):
        args.qmix_packed, tr._packed = on, on

    # one learn on the same draws: the padded path gathers the batch and learns on (B, longest episode), the packed one reads the ring
    draws = [buf.draw(512) for _ in range(learn_reps)]
    share_trim = float(np.mean([lens.sum() / (len(lens) * lens[0]) for _, lens in draws]))
    share_limit = float(np.mean([lens.sum() / (len(lens) * args.episode_limit) for _, lens in draws]))
    k = [tr.trained_times]

    def learn_padded(d):
        tr.agents.train(buf.gather(d[0]), k[0], max_len=int(d[1][0]))
        k[0] += 1

    def learn_packed(d):
        pol.learn_packed(buf.buffers, d[0], d[1], k[0])
        k[0] += 1
    tp, tk = [], []
    for i, d in enumerate(draws + draws[:3]):      # the first three pairs are the warm-up
        set_flag(False)
        a = timed(lambda: learn_padded(d), 1)
        set_flag(True)
        b = timed(lambda: learn_packed(d), 1)
        if i >= 3:
            tp += a
            tk += b
    res['learn'] = {'padded_learn_ms_median': float(np.median(tp)), 'packed_learn_ms_median': float(np.median(tk)),
                    'speedup': float(np.median(tp) / np.median(tk)), 'valid_share_of_trimmed_rows': share_trim,
                    'valid_share_of_episode_limit_rows': share_limit, 'mean_longest_episode': float(np.mean([d[1][0] for d in draws])),
                    'what': '512 episodes per learn, the same draws for both; padded = ReplayBuffer.gather + QMIX.learn trimmed to the '
                            'longest drawn episode, packed = QMIX.learn_packed on the ring'}
    res['mixer'] = bench_packed_mixer(pol, buf.buffers, *draws[0])
    res['kernels'] = [bench_packed_kernels(4, 24), bench_packed_kernels(10, 32), bench_packed_kernels(16, 32, A=16)]
    # episode mode (stream=False) under the same trained policy: a second trainer with the weights and epsilon of the first
    ep = _round_trainer('qmix', False, E)
    for name in ('eval_rnn', 'target_rnn', 'eval_qmix_net', 'target_qmix_net'):
        getattr(ep.agents.policy, name).load_state_dict(getattr(pol, name).state_dict())
    ep.rolloutWorker.epsilon = tr.rolloutWorker.epsilon.clone() if isinstance(tr.rolloutWorker.epsilon, torch.Tensor) else tr.rolloutWorker.epsilon
    for _ in range(3):
        ep.collect_and_learn()
    modes = [('qmix_stream', tr, False), ('qmix_stream_packed', tr, True), ('qmix_episode', ep, None)]
    times = {m[0]: [] for m in modes}
    played = {}
    for _ in range(reps):
        for name, t, flag in modes:
            if flag is not None:
                set_flag(flag)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            played[name] = sum(t.collect_and_learn() for _ in range(rounds))
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    for name, _, _ in modes:
        dt = float(np.median(times[name]))
        res[name] = {'env_steps_per_s': played[name] / dt, 'ms_per_round': 1e3 * dt / rounds, 'env_steps_per_round': played[name] / rounds,
                     'runs_s': times[name]}
    res['rounds_config'] = ('the trained run above with the flag off / on, and episode mode (stream=False) with its weights and '
                            'epsilon, interleaved; median of %d runs of %d rounds' % (reps, rounds))
    return res


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
    if 'packed' in parts:
        out['packed'] = bench_packed()
        if a.out is None and parts == ['packed']:
            a.out = os.path.join(ROOT, 'profiles', 'qmix', 'bench_packed.json')
    out['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(out, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
