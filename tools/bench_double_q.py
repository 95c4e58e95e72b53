"""Measurements of the double-Q targets of the VDN learn (--double_q; profiles/double_q/NOTES.md).  One JSON line per result.

    python tools/bench_double_q.py learn [ROUNDS]       # packed learns with double_q off and on, alternating in one process, on a ring
                                                        # filled by ROUNDS (default 200) rounds of the default config
    rocprofv3 --kernel-trace --stats -- python tools/bench_double_q.py kernel     # 100 learns each way: read k_td_forward<PackedIndex>
                                                                                  # and k_td_double_forward<PackedIndex> off the trace
                                                                                  # (counters, if wanted, in a run of their own)
    python tools/bench_double_q.py train {0,1} [train.py flags]     # a training run (default --n_steps 5) with --double_q off / on, greedy
                                                                    # success and steps at every evaluation against the number of learns

The default config: 10x10 chips, 4 droplets, 4096 chips, 512 episodes per learn.
"""
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def _trainer(argv):
    from marl_dmfb_amd.common.arguments import get_train_args
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.train import Trainer
    args = get_train_args(argv)
    env = VecDMFB(args.width, args.length, args.drop_num, args.block_num, fov=args.fov, stall=args.stall, n_envs=args.n_envs,
                  seed=args.seed)
    args.__dict__.update(env.get_env_info())
    args.device = str(env.device)
    args.buffer_size = max(args.buffer_size, 4 * args.n_envs)
    return Trainer(env, args)


def _filled(rounds):
    tr = _trainer(['dmfb'])
    for _ in range(rounds):
        tr.collect_and_learn()
    torch.cuda.synchronize()
    assert tr.stream and tr._packed, 'the packed learn on the continuous rollout is the path measured here'
    return tr


def learn(rounds):
    tr = _filled(rounds)
    pol, buf = tr.agents.policy, tr.buffer
    draws = [buf.draw(tr.args.batch_size) for _ in range(8)]
    step = [tr.trained_times]

    def batch_ms(on, n=16):
        pol.args.double_q = on
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(n):
            idx, lens = draws[k % len(draws)]
            pol.learn_packed(buf.buffers, idx, lens, step[0])
            step[0] += 1
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for on in (False, True, False, True):      # warm-up, both ways
        batch_ms(on)
    ms = {False: [], True: []}
    for _ in range(12):                        # alternating: drift of the clocks hits both modes alike
        for on in (False, True):
            ms[on].append(batch_ms(on))
    out = {'what': 'learn', 'rounds_before': rounds, 'episodes_per_learn': int(tr.args.batch_size), 'learns_per_sample': 16, 'samples': 12,
           'units_per_learn': int(sum(int(l.sum()) for _, l in draws) / len(draws))}
    for on, v in ms.items():
        out['ms_per_learn_double_q_%s' % ('on' if on else 'off')] = {'mean': round(statistics.mean(v), 4), 'stdev': round(statistics.stdev(v), 4),
                                                                     'min': round(min(v), 4), 'max': round(max(v), 4)}
    out['difference_ms'] = round(statistics.mean(ms[True]) - statistics.mean(ms[False]), 4)
    print(json.dumps(out), flush=True)


def kernel():
    tr = _filled(20)
    pol, buf = tr.agents.policy, tr.buffer
    step = tr.trained_times
    for on in (False, True):
        pol.args.double_q = on
        for _ in range(100):
            idx, lens = buf.draw(tr.args.batch_size)
            pol.learn_packed(buf.buffers, idx, lens, step)
            step += 1
    torch.cuda.synchronize()
    print(json.dumps({'what': 'kernel', 'learns_each_way': 100, 'episodes_per_learn': int(tr.args.batch_size)}), flush=True)


def train(on, flags):
    import numpy as np
    with tempfile.TemporaryDirectory() as d:
        argv = ['dmfb', '--model_dir', os.path.join(d, 'model'), '--result_dir', os.path.join(d, 'result')] + (['--double_q'] if on else [])
        if '--n_steps' not in flags:
            argv += ['--n_steps', '5']
        tr = _trainer(argv + flags)
        learns = []
        record = tr._evaluate_and_record

        def recording(*a, **k):
            learns.append(tr.trained_times)
            return record(*a, **k)
        tr._evaluate_and_record = recording
        tr.run(online_evaluate=True)
        torch.cuda.synchronize()
        tr.agents.policy.check_td_inputs()
        a = tr.args
        print(json.dumps({'what': 'train', 'double_q': bool(a.double_q), 'td_lambda': a.td_lambda, 'chip': '%dx%d' % (a.width, a.length),
                          'droplets': a.drop_num, 'seed': a.seed, 'packed_learn': bool(tr._packed), 'learns_at_evaluation': learns,
                          'success': [round(float(x), 4) for x in np.asarray(tr.success_rate).reshape(-1)],
                          'steps': [round(float(x), 3) for x in np.asarray(tr.episode_steps).reshape(-1)]}), flush=True)


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else ''
    if what == 'learn':
        learn(int(sys.argv[2]) if len(sys.argv) > 2 else 200)
    elif what == 'kernel':
        kernel()
    elif what == 'train' and len(sys.argv) > 2 and sys.argv[2] in ('0', '1'):
        train(sys.argv[2] == '1', sys.argv[3:])
    else:
        sys.exit(__doc__)
