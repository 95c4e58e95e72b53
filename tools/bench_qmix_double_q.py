"""Measurements of the double-Q targets of the QMIX learn (--qmix_double_q; profiles/qmix_double_q/NOTES.md).  One JSON line per
result.  The run measured is `train dmfb --alg qmix --stream_state --qmix_packed`: the continuous rollout and the packed learn.

    python tools/bench_qmix_double_q.py learn [ROUNDS] [LAMBDA]   # packed learns with the flag off and on at qmix_lambda LAMBDA
                                                                  # (default 0), alternating in one process, on a ring filled by
                                                                  # ROUNDS (default 200) rounds
    python tools/bench_qmix_double_q.py learn ROUNDS LAMBDA off   # the flag off alone (a tree without the knob too)
    rocprofv3 --kernel-trace --stats -- python tools/bench_qmix_double_q.py kernel [off]   # 100 learns each way at lambda 0 and 0.8
                                                                  # ('off': the flag off only): read k_mix_forward<.., MixNoSel> and
                                                                  # <.., MixSel> and the launches per learn off the trace
    python tools/bench_qmix_double_q.py train on|off [train.py flags]   # a training run (default --n_steps 5), greedy success and
                                                                        # steps at every evaluation against the number of learns

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

LAMBDA = 0.8
QMIX = ['dmfb', '--alg', 'qmix', '--stream_state', '--qmix_packed']


def _trainer(argv):
    from marl_dmfb_amd.common.arguments import get_train_args
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.train import Trainer
    args = get_train_args(argv)
    env = VecDMFB(args.width, args.length, args.drop_num, args.block_num, fov=args.fov, stall=args.stall, n_envs=args.n_envs,
                  seed=args.seed)
    args.__dict__.update(env.get_env_info())
    args.state_shape = env.state_shape
    args.device = str(env.device)
    args.buffer_size = max(args.buffer_size, 4 * args.n_envs)
    return Trainer(env, args)


def _filled(rounds):
    tr = _trainer(QMIX)
    for _ in range(rounds):
        tr.collect_and_learn()
    torch.cuda.synchronize()
    assert tr.stream and tr._packed and tr.agents.policy.MIXER == 'qmix', 'the packed QMIX learn on the continuous rollout is measured here'
    return tr


def learn(rounds, lam, both):
    tr = _filled(rounds)
    pol, buf = tr.agents.policy, tr.buffer
    draws = [buf.draw(tr.args.batch_size) for _ in range(8)]
    step = [tr.trained_times]
    modes = (False, True) if both else (False,)
    pol.args.qmix_lambda = lam

    def batch_ms(on, n=16):
        if both:
            pol.args.qmix_double_q = on
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(n):
            idx, lens = draws[k % len(draws)]
            pol.learn_packed(buf.buffers, idx, lens, step[0])
            step[0] += 1
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for on in modes * 2:                       # warm-up, both ways
        batch_ms(on)
    ms = {on: [] for on in modes}
    for _ in range(12):                        # alternating: drift of the clocks hits both modes alike
        for on in modes:
            ms[on].append(batch_ms(on))
    out = {'what': 'learn', 'qmix_lambda': lam, 'rounds_before': rounds, 'episodes_per_learn': int(tr.args.batch_size),
           'learns_per_sample': 16, 'samples': 12, 'units_per_learn': int(sum(int(l.sum()) for _, l in draws) / len(draws))}
    for on, v in ms.items():
        out['ms_per_learn_%s' % ('on' if on else 'off')] = {'mean': round(statistics.mean(v), 4), 'stdev': round(statistics.stdev(v), 4),
                                                            'min': round(min(v), 4), 'max': round(max(v), 4)}
    if both:
        out['difference_ms'] = round(statistics.mean(ms[True]) - statistics.mean(ms[False]), 4)
    pol.check_td_inputs()
    print(json.dumps(out), flush=True)


def kernel(both):
    tr = _filled(20)
    pol, buf = tr.agents.policy, tr.buffer
    step = tr.trained_times
    for on in ((False, True) if both else (False,)):
        if both:
            pol.args.qmix_double_q = on
        for lam in (0.0, LAMBDA):
            pol.args.qmix_lambda = lam
            for _ in range(100):
                idx, lens = buf.draw(tr.args.batch_size)
                pol.learn_packed(buf.buffers, idx, lens, step)
                step += 1
    torch.cuda.synchronize()
    print(json.dumps({'what': 'kernel', 'flag': ['off', 'on'] if both else ['off'], 'lambdas': [0.0, LAMBDA], 'learns_each_way': 100,
                      'episodes_per_learn': int(tr.args.batch_size)}), flush=True)


def train(on, flags):
    import numpy as np
    with tempfile.TemporaryDirectory() as d:
        argv = QMIX + (['--qmix_double_q'] if on else []) + ['--model_dir', os.path.join(d, 'model'), '--result_dir', os.path.join(d, 'result')]
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
        a = tr.args
        print(json.dumps({'what': 'train', 'qmix_double_q': on, 'qmix_lambda': a.qmix_lambda, 'chip': '%dx%d' % (a.width, a.length),
                          'droplets': a.drop_num, 'seed': a.seed, 'learns_at_evaluation': learns,
                          'success': [round(float(x), 4) for x in np.asarray(tr.success_rate).reshape(-1)],
                          'steps': [round(float(x), 3) for x in np.asarray(tr.episode_steps).reshape(-1)]}), flush=True)


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else ''
    if what == 'learn':
        learn(int(sys.argv[2]) if len(sys.argv) > 2 else 200, float(sys.argv[3]) if len(sys.argv) > 3 else 0.0, sys.argv[4:5] != ['off'])
    elif what == 'kernel':
        kernel(sys.argv[2:3] != ['off'])
    elif what == 'train' and len(sys.argv) > 2 and sys.argv[2] in ('on', 'off'):
        train(sys.argv[2] == 'on', sys.argv[3:])
    else:
        sys.exit(__doc__)
