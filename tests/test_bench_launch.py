"""bench.py --gpus N must start N cooperating ranks by itself when no launcher set WORLD_SIZE
(BASELINE.json metric "1/2/4/8 MI355X").  The CPU test checks the launch plumbing with
`--launch_check` (rendezvous + all-reduces, no GPU work); the GPU test runs the real workload with two ranks
sharing the one card over gloo."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env):
    e = dict(os.environ, **env)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        e.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=e, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=900)


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_gpus_2_spawns_two_ranks():
    p = _run(['--gpus', '2', '--launch_check'], BENCH_DIST_BACKEND='gloo')
    assert p.returncode == 0, p.stderr[-2000:]
    rec = _json_line(p.stdout)
    assert rec['n_gpus'] == 2 and rec['max_rank'] == 1 and rec['asked'] == 2


def test_world_size_mismatch_is_an_error():
    e = dict(os.environ, WORLD_SIZE='3', RANK='0')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--launch_check'], env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode != 0 and 'WORLD_SIZE' in p.stderr


@pytest.mark.gpu
def test_gpus_2_real_workload_on_one_card():
    """Two ranks share the card (gloo carries the collectives): the line must say n_gpus == 2 and the whole-job value
    must count both ranks' chips; with --full rank 0 also times the roofline kernel."""
    p = _run(['--gpus', '2', '--steps', '2', '--warmup', '1', '--n_envs', '512', '--batch_size', '64', '--train_time', '1',
              '--buffer_size', '1024', '--full', '--roofline_envs', '16384', '--roofline_envs_cached', '0'], BENCH_DIST_BACKEND='gloo')
    assert p.returncode == 0, p.stderr[-3000:]
    rec = _json_line(p.stdout)
    assert rec['n_gpus'] == 2
    assert rec['config']['env_steps_per_round'] > 512 * 2  # both shards counted (>= 2 lock-steps per chip)
    assert rec['roofline']['kernel'] == 'dmfbk::k_observe<4>' and rec['roofline']['frac'] > 0
    assert 'cpu_baseline' not in rec
    # a multi-rank line must be diagnosable from the record alone: per-rank round time, env steps, all-reduce time, GEMM mode
    rk = rec['ranks']
    assert len(rk['ms_per_step']) == len(rk['played']) == len(rk['allreduce_ms_per_learn']) == 2
    assert rk['ms_per_step_min'] <= rk['ms_per_step_max'] <= rec['ms_per_step'] * 1.05
    assert sum(rk['played']) == round(rec['config']['env_steps_per_round'] * rec['steps'])
    assert rk['allreduces_timed_per_rank'] == 2 * 1 and min(rk['allreduce_ms_per_learn']) > 0     # steps x train_time
    assert rec['gemm_solutions'].startswith(('tuned', 'library default', 'tuning to'))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only():
    """Without --full the run sets up, warms up, times its rounds and prints the line: none of the figures that take runs
    of their own (roofline kernels, tiers, CPU baseline)."""
    p = _run(['--steps', '2', '--warmup', '1', '--n_envs', '1024', '--batch_size', '128', '--train_time', '2',
              '--buffer_size', '4096'])
    assert p.returncode == 0, p.stderr[-3000:]
    rec = _json_line(p.stdout)
    assert rec['value'] > 0 and rec['ms_per_step'] > 0 and rec['unit'] == 'env-steps/s' and rec['higher_is_better'] is True
    assert rec['metric'].startswith('env-steps/sec') and rec['dtype'] and (rec['steps'], rec['warmup']) == (2, 1)
    assert not {'roofline', 'roofline_loop', 'tiers', 'cpu_baseline'} & set(rec), sorted(rec)


@pytest.mark.gpu
def test_one_rank_over_rccl_reproduces_the_plain_run(tmp_path):
    """The RCCL path with one rank (BENCH_FORCE_DIST=1: process group on the `nccl` backend, parameter broadcast, the flat
    gradient all-reduce of every learn with the next sample queued behind it, the step count riding along): every learn's
    all-reduce is timed, and -- the un-normalised gradients being divided by the (all-reduced) mask count inside the clip + Adam
    kernel on both paths -- the weights after the run equal those of the plain run bit for bit."""
    import torch
    common = ['--steps', '2', '--warmup', '1', '--no_cpu_baseline', '--no_tiers', '--n_envs', '1024', '--batch_size', '128',
              '--train_time', '3', '--buffer_size', '4096', '--roofline_envs', '16384', '--roofline_envs_cached', '0']
    recs, weights = [], []
    for name, env in (('dist', {'BENCH_FORCE_DIST': '1'}), ('plain', {})):
        path = str(tmp_path / (name + '.pt'))
        p = _run(common + ['--dump_weights', path], **env)
        assert p.returncode == 0, p.stderr[-3000:]
        recs.append(_json_line(p.stdout))
        weights.append(torch.load(path))
    dist, plain = recs
    assert dist['n_gpus'] == 1 and 'ranks' in dist and 'ranks' not in plain
    assert dist['ranks']['allreduces_timed_per_rank'] == 2 * 3                 # steps x train_time
    assert dist['ranks']['allreduce_ms_per_learn'][0] > 0
    assert dist['config']['env_steps_per_round'] == plain['config']['env_steps_per_round']
    for k in weights[0]:
        assert torch.equal(weights[0][k], weights[1][k]), 'RCCL one-rank run and plain run differ in %s' % k


@pytest.mark.gpu
def test_dump_outputs_is_the_last_step_and_repeats(tmp_path):
    """--dump-outputs DIR: float32 / float64 .npy files under 64 MB of what the last timed round left (networks after its
    learns, its loss and counters, the replay ring); the same arguments give the same files, and they depend only on how many
    rounds ran, not on how many of them were timed."""
    import numpy as np
    common = ['--no_cpu_baseline', '--no_tiers', '--n_envs', '1024', '--batch_size', '128', '--train_time', '2',
              '--buffer_size', '4096', '--roofline_envs', '16384', '--roofline_envs_cached', '0']
    dumps = {}
    for name, warmup, steps in (('a', 1, 2), ('b', 1, 2), ('c', 2, 1), ('d', 1, 1)):
        d = tmp_path / name
        p = _run(common + ['--warmup', str(warmup), '--steps', str(steps), '--dump-outputs', str(d)])
        assert p.returncode == 0, p.stderr[-3000:]
        rec = _json_line(p.stdout)
        assert rec['steps'] == steps and rec['ms_per_step'] > 0
        files = sorted(os.listdir(d))
        assert sum(os.path.getsize(d / f) for f in files) <= 64e6
        dumps[name] = {f[:-4]: np.load(d / f) for f in files}
        assert all(f.endswith('.npy') for f in files)
        assert all(v.dtype in (np.float32, np.float64) for v in dumps[name].values())
    a = dumps['a']
    for key in ('played', 'loss', 'replay_len', 'replay_stats', 'replay_slots', 'replay_o', 'replay_r'):
        assert key in a, key
    assert any(k.startswith('eval_rnn.') for k in a) and any(k.startswith('target_rnn.') for k in a)
    assert len(a['replay_slots']) > 0 and a['replay_o'].shape[0] == len(a['replay_slots'])
    for other in ('b', 'c'):   # same arguments; the same three rounds split differently between warm-up and timed steps
        assert sorted(dumps[other]) == sorted(a)
        for k in a:
            assert np.array_equal(a[k], dumps[other][k]), '%s differs in run %s' % (k, other)
    assert not all(np.array_equal(a[k], dumps['d'][k]) for k in a if k.startswith('eval_rnn.'))   # two rounds are not three
