"""Shared set-up of the fov 5 / 7 GPU tests: a vectorised DMFB env, its Trainer, and the replay of a continuous rollout's
closed episodes through the CPU oracle (the method of tests/test_gpu_rollout_stream.py)."""
import numpy as np
import torch

# the two shapes of the reference's field-of-view sweep (multiTrain.py) this project runs on the HIP front end
SHAPES = {7: dict(W=10, n=3), 5: dict(W=10, n=4)}


def make_trainer(fov, E, seed=7, W=None, n=None, **kw):
    """A GPU Trainer on a W x W chip with n droplets (default: the sweep's shape for this fov)."""
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.train import Trainer
    W, n = W or SHAPES[fov]['W'], n or SHAPES[fov]['n']
    env = VecDMFB(W, W, n, fov=fov, n_envs=E, seed=seed, device='cuda:0')
    args = make_args(device='cuda:0', n_envs=E, drop_num=n if n in (2, 3, 4, 5, 10) else 2, width=W, length=W, fov=fov, **kw,
                     **env.get_env_info())
    args.drop_num = n
    return Trainer(env, args)


def stream_replays_through_oracle(tr, fov, seed, K, eps=1.0, early_ends=True):
    """Runs K lock-steps of the continuous rollout of Trainer `tr` (two calls: episodes straddle the boundary), then replays the
    recorded actions through the CPU oracle and compares every closed episode in the ring bit for bit."""
    from test_gpu_rollout_stream import _compare_ring, _oracle_episodes
    worker, buf, env, args = tr.rolloutWorker, tr.buffer, tr.env, tr.args
    E, n = env.n_envs, args.n_agents
    worker.epsilon = torch.tensor(eps, device='cuda:0')
    worker.anneal_epsilon, worker.min_epsilon = 0.0, 0.0
    steps = []
    worker.stream_step_hook = lambda s, a, term: steps.append((a.cpu().numpy().copy(), term.cpu().numpy().copy()))
    acc = np.zeros(4, np.int64)
    for chunk in (K // 2, K - K // 2):
        acc += np.asarray(buf.sync_host(worker.generate_steps(buf, chunk)))
    cfg = dict(width=env.width, length=env.length, n_agents=n, fov=fov)
    want = _oracle_episodes(cfg, E, seed, steps, args.episode_limit, n, env.obs_len)
    assert len(want) == buf.host_closed == buf.current_size == acc[0] > E
    lens = np.array([d['len'] for d in want])
    if early_ends:   # the case does exercise episodes that end before the step limit
        assert (lens < args.episode_limit).sum() >= 3 and len(set(lens.tolist())) >= 3, lens
    _compare_ring(buf, want)
    assert acc[1] == sum(d['stats'][1] for d in want) and acc[2] == sum(1 for d in want if d['stats'][3])
