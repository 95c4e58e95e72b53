"""A MEDA policy round for tests/test_gpu_meda_shield.py: the 30x30 / 4 droplet configuration, a deterministic random-init policy,
a seeded health map, and the recorded round whose outputs tests/golden/shield_off_meda_round.npz holds.  This module uses
nothing of the action shield, so that it runs unchanged on a tree without it."""
import numpy as np
import torch

from vdn_helpers import det_init

DEV = 'cuda:0'
CFG = dict(width=30, length=30, n_agents=4, fov=19)


def agents(env, salt=0.25, **over):
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    args = make_args(name='meda', drop_num=env.n_agents, width=env.width, length=env.length, fov=env.fov, device=DEV,
                     **dict(env.get_env_info(), **over))
    a = Agents(args)
    det_init(a.policy.eval_rnn, salt=salt)
    return a, args


def health(E, seed):
    return np.random.default_rng(seed).uniform(0.6, 1.0, (E, 30, 30))


def switch_off_round(E=16, seed=17):
    """One recorded MEDA round with no shield switch set: every output, as integers or the bytes of the floats."""
    from marl_dmfb_amd.common.rollout import RolloutWorker
    from marl_dmfb_amd.env.meda import VecMEDA
    env = VecMEDA(n_envs=E, seed=seed, with_maps=True, device=DEV, **CFG)
    env.set_map('health', health(E, seed))
    a, args = agents(env, n_envs=E)
    worker = RolloutWorker(env, a, args)
    worker.epsilon = torch.tensor(0.3, device=DEV)
    worker.anneal_epsilon, worker.min_epsilon = 0.0, 0.0
    reward, steps, cons, success, ep = worker.generate_episode()
    out = {'reward': reward, 'steps': steps, 'constraints': cons, 'success': success}
    out.update({'ep_' + k: v for k, v in ep.items()})
    return {k: (v.cpu().numpy().view(np.int64) if v.dtype == torch.float64 else
                v.cpu().numpy().view(np.int32) if v.dtype == torch.float32 else v.cpu().numpy()) for k, v in out.items()}
