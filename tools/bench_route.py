"""Routed tasks per second of marl_dmfb_amd.route.Router with a random-init policy: DMFB 10x10 / 4 droplets / fov 9 with
B = 4096 tasks at K = 1 and K = 8 tries, and MEDA 30x30 / 4 droplets / fov 19 at K = 1.  One JSON line per configuration.
--shield plays the DMFB configurations under the action shield (marl_dmfb_amd.shield) and adds the mean constraints and replaced
picks per task to the line; --meda_shield does the same for the MEDA configuration under the MEDA shield.  A configuration whose
switch is not given is left out when the other is.
`python tools/bench_route.py [--reps N] [--shield] [--meda_shield]`"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def agents_for(env, name):
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    torch.manual_seed(0)
    args = make_args(name=name, drop_num=env.n_agents, width=env.width, length=env.length, fov=env.fov, device='cuda:0',
                     **env.get_env_info())
    return Agents(args)


def run(name, cfg, B, K, reps, shield=False):
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.env.meda import VecMEDA
    from marl_dmfb_amd.route import Router
    Env = VecDMFB if name == 'dmfb' else VecMEDA
    env = Env(n_envs=B, seed=1, device='cuda:0', **cfg)   # random valid tasks, as the env generates them
    env.reset()
    s, g = (t.cpu().numpy() for t in env.get_task())
    router = Router(agents_for(env, name), name=name, device='cuda:0', **{'shield' if name == 'dmfb' else 'meda_shield': shield},
                    **cfg)
    res = router.route(s, g, tries=K, epsilon=0.1, seed=0)   # warm-up: handle, graph capture
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in range(reps):
        res = router.route(s, g, tries=K, epsilon=0.1, seed=r)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    out = {'env': name, 'cfg': cfg, 'tasks': B, 'tries': K, 'ms_per_call': round(dt * 1e3, 3),
           'tasks_per_s': round(B / dt, 1), 'success': round(float(np.mean(res.success)), 4),
           'steps': round(float(np.mean(np.where(res.success, res.steps, router.episode_limit))), 3),
           'constraints': round(float(np.mean(res.constraints)), 4)}
    if shield:
        out.update(shield=True, overrides=round(float(np.mean(res.overrides)), 4))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--tasks', type=int, default=4096)
    p.add_argument('--shield', default=False, action='store_true')
    p.add_argument('--meda_shield', default=False, action='store_true')
    a = p.parse_args()
    dmfb = dict(width=10, length=10, n_agents=4, fov=9)
    meda = dict(width=30, length=30, n_agents=4, fov=19, version=2)
    for name, cfg, K in (('dmfb', dmfb, 1), ('dmfb', dmfb, 8), ('meda', meda, 1)):
        on = a.shield if name == 'dmfb' else a.meda_shield
        if (a.shield or a.meda_shield) and not on:
            continue
        print(json.dumps(run(name, cfg, a.tasks, K, a.reps, on)), flush=True)


if __name__ == '__main__':
    main()
