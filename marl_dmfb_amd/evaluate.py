"""`python -m marl_dmfb_amd.evaluate {dmfb,meda}`: the reference's evaluate.py (evaluate.py:7-25 with Evaluator.evaluate,
common/rollout.py:41-85) on the vectorised HIP path, plus the routes.

    python -m marl_dmfb_amd.evaluate dmfb --fov 9 --chip_size 20 --evaluate_task 1000 --routes routes.npz
    python -m marl_dmfb_amd.evaluate dmfb --fov 9 --chip_size 20 --tasks tasks.npz --tries 8 --routes routes.npz

Without --tasks it plays --evaluate_task random greedy episodes, min(evaluate_task, n_envs) chips at a time, and prints the
reference's four lines (a failed episode counts episode_limit steps, as in the reference).  The chip may differ from the one the
model was trained on (--chip_size / --width / --length).  --routes saves the recorded routes of those episodes (.npz: positions
uint8 (N, T+1, n, 2), actions int8 (N, T, n) with -1 after the end, steps (played), success, constraints, starts, goals,
blocks when the chips have any, cfg = (width, length, droplets, fov, stall, blocks)).
With --tasks FILE.npz (starts, goals, optional blocks, health) the given tasks are routed by marl_dmfb_amd.route.Router with
--tries / --epsilon / --seed, and --routes saves their routes with the same keys plus try_index.
--planner fallback (DMFB) hands the tasks the policy fails to the space-time planner (marl_dmfb_amd.plan); --planner only routes
with the planner alone and loads no model; --reserve R / --retries Q give that planner the two opt-in parameters of its rule.
Both also save source (0 policy, 1 planner) and lower_bound, and print the mean steps / lower_bound of the successful routes.
Rendering (--show / --show_save of the reference) stays out of scope."""
import time

import numpy as np
import torch


def _env_info_args(args, env):
    args.__dict__.update(env.get_env_info())
    if args.alg == 'qmix':
        args.state_shape = env.state_shape   # as evaDegre.main: the mixer is loaded with the checkpoint, only the agent network plays
    args.device = str(env.device)


def _make_env(args, n_envs):
    if args.name == 'dmfb':
        from .env.dmfb import VecDMFB
        return VecDMFB(args.width, args.length, args.drop_num, args.block_num, fov=args.fov, stall=args.stall, n_envs=n_envs,
                       seed=args.seed)
    from .env.meda import VecMEDA
    return VecMEDA(args.width, args.length, args.drop_num, fov=args.fov, n_envs=n_envs, seed=args.seed,
                   version=2 if args.version == '0.2' else 0)


def _cfg(args):
    return np.array([args.width, args.length, args.drop_num, args.fov, int(bool(args.stall)),
                     args.block_num if args.name == 'dmfb' else 0], np.int64)


def evaluate_random(args):
    """--evaluate_task random greedy episodes; returns (means (reward, steps, constraints, success), routes dict)."""
    from .agent.agent import Agents
    from .common.rollout import Evaluator
    E = max(1, min(int(args.evaluate_task), int(args.n_envs)))
    env = _make_env(args, E)
    _env_info_args(args, env)
    ev = Evaluator(env, Agents(args), args.episode_limit)
    ev.use_graph = args.use_graph is not False
    ev.shield = bool(getattr(args, 'shield', False))
    ev.meda_shield = bool(getattr(args, 'meda_shield', False))
    T = args.episode_limit
    keep = {k: [] for k in ('reward', 'steps', 'played', 'constraints', 'success', 'positions', 'u', 'starts', 'goals', 'blocks',
                            'overrides')}
    left = int(args.evaluate_task)
    while left > 0:
        m = min(left, E)
        play = ev._play_graphed if ev.use_graph else ev._play
        reward, steps, cons, success, ep, _ = play(0.0, evaluate=True, record=False, route=True)
        starts, goals = env.get_task()
        rows = {'reward': reward, 'steps': steps, 'played': ep['steps'], 'constraints': cons, 'success': success,
                'positions': ep['route'], 'u': ep['u'][..., 0], 'starts': starts, 'goals': goals}
        if args.name == 'dmfb' and args.block_num > 0:
            rows['blocks'] = env.get_blocks()
        if ev.shielded:
            rows['overrides'] = ev.shield_overrides
        for k, v in rows.items():
            keep[k].append(v[:m].cpu().numpy())
        left -= m
    out = {k: np.concatenate(v) for k, v in keep.items() if v}
    means = tuple(float(out[k].astype(np.float64).mean()) for k in ('reward', 'steps', 'constraints', 'success'))
    played = out['played'].astype(np.int64)
    routes = {'positions': out['positions'],
              'actions': np.where(np.arange(T)[None, :, None] < played[:, None, None], out['u'], np.int8(-1)).astype(np.int8),
              'steps': played, 'success': out['success'] > 0,
              'constraints': out['constraints'].astype(np.int64) if args.name == 'dmfb' else out['constraints'],
              'starts': out['starts'], 'goals': out['goals'], 'cfg': _cfg(args)}
    if 'blocks' in out:
        routes['blocks'] = out['blocks']
    if 'overrides' in out:
        routes['overrides'] = out['overrides']
    return means, routes


def _rule(args):
    """--reserve / --retries as keywords of plan.Planner, those that are set."""
    return {k: int(getattr(args, k)) for k in ('reserve', 'retries') if getattr(args, k, 0)}


def _plan_only(args, tasks):
    """--planner only: the tasks through the planner alone, as a RouteResult."""
    from .plan import Planner
    from .route import RouteResult
    args.episode_limit = 2 * (args.width + args.length)
    planner = Planner(args.width, args.length, args.drop_num, **_rule(args))
    plan = planner.plan(tasks['starts'], tasks['goals'], blocks=tasks.get('blocks'), health=tasks.get('health'))
    return RouteResult(plan.positions, plan.actions, plan.steps, plan.success, plan.constraints,
                       np.full(len(plan), -1, np.int32), source=plan.success.astype(np.int8), lower_bound=plan.lower_bound)


def route_tasks(args):
    """The tasks of --tasks through Router (or the planner alone); returns (RouteResult, routes dict)."""
    from .route import Router
    planner = getattr(args, 'planner', 'off')
    if planner != 'off' and args.name != 'dmfb':
        raise ValueError('--planner routes DMFB only')
    with np.load(args.tasks) as f:
        tasks = {k: f[k] for k in f.files}
    for k in ('starts', 'goals'):
        if k not in tasks:
            raise ValueError('%s: missing key %r (keys: starts, goals, optional blocks, health)' % (args.tasks, k))
    if planner == 'only':
        return _with_routes(args, tasks, _plan_only(args, tasks), True)
    from .agent.agent import Agents
    nb = tasks['blocks'].shape[1] if 'blocks' in tasks else 0
    env = _make_env(args, 1)   # the env info the network is built from
    _env_info_args(args, env)
    env.close()
    router = Router(Agents(args), name=args.name, width=args.width, length=args.length, n_agents=args.drop_num, fov=args.fov,
                    n_blocks=max(nb, args.block_num) if args.name == 'dmfb' else 0, stall=args.stall, version=args.version,
                    max_chips=max(int(args.n_envs), int(args.tries)), use_graph=args.use_graph is not False,
                    shield=bool(getattr(args, 'shield', False)), meda_shield=bool(getattr(args, 'meda_shield', False)))
    more = {'fallback': 'plan'} if planner == 'fallback' else {}
    if more and _rule(args):      # the router's own planner has the default rule
        from .plan import Planner
        more['planner'] = Planner(args.width, args.length, args.drop_num, device=router.device, **_rule(args))
    res = router.route(tasks['starts'], tasks['goals'], blocks=tasks.get('blocks'), health=tasks.get('health'), tries=args.tries,
                       epsilon=args.route_epsilon, seed=args.seed, **more)
    return _with_routes(args, tasks, res, bool(more))


def _with_routes(args, tasks, res, planned):
    routes = {'positions': res.positions, 'actions': res.actions, 'steps': res.steps, 'success': res.success,
              'constraints': res.constraints, 'try_index': res.try_index, 'starts': np.asarray(tasks['starts'], np.int32),
              'goals': np.asarray(tasks['goals'], np.int32), 'cfg': _cfg(args)}
    if 'blocks' in tasks:
        routes['blocks'] = np.asarray(tasks['blocks'], np.int32)
    if planned:
        routes['source'], routes['lower_bound'] = res.source, res.lower_bound
    if res.overrides is not None:
        routes['overrides'] = res.overrides
    return res, routes


def _print_shield(constraints, overrides):
    print('The average constraints under the shield is: {}'.format(float(np.mean(constraints)) if len(constraints) else 0.0))
    print('The average picks replaced by the shield is: {}'.format(float(np.mean(overrides)) if len(overrides) else 0.0))


def main(argv=None):
    from .common.arguments import get_route_args
    args = get_route_args(argv)
    start = time.time()
    if args.tasks:
        res, routes = route_tasks(args)
        steps = np.where(res.success, res.steps, args.episode_limit)
        print('time:', time.time() - start)
        print('The average total_steps is: {}'.format(float(steps.mean()) if len(steps) else 0.0))
        print('The successful rate is: {}'.format(float(res.success.mean()) if len(steps) else 0.0))
        if res.lower_bound is not None:
            ok = res.success & (res.lower_bound > 0)
            print('The average steps / lower_bound is: {}'.format(float((res.steps[ok] / res.lower_bound[ok]).mean()) if ok.any()
                                                                  else 0.0))
        if res.overrides is not None:
            _print_shield(res.constraints, res.overrides)
    else:
        (reward, steps, _, success), routes = evaluate_random(args)
        print('time:', time.time() - start)
        print('The average total_rewards of {} is  {}'.format(args.alg, reward))
        print('The average total_steps is: {}'.format(steps))
        print('The successful rate is: {}'.format(success))
        if 'overrides' in routes:
            _print_shield(routes['constraints'], routes['overrides'])
    if args.routes:
        np.savez_compressed(args.routes, **routes)
        print('routes saved to', args.routes)
    return routes


if __name__ == '__main__':
    main()
