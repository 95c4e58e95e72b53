"""Planned tasks per second of marl_dmfb_amd.plan.Planner (include/route_plan.h) with B = 4096 tasks on DMFB 10x10 / 4 droplets,
20x20 / 10 and 50x50 / 10: the whole call (upload, kernel, download) and the kernel alone (device events around the launch),
plan_reference on one core over the first --ref-tasks of the same tasks, the planner's success share and mean steps / lower
bound.  With --model_dir (and --alg / --fov / --chip_size / -d as `python -m marl_dmfb_amd.evaluate`) a policy-vs-planner table
for that checkpoint follows: success share, mean steps and mean steps / lower bound of the policy, the planner and the policy
with the planner as fallback.  One JSON line per row.
`python tools/bench_plan.py [--reps N] [--tasks B] [--reserve R] [--retries Q|n] [--model_dir DIR ...]`

`--reserve R` / `--retries Q` (DMFB, with and without --follow) measure the rule with reservations over R levels and Q retries
(`--retries n`: as many as the config has droplets); every row then names them, and the kernel is timed through
route_plan_dmfb_opt, also at 0 / 0.

`--meda` measures marl_dmfb_amd.plan.MedaPlanner (include/meda_plan.h) instead, on MEDA 30x30 / 4 droplets, 30x60 / 8 and 60x60 / 16
against plan_reference_meda, and prints the policy-vs-planner table of a random-init policy on 30x30 / 4 (Router.route with
planner=MedaPlanner(...)).

`--meda --wide` measures marl_dmfb_amd.plan.MedaWidePlanner (include/meda_plan_wide.h) on MEDA 80x80 / 10 droplets and 128x128 / 16,
and runs 60x60 / 16 through the wide and the narrow planner as calibration.  A wide row also names the levels the LDS holds, the
tasks whose last arrival lies beyond them and the tasks with a failed search (attempt != 0: a search that finds no route runs
to the last level); both kinds reach the workspace.

`--follow` measures the closed-loop router (marl_dmfb_amd.plan.Follower, include/route_plan.h: route_follow_dmfb) on the three DMFB
shapes: ms per episode and tasks/s of a captured-graph episode on healthy chips (beside T env steps alone) and on health uniform
in [0.6, 1) with min_health 0, 0.5 and 0.8: replans per episode, success,
steps / lower bound and the gave-up share.

`--meda --follow` measures the MEDA closed loop (marl_dmfb_amd.plan.MedaFollower, include/meda_follow.h: meda_follow_step) on 30x30 / 4
and 30x60 / 8: ms per call of MedaFollower.play, eager and as a captured graph, and of MedaPlanner.follow (numpy in and out) on
healthy chips and on health uniform in [0.6, 1), with the success share of the closed loop beside that of the open-loop planner
(MedaPlanner.plan(health=...), plain and safe rule) on the same tasks.

`--meda --wide --follow` measures the wide closed loop (marl_dmfb_amd.plan.MedaWideFollower, include/meda_follow_wide.h:
meda_follow_wide_step) on 80x80 / 10 and 128x128 / 16 (the latter on at most 1024 of the tasks: a worn chip with 16 droplets is
replanned at almost every one of its 256 lock-steps), and runs 60x60 / 8 through the wide and the narrow follower as calibration:
ms per episode batch eager and as a captured graph on health uniform in [0.6, 1), the healthy-chip time, the routed and gave-up
shares, plans per episode, and follow_reference_meda on one core over the first tasks (--ref-tasks, at most 8; none at
128x128 / 16, where one chip takes it minutes) with whether the kernel's episodes equal it."""
import argparse
import functools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = 'cuda:0'
FOLLOW_FIELDS = ('positions', 'actions', 'steps', 'success', 'constraints', 'replans', 'gave_up', 'lower_bound')


def make_env(meda, width, length, n_agents, B, seed, **kw):
    """The vectorised env the planners' tables use: VecDMFB fov 5, or VecMEDA fov 19."""
    if meda:
        from marl_dmfb_amd.env.meda import VecMEDA
        return VecMEDA(width, length, n_agents, fov=19, n_envs=B, seed=seed, device=DEV, **kw)
    from marl_dmfb_amd.env.dmfb import VecDMFB
    return VecDMFB(width, length, n_agents, fov=5, n_envs=B, seed=seed, device=DEV, **kw)


def tasks_for(width, length, n_agents, B, seed=1, meda=False):
    env = make_env(meda, width, length, n_agents, B, seed)   # random valid tasks, as the env draws them
    env.reset()
    return tuple(t.cpu().numpy() for t in env.get_task())


def quality(res):
    ok = res.success & (res.lower_bound > 0)
    return {'success': round(float(res.success.mean()), 4),
            'mean_steps': round(float(res.steps[res.success].mean()), 3) if res.success.any() else None,
            'steps_over_lower_bound': round(float((res.steps[ok] / res.lower_bound[ok]).mean()), 4) if ok.any() else None}


def kinds():
    """Per env: the task drawer, the planner class, the reference, the library call (name, function and what it takes before
    the starts and after the goals), T and the `cfg` prefix.  `rule`: does it take reserve / retries (then after the outputs)?"""
    from marl_dmfb_amd import plan
    return {
        'dmfb': dict(tasks=tasks_for, planner=plan.Planner, reference=plan.plan_reference, lib='route_plan', fn='route_plan_dmfb_opt',
                     pre=(0,), post=(None, None), T=lambda w, l: 2 * (w + l), prefix='', rule=True),
        'meda': dict(tasks=functools.partial(tasks_for, meda=True), planner=plan.MedaPlanner, reference=plan.plan_reference_meda, lib='meda_plan',
                     fn='meda_plan_route', pre=(), post=(None,), T=lambda w, l: w + l, prefix='meda ', rule=False),
        'wide': dict(tasks=functools.partial(tasks_for, meda=True), planner=plan.MedaWidePlanner, reference=plan.plan_reference_meda,
                     lib='meda_plan_wide', fn='meda_plan_wide_route', pre=(0,), post=(None,), T=lambda w, l: w + l, prefix='meda wide ',
                     rule=False, work=True),
    }


def rule_for(a, n):
    """{'reserve': R, 'retries': Q} of the command line for a config with n droplets."""
    return {'reserve': a.reserve, 'retries': n if a.retries == 'n' else int(a.retries)}


def kernel_ms(kind, width, length, n, s, g, reps, rule):
    """The launch alone: inputs and outputs stay on the device, device events around `reps` launches."""
    from marl_dmfb_amd import _lib
    fn = getattr(_lib.checked(kind['lib']), kind['fn'])
    B, T = s.shape[0], kind['T'](width, length)
    d_s, d_g = torch.as_tensor(s, device=DEV), torch.as_tensor(g, device=DEV)
    pos = torch.empty((B, T + 1, n, 2), dtype=torch.uint8, device=DEV)
    u = torch.empty((B, T, n), dtype=torch.int8, device=DEV)
    i32 = [torch.empty(B, dtype=torch.int32, device=DEV) for _ in range(3)]
    ok = torch.empty(B, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    tail = (rule['reserve'], rule['retries']) if kind['rule'] else ()
    if kind.get('work'):   # the workspace, its size and lds_levels = 0 (as many levels in LDS as fit)
        need = _lib.meda_plan_wide().meda_plan_wide_work_bytes(B, width, length, n, 0)
        work = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
        tail = (work.data_ptr(), need, 0)
    call = lambda: fn(B, width, length, n, *kind['pre'], d_s.data_ptr(), d_g.data_ptr(), *kind['post'], pos.data_ptr(),
                      u.data_ptr(), i32[0].data_ptr(), ok.data_ptr(), i32[1].data_ptr(), i32[2].data_ptr(), *tail, stream)
    call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(kind, width, length, n, B, reps, ref_tasks, rule):
    s, g = kind['tasks'](width, length, n, B)
    more = rule if kind['rule'] else {}
    planner = kind['planner'](width, length, n, device=DEV, **more)
    res = planner.plan(s, g)   # warm-up: the code object
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        res = planner.plan(s, g)
    dt = (time.perf_counter() - t0) / reps
    k_ms = kernel_ms(kind, width, length, n, s, g, reps, rule)
    m = min(ref_tasks, B)
    t0 = time.perf_counter()
    ref = kind['reference'](width, length, s[:m], g[:m], **more)
    ref_dt = (time.perf_counter() - t0) / m
    same = all(np.array_equal(getattr(ref, k), getattr(res, k)[:m]) for k in ('positions', 'actions', 'steps', 'attempt'))
    row = {'cfg': '%s%dx%d/%d' % (kind['prefix'], width, length, n), 'tasks': B, 'ms_per_call': round(dt * 1e3, 3),
           'tasks_per_s': round(B / dt, 1), 'kernel_ms': round(k_ms, 3), 'kernel_tasks_per_s': round(B / (k_ms * 1e-3), 1),
           'reference_tasks_per_s_one_core': round(1.0 / ref_dt, 1), 'equals_reference': bool(same)}
    row.update(quality(res))
    row.update(more)
    if kind.get('work'):
        from marl_dmfb_amd import _lib
        H = _lib.meda_plan_wide().meda_plan_wide_lds_levels(width, length, n)
        row.update({'lds_levels': H, 'levels': kind['T'](width, length) - 2,
                    'tasks_arriving_past_lds_levels': int((res.steps - 1 > H).sum()), 'tasks_with_a_failed_search': int((res.attempt != 0).sum())})
    return row


def meda_policy_table(B):
    """A random-init policy (no MEDA checkpoint ships with the repository) against the planner, 30x30 / 4."""
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.meda import VecMEDA
    from marl_dmfb_amd.plan import MedaPlanner
    from marl_dmfb_amd.route import Router
    cfg = dict(width=30, length=30, n_agents=4, fov=19)
    probe = VecMEDA(n_envs=1, device=DEV, **cfg)
    torch.manual_seed(0)
    agents = Agents(make_args(name='meda', drop_num=4, width=30, length=30, fov=19, device=DEV, alg='vdn', **probe.get_env_info()))
    s, g = tasks_for(30, 30, 4, B, seed=2, meda=True)
    router = Router(agents, name='meda', device=DEV, **cfg)
    planner = MedaPlanner(30, 30, 4, device=DEV)
    yield dict(row='meda planner', **quality(planner.plan(s, g)))
    for K in (1, 8):
        for fb in (None, 'plan'):
            res = router.route(s, g, tries=K, seed=0, fallback=fb, lower_bound=True, planner=planner)
            yield dict(row='meda random-init policy tries=%d%s' % (K, ' + planner fallback' if fb else ''), **quality(res))


def policy_table(argv, B):
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import get_route_args
    from marl_dmfb_amd.evaluate import _env_info_args, _make_env
    from marl_dmfb_amd.plan import Planner
    from marl_dmfb_amd.route import Router
    args = get_route_args(argv)
    env = _make_env(args, 1)
    _env_info_args(args, env)
    env.close()
    s, g = tasks_for(args.width, args.length, args.drop_num, B, seed=2)
    router = Router(Agents(args), name='dmfb', width=args.width, length=args.length, n_agents=args.drop_num, fov=args.fov,
                    stall=args.stall, device=DEV)
    plan = Planner(args.width, args.length, args.drop_num, device=DEV).plan(s, g)
    yield dict(row='planner', **quality(plan))
    for K in (1, 8):
        for fb in (None, 'plan'):
            res = router.route(s, g, tries=K, seed=0, fallback=fb, lower_bound=True)
            yield dict(row='policy tries=%d%s' % (K, ' + planner fallback' if fb else ''), **quality(res))


def follow_setup(meda, width, length, n, B, reps, **kw):
    """What both closed-loop tables start from: (tasks, a handle with maps that holds them, seeded move draws (T, B, n), a worn
    health map uniform in [0.6, 1), `timed(fn)` = seconds per call over `reps` calls after one warm-up)."""
    s, g = tasks_for(width, length, n, B, meda=meda)
    T = width + length if meda else 2 * (width + length)
    env = make_env(meda, width, length, n, B, 0, with_maps=True, **kw)
    env.set_task(s, g)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    draws = torch.empty((T, B, n), dtype=torch.float64, device=DEV).uniform_(0.0, 1.0, generator=gen)
    worn = torch.empty((B, width, length), dtype=torch.float64, device=DEV).uniform_(0.6, 1.0, generator=gen)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    return (s, g), env, draws, worn, timed


def follow_quality(res):
    ok = res.success & (res.lower_bound > 0)
    return {'success': round(float(res.success.float().mean()), 4), 'gave_up': round(float(res.gave_up.float().mean()), 4),
            'replans_per_episode': round(float(res.replans.float().mean()), 3),
            'steps_over_lower_bound': round(float((res.steps[ok].double() / res.lower_bound[ok]).mean()), 4) if ok.any() else None}


def follow_rows(width, length, n, B, reps, rule):
    from marl_dmfb_amd.plan import Follower
    _, env, draws, worn, timed = follow_setup(False, width, length, n, B, reps)

    def steps_alone():
        env.restart()
        a = torch.zeros((B, n), dtype=torch.int32, device=DEV)
        for t in range(len(draws)):
            env.step(a, draws[t], record=False)

    cfg = '%dx%d/%d' % (width, length, n)
    yield {'cfg': cfg, 'row': 'T env steps alone (eager)', 'ms': round(timed(steps_alone) * 1e3, 3)}
    for label, health, min_health in (('healthy', None, 0.0), ('health [0.6, 1)', worn, 0.0), ('health [0.6, 1)', worn, 0.5),
                                      ('health [0.6, 1)', worn, 0.8)):
        env.set_map('health', torch.ones_like(worn) if health is None else health)
        f = Follower(env, min_health=min_health, use_graph=True, **rule)
        run = lambda: (env.restart(), f.play(uniforms=draws, record=False))[1]
        dt = timed(run)
        row = {'cfg': cfg, 'row': 'follow, ' + label, 'min_health': min_health, 'tasks': B, 'ms_per_episode': round(dt * 1e3, 3),
               'tasks_per_s': round(B / dt, 1)}
        row.update(follow_quality(run()))
        row.update(rule)
        yield row


def meda_follow_rows(width, length, n, B, reps):
    from marl_dmfb_amd.plan import MedaFollower, MedaPlanner
    (s, g), env, draws, worn, timed = follow_setup(True, width, length, n, B, reps, version=2)
    cfg = 'meda %dx%d/%d' % (width, length, n)
    planner = MedaPlanner(width, length, n, device=DEV)
    for label, health in (('healthy', None), ('health [0.6, 1)', worn)):
        env.set_map('health', torch.ones_like(worn) if health is None else health)
        row = {'cfg': cfg, 'row': 'follow, ' + label, 'tasks': B}
        for mode, graph in (('eager', False), ('graph', True)):
            f = MedaFollower(env, use_graph=graph)
            run = lambda: (env.restart(), f.play(uniforms=draws, record=False))[1]
            row['ms_per_play_' + mode] = round(timed(run) * 1e3, 3)
        row.update(follow_quality(run()))
        row['failed_chips'] = int((env.get_state()['failed'] != 0).sum().item())
        h, u = (None, None) if health is None else (health.cpu().numpy(), draws.cpu().numpy())
        row['ms_per_follow_call'] = round(timed(lambda: planner.follow(s, g, health=h, uniforms=u)) * 1e3, 3)
        row['open_loop_success'] = round(float(planner.plan(s, g, health=h).success.mean()), 4)
        row['open_loop_safe_success'] = round(float(planner.plan(s, g, health=h, safe=True).success.mean()), 4)
        yield row


def meda_wide_follow_row(width, length, n, B, reps, ref_tasks, wide=True):
    """One row of the wide closed loop (or, `wide=False`, of the narrow follower on the same tasks and draws)."""
    from marl_dmfb_amd.plan import MedaFollower, MedaWideFollower, follow_reference_meda
    (s, g), env, draws, worn, timed = follow_setup(True, width, length, n, B, reps, version=2)
    Follower_ = MedaWideFollower if wide else MedaFollower
    row = {'cfg': 'meda %s%dx%d/%d' % ('wide ' if wide else '', width, length, n), 'row': 'follow, health [0.6, 1)', 'tasks': B}
    env.set_map('health', torch.ones_like(worn))
    f = Follower_(env, use_graph=True)
    run = lambda: (env.restart(), f.play(uniforms=draws, record=False))[1]
    row['ms_per_play_healthy_graph'] = round(timed(run) * 1e3, 3)
    row['healthy_success'] = round(float(run().success.float().mean()), 4)
    env.set_map('health', worn)
    for mode, graph in (('eager', False), ('graph', True)):
        f = Follower_(env, use_graph=graph)
        row['ms_per_play_' + mode] = round(timed(run) * 1e3, 3)
    res = run()
    row.update(follow_quality(res))
    row['failed_chips'] = int((env.get_state()['failed'] != 0).sum().item())
    row['replans_most'] = int(res.replans.max().item())
    if wide:
        from marl_dmfb_amd import _lib
        row.update({'lds_levels': _lib.meda_follow_wide().meda_follow_wide_lds_levels(width, length, n), 'levels': width + length - 2,
                    'workgroups': min(B, _lib.meda_follow_wide().meda_follow_wide_max_groups())})
    m = min(ref_tasks, B)
    if m:
        h, u = worn[:m].cpu().numpy(), draws[:, :m].cpu().numpy()
        t0 = time.perf_counter()
        ref = follow_reference_meda(width, length, s[:m], g[:m], health=h, uniforms=u)
        row['reference_s_per_task_one_core'] = round((time.perf_counter() - t0) / m, 3)
        row['equals_reference'] = all(np.array_equal(getattr(ref, k), getattr(res, k)[:m].cpu().numpy()) for k in FOLLOW_FIELDS)
    return row


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=5)
    p.add_argument('--tasks', type=int, default=4096)
    p.add_argument('--ref-tasks', type=int, default=64)
    p.add_argument('--meda', action='store_true')
    p.add_argument('--follow', action='store_true')
    p.add_argument('--wide', action='store_true', help='with --meda: the wide planner, chips up to 128 x 128')
    p.add_argument('--reserve', type=int, default=0, help='DMFB: levels over which unplanned droplets keep their start box')
    p.add_argument('--retries', default='0', help="DMFB: attempts after the n rotations; 'n' = the droplet count of the config")
    a, rest = p.parse_known_args()
    if a.meda and (a.reserve or a.retries != '0'):
        p.error('--reserve / --retries belong to the DMFB rule')
    if a.wide and not a.meda:
        p.error('--wide goes with --meda')
    if a.wide and a.follow:
        for (w, l, n), tasks, ref, wide in (((80, 80, 10), a.tasks, 8, True), ((128, 128, 16), min(a.tasks, 1024), 0, True),
                                            ((60, 60, 8), a.tasks, 8, True), ((60, 60, 8), a.tasks, 8, False)):
            print(json.dumps(meda_wide_follow_row(w, l, n, tasks, a.reps, min(a.ref_tasks, ref), wide)), flush=True)
        return
    if a.wide:
        for name, (w, l, n) in (('wide', (80, 80, 10)), ('wide', (128, 128, 16)), ('wide', (60, 60, 16)), ('meda', (60, 60, 16))):
            print(json.dumps(run(kinds()[name], w, l, n, a.tasks, a.reps, a.ref_tasks, {})), flush=True)
        return
    if a.follow and a.meda:
        for w, l, n in ((30, 30, 4), (30, 60, 8)):
            for row in meda_follow_rows(w, l, n, a.tasks, a.reps):
                print(json.dumps(row), flush=True)
        return
    if a.follow:
        for w, l, n in ((10, 10, 4), (20, 20, 10), (50, 50, 10)):
            for row in follow_rows(w, l, n, a.tasks, a.reps, rule_for(a, n)):
                print(json.dumps(row), flush=True)
        return
    kind = kinds()['meda' if a.meda else 'dmfb']
    for w, l, n in (((30, 30, 4), (30, 60, 8), (60, 60, 16)) if a.meda else ((10, 10, 4), (20, 20, 10), (50, 50, 10))):
        print(json.dumps(run(kind, w, l, n, a.tasks, a.reps, a.ref_tasks, rule_for(a, n))), flush=True)
    if a.meda:
        rows = meda_policy_table(a.tasks)
    else:
        rows = policy_table(['dmfb'] + rest, a.tasks) if '--model_dir' in rest else ()
    for row in rows:
        print(json.dumps(row), flush=True)

if __name__ == '__main__':
    main()
