"""No rollout, evaluation, route round or planner reads memory that nothing wrote: each scenario runs from identical seeds and
weights with clean allocations, with every torch.empty / torch.empty_like filled with pattern 'A' (NaN / 1 / True) and with pattern
'B' (-777.25 / 2 / False) (tests/poison_alloc.py), set-up included, and everything a caller can observe must come out with the same
bits: every tensor of the recorded episode batch, the four per-chip statistics, epsilon, `hidden` and `last_action` at the end;
for the continuous rollout the whole replay ring with ring_len / ring_stats / ring_state, what generate_steps returns and the
stage's chip_acc; for the planners every field of their results.  Control: two clean runs are bit-equal first (as
test_graph_rollout_equals_eager_rollout relies on).  Every poisoned run must have poisoned allocations of the scenario's own call
sites.  E = 48 chips (MEDA: 32).

Nothing is masked but route mode's `u`, by the docstring of common/rollout.py: Evaluator._play ("slots past a chip's episode are
not meaningful"; a chip that starts frozen plays no step): the mask is built from route_active and the clean run's `steps`.
Intermediate tensors (`actions` rows of frozen chips, `x_live` rows behind the live ones) are not compared.
profiles/poisoned_alloc/NOTES.md has the table of scenarios and what the tests found."""
import functools

import numpy as np
import pytest
import torch

import poison_alloc as PA
from vdn_helpers import det_init

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _host(v):
    return v.detach().cpu().clone() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))


def _three(label, run, sites, masks=None):
    """run(mode) -> ({name: tensor / array}, poison log or None).  masks(clean) -> {name: bool array, True = compared}."""
    clean, _ = run('clean')
    again, _ = run('clean')
    assert clean and list(clean) == list(again)
    control = ['%s: %s' % (k, PA.first_difference(clean[k], again[k])) for k in clean if not PA.bits_equal(clean[k], again[k])]
    assert not control, 'two clean runs of %s differ:\n%s' % (label, '\n'.join(control))
    keep = masks(clean) if masks is not None else {}
    for k, m in keep.items():
        assert m.shape == tuple(clean[k].shape) and m.mean() >= 0.5, 'mask of %s leaves %.2f of the tensor' % (k, m.mean())
    bad = []
    for mode in ('A', 'B'):
        got, log = run(mode)
        seen = {f: log.functions_seen(f, names) for f, names in sites.items()}
        print('poisoned %-44s pattern %s: %4d allocations (%4d in the package), sites %s' % (
            label, mode, log.count, log.package_count(), ' '.join(sorted(log.sites))))
        assert log.package_count() > 0 and seen == sites, 'the scenario did not allocate where it should: %r, wanted %r' % (seen, sites)
        assert list(got) == list(clean)
        for k in clean:
            x, y = clean[k], got[k]
            if k in keep:
                m = torch.as_tensor(keep[k])
                x, y = torch.where(m, x, torch.zeros_like(x)), torch.where(m, y, torch.zeros_like(y))
            d = PA.first_difference(x, y)
            if d:
                bad.append('%s pattern %s %s: %s' % (label, mode, k, d))
    assert not bad, '\n'.join(bad)


def _worker(name='dmfb', alg='vdn', fov=9, E=48, **over):
    """(env, args, agents, RolloutWorker) on DMFB 10x10 / 4 droplets or MEDA 30x30 / 4 droplets / fov 19, deterministic weights."""
    from marl_dmfb_amd.agent.agent import Agents
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.common.rollout import RolloutWorker
    if name == 'dmfb':
        from marl_dmfb_amd.env.dmfb import VecDMFB
        env = VecDMFB(10, 10, 4, fov=fov, n_envs=E, seed=11, device=DEV)
        kw = dict(drop_num=4, width=10, length=10, fov=fov)
    else:
        from marl_dmfb_amd.env.meda import VecMEDA
        env = VecMEDA(30, 30, 4, fov=19, n_envs=E, seed=11, device=DEV, version=2)
        kw = dict(name='meda', drop_num=4, width=30, length=30, fov=19)
    if alg == 'qmix':
        kw.update(state_shape=env.state_shape, **(dict(meda_state=True) if name == 'meda' else {}))
    kw = dict(dict(alg=alg, device=DEV, n_envs=E, buffer_size=E, anneal_steps=20000), **kw)
    kw.update(over)
    args = make_args(**kw, **env.get_env_info())
    torch.manual_seed(5)
    agents = Agents(args)
    det_init(agents.policy.eval_rnn, salt=0.25)
    return env, args, agents, RolloutWorker(env, agents, args)


def _keep_round_state(worker):
    """The `hidden` and `last_action` of the worker's latest round (updated in place by the fused lock-step tail)."""
    kept, real = [], worker._new_round

    def new_round(new=False):
        out = real(new)
        kept[:] = [out[1], out[2]]
        return out
    worker._new_round = new_round
    return kept


def _scattered_tasks(E, n=4):
    """Tasks of test_rollout_skipping_finished_chips_equals_the_full_batch_rollout: every droplet one cell from its goal or on it,
    so that under random actions chips finish at scattered times."""
    rng = torch.Generator().manual_seed(3)
    starts = torch.zeros((E, n, 2), dtype=torch.int32)
    starts[:, :, 0] = torch.tensor([1, 4, 7, 4])
    starts[:, :, 1] = torch.tensor([1, 4, 7, 8])
    ends = starts.clone()
    off = torch.randint(0, 3, (E, n), generator=rng)
    off[:, :3] *= (torch.rand(E, 1, generator=rng) < 0.2).long()
    ends[:, :, 0] += (off == 1).int()
    ends[:, :, 1] -= (off == 2).int()
    return starts, ends


# ------------------------------------------------------------------------------------------------ episodic _play(record=True)
# variant -> _worker arguments and switches.  fov5_forward_obs: fov 5 has a fused tail of its own by now, so the tail is switched
# off there (Evaluator.fuse_tail) to run the `forward_obs` lock-step.
VARIANTS = {'fov9_fused_tail': dict(),
            'fov9_live_compaction': dict(compact=True),
            'fov5_forward_obs': dict(fov=5, fuse_tail=False),
            'fov9_shield': dict(shield=True),
            'fov9_qmix_record_state': dict(alg='qmix'),
            'meda_fov19': dict(name='meda', E=32)}
EPISODIC = [(v, graph) for v in ('fov9_fused_tail', 'fov9_live_compaction', 'fov5_forward_obs') for graph in (False, True)] + \
           [(v, False) for v in ('fov9_shield', 'fov9_qmix_record_state', 'meda_fov19')]


def _variant_worker(variant, graph):
    v = dict(VARIANTS[variant])
    compact, fuse_tail, shield = v.pop('compact', False), v.pop('fuse_tail', True), v.pop('shield', False)
    env, args, agents, w = _worker(**v)
    w.use_graph, w.fuse_tail = graph, fuse_tail
    if shield:
        w.shield = True
        w._shield_state()
    if compact:
        env.set_task(*_scattered_tasks(env.n_envs))
        w.reset_fn, w.compact_every, w.live_share = env.restart, 2, 0.5
        w.epsilon = torch.tensor(1.0, device=DEV)
        assert w._skip_finished() and agents.policy.eval_rnn._hip_geometry() == 9
    return env, args, agents, w


@pytest.mark.parametrize('variant,graph', EPISODIC, ids=['%s-%s' % (v, 'graph' if g else 'eager') for v, g in EPISODIC])
def test_recorded_episodes_read_no_unwritten_memory(variant, graph):
    def run(mode):
        with PA.run_mode(mode) as log:
            env, args, agents, w = _variant_worker(variant, graph)
            kept = _keep_round_state(w)
            out = {}
            for rnd in range(2):
                res = w.generate_episode()
                for k, name in enumerate(('reward', 'steps', 'constraints', 'success')):
                    out['round%d/%s' % (rnd, name)] = _host(res[k])
                for key, val in res[4].items():
                    out['round%d/ep/%s' % (rnd, key)] = _host(val)
                out['round%d/epsilon' % rnd] = _host(w.epsilon)
                out['round%d/hidden' % rnd], out['round%d/last_action' % rnd] = _host(kept[0]), _host(kept[1])
            if variant == 'fov9_shield':
                out['shield_overrides'], out['shield_unsafe'] = _host(w.shield_overrides), _host(w.shield_unsafe)
            if variant == 'fov9_qmix_record_state':
                assert 'round1/ep/s' in out and 'round1/ep/s_next' in out
            if variant == 'fov9_live_compaction':
                lengths = (~res[4]['padded'][:, :, 0]).sum(1)
                assert float((lengths < args.episode_limit).float().mean()) > 0.3 and len(torch.unique(lengths)) > 3
        return out, log
    front = {'fov5_forward_obs': '_fov_front_forward'}.get(variant, '_front_features_hip')
    sites = {'common/rollout.py': {'_play'}}
    if variant != 'fov9_live_compaction':      # the live list runs CRNN.front_features_live on the caller's x_live
        sites['network/base_net.py'] = {front}
    print()
    _three('episodic %s %s' % (variant, 'graph' if graph else 'eager'), run, sites)


# ----------------------------------------------------------------------------------------------------------- greedy evaluation
@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_greedy_evaluation_reads_no_unwritten_memory(graph):
    def run(mode):
        with PA.run_mode(mode) as log:
            env, args, agents, w = _worker()
            w.use_graph = graph
            kept = _keep_round_state(w)
            out = {}
            for rnd in range(2):
                res = w._generate_episode()
                for k, name in enumerate(('reward', 'steps', 'constraints', 'success')):
                    out['round%d/%s' % (rnd, name)] = _host(res[k])
                out['round%d/hidden' % rnd], out['round%d/last_action' % rnd] = _host(kept[0]), _host(kept[1])
        return out, log
    print()
    _three('greedy evaluation %s' % ('graph' if graph else 'eager'), run,
           {'common/rollout.py': {'_play'}, 'network/base_net.py': {'_front_features_hip'}})


# ---------------------------------------------------------------------------------------------------------- continuous rollout
STREAMS = {'vdn_dmfb': (dict(), False), 'vdn_dmfb_graph': (dict(), True),
           'qmix_dmfb_stream_state': (dict(alg='qmix', stream_state=True), False),
           'qmix_meda_meda_state': (dict(name='meda', alg='qmix', stream_state=True, E=32), False)}


@pytest.mark.parametrize('case', list(STREAMS))
def test_continuous_rollout_reads_no_unwritten_memory(case):
    """1.5 episode limits of lock-steps in calls of half a limit (graph: the first call is the warm-up and the capture, the other
    two replay) or three quarters of one, so episodes close, restart and straddle the calls.  The ring has as many slots as there
    are chips: every chip closes an episode within one limit, so every slot has been written when the ring is compared."""
    over, graph = STREAMS[case]

    def run(mode):
        from marl_dmfb_amd.common.replay_buffer import ReplayBuffer
        with PA.run_mode(mode) as log:
            env, args, agents, w = _worker(**over)
            buf = ReplayBuffer(args, device=DEV)
            assert w.stream_ok() and buf.size == env.n_envs
            w.use_graph = graph
            T = args.episode_limit
            out = {}
            for call, K in enumerate([T // 2] * 3 if graph else [3 * T // 4] * 2):
                out['call%d/returned' % call] = _host(w.generate_steps(buf, K))
                out['call%d/epsilon' % call] = _host(w.epsilon)
            st = w._stream_state(buf)
            assert int(buf.ring_len.min()) > 0, 'a slot of the ring was never written'
            for k, v in buf.buffers.items():
                out['ring/' + k] = _host(v)
            if buf.states is not None:
                out['ring/states'] = _host(buf.states)
            for k in ('ring_len', 'ring_stats', 'ring_state'):
                out[k] = _host(getattr(buf, k))
            for k in ('chip_acc', 'ep_acc', 'hidden', 'last_action', 't_ep', 'eps'):
                out['stage/' + k] = _host(getattr(st, k))
        return out, log
    print()
    _three('continuous %s' % case, run, {'common/replay_buffer.py': {'__init__'}, 'network/base_net.py': {'_front_features_hip'}})


def test_poison_reaches_the_device_and_a_closed_slot_is_written_whole():
    """The other direction: memory that really is never written must show.  A ring of 2 E slots after one episode limit of
    lock-steps has slots no episode was closed into (ring_len 0 = never written, common/replay_buffer.py).  Under either pattern
    those slots hold the pattern in every replay tensor -- so a read of them could not have gone unnoticed above -- while every
    slot an episode was closed into is the same under both patterns, padding included."""
    from marl_dmfb_amd.common.replay_buffer import ReplayBuffer
    rings = {}
    for mode in ('A', 'B'):
        with PA.poisoned(mode):
            env, args, agents, w = _worker(buffer_size=96)
            buf = ReplayBuffer(args, device=DEV)
            w.generate_steps(buf, args.episode_limit)
            rings[mode] = (buf.ring_len.cpu().numpy().copy(), {k: _host(v) for k, v in buf.buffers.items()})
    (len_a, ring_a), (len_b, ring_b) = rings['A'], rings['B']
    assert np.array_equal(len_a, len_b)
    written = len_a > 0
    assert written.sum() >= 48 and (~written).sum() >= 8, (written.sum(), len(written))
    for k in ring_a:
        a, b = ring_a[k].numpy(), ring_b[k].numpy()
        assert a[written].tobytes() == b[written].tobytes(), 'a closed slot of %s depends on what the memory held before' % k
        fa, fb = PA.fill_value('A', ring_a[k].dtype), PA.fill_value('B', ring_a[k].dtype)
        assert (np.isnan(a[~written]) if ring_a[k].dtype.is_floating_point else a[~written] == fa).all(), k
        assert (b[~written] == fb).all(), k


# ---------------------------------------------------------------------------------------------------------- env introspection
@pytest.mark.parametrize('name', ['dmfb', 'meda'])
def test_env_step_and_introspection_read_no_unwritten_memory(name):
    """The env facade on its own, on chips that degrade: twelve lock-steps of seeded actions with a reset of the finished chips,
    then every tensor of get_state and the three maps of get_map (each an `empty` buffer that one kernel must fill)."""
    E, A = (48, 5) if name == 'dmfb' else (32, 9)
    acts = np.random.default_rng(4).integers(0, A, (12, E, 4)).astype(np.int32)

    def run(mode):
        with PA.run_mode(mode) as log:
            if name == 'dmfb':
                from marl_dmfb_amd.env.dmfb import VecDMFB
                env = VecDMFB(10, 10, 4, fov=9, n_envs=E, seed=11, device=DEV, b_degrade=True, per_degrade=0.5)
            else:
                from marl_dmfb_amd.env.meda import VecMEDA
                env = VecMEDA(30, 30, 4, fov=19, n_envs=E, seed=11, device=DEV, version=2, b_degrade=True, per_degrade=0.5)
            out = {'obs0': _host(env.reset())}
            for t in range(12):
                obs, r, d, info = env.step(torch.as_tensor(acts[t], device=DEV), autoreset=True)
                out['step%d/obs' % t], out['step%d/r' % t], out['step%d/done' % t] = _host(obs), _host(r), _host(d)
                for k, v in info.items():
                    if isinstance(v, torch.Tensor):
                        out['step%d/%s' % (t, k)] = _host(v)
            out.update({'state/' + k: _host(v) for k, v in env.get_state().items()})
            out.update({'map/' + k: _host(env.get_map(k)) for k in ('health', 'usage', 'degrade')})
            s, g = env.get_task()
            out['task/starts'], out['task/goals'] = _host(s), _host(g)
        return out, log
    print()
    _three('env %s' % name, run, {'env/_vec.py': {'get_map', 'get_task'}, 'env/%s.py' % name: {'get_state'}})


# ------------------------------------------------------------------------------------------------------------------ route mode
def test_route_round_with_frozen_chips_reads_no_unwritten_memory():
    """Evaluator._play(route=True), a quarter of the chips frozen from the start through route_active, epsilon 0.5 (most chips play
    to the limit, so `u` stays meaningful in most slots)."""
    E = 48
    frozen = np.arange(E) % 4 == 0

    def run(mode):
        with PA.run_mode(mode) as log:
            env, args, agents, w = _worker()
            env.reset()
            s, g = env.get_task()
            env.set_task(s, g)
            w.reset_fn = env.restart
            w.route_active = torch.as_tensor(~frozen, device=DEV).to(torch.uint8)
            agents.policy.init_hidden(1)
            res = w._play(torch.tensor(0.5, device=DEV), evaluate=False, record=False, route=True)
            out = {name: _host(res[k]) for k, name in enumerate(('reward', 'steps', 'constraints', 'success'))}
            out.update({'ep/' + k: _host(v) for k, v in res[4].items()})
            out['epsilon'] = _host(res[5])
        return out, log

    def masks(clean):
        # common/rollout.py: Evaluator._play: "'u': int8 (E, T, n, 1) actions (slots past a chip's episode are not meaningful)";
        # a chip whose route_active byte is 0 starts frozen and plays no step
        steps = clean['ep/steps'].numpy()
        assert (steps[frozen] == 0).all() and (steps[~frozen] > 0).all()
        T = clean['ep/u'].shape[1]
        played = (np.arange(T)[None, :] < steps[:, None]) & ~frozen[:, None]
        return {'ep/u': np.broadcast_to(played[:, :, None, None], tuple(clean['ep/u'].shape)).copy()}
    print()
    _three('route round, frozen chips', run, {'common/rollout.py': {'_play'}, 'network/base_net.py': {'_front_features_hip'}}, masks)


@functools.lru_cache(maxsize=None)
def _dmfb_tasks(B, n_blocks=0, seed=21):
    from plan_helpers import oracle_tasks
    return oracle_tasks(10, 10, 4, n_blocks, seed, B=B)


@pytest.mark.parametrize('tries', [1, 3])
def test_router_reads_no_unwritten_memory(tries):
    """Router.route: tries 1 is one greedy round, tries 3 adds two epsilon rounds and the best-of-K pick (rollout_route_select into
    `empty` outputs).  RouteResult.actions is -1 past a task's episode, so nothing is masked."""
    s, g, _ = _dmfb_tasks(48)

    def run(mode):
        from marl_dmfb_amd.route import Router
        with PA.run_mode(mode) as log:
            env, args, agents, w = _worker(E=4)
            router = Router(agents, name='dmfb', width=10, length=10, n_agents=4, fov=9, device=DEV)
            out = {}
            for call in range(2):       # the second call replays the handle's captured graphs
                r = router.route(s, g, tries=tries, epsilon=0.3, seed=3)
                for k in ('positions', 'actions', 'steps', 'success', 'constraints', 'try_index'):
                    out['call%d/%s' % (call, k)] = _host(getattr(r, k))
        return out, log
    sites = {'common/rollout.py': {'_play'}}
    if tries > 1:
        sites['route.py'] = {'route'}
    print()
    _three('router tries=%d' % tries, run, sites)


# -------------------------------------------------------------------------------------------------------------------- planners
PLAN_FIELDS = ('positions', 'actions', 'steps', 'success', 'constraints', 'attempt', 'lower_bound')
FOLLOW_FIELDS = ('positions', 'actions', 'steps', 'success', 'constraints', 'replans', 'gave_up', 'lower_bound', 'reward')


@functools.lru_cache(maxsize=None)
def _planner_inputs(kind):
    """Tasks the planners' own GPU tests use, a handful of them: -> (planner factory, call(planner, slice) -> result, fields,
    the two batch sizes)."""
    from marl_dmfb_amd import plan
    if kind == 'dmfb_plan':
        s, g, b = _dmfb_tasks(10, 2, 2)
        return (lambda: plan.Planner(10, 10, 4, device=DEV)), (lambda p, k: p.plan(s[k], g[k], blocks=b[k])), PLAN_FIELDS, (6, 4)
    if kind in ('dmfb_follow', 'dmfb_follow_seeded'):      # seeded: the move draws from a torch.Generator into an `empty` tensor
        import follow_helpers
        c, s, g, b, health, uniforms = follow_helpers.case('10x10_4_2b')
        draws = (lambda k: dict(seed=5)) if kind.endswith('seeded') else (lambda k: dict(uniforms=uniforms[:, k]))
        return ((lambda: plan.Planner(10, 10, 4, device=DEV)),
                (lambda p, k: p.follow(s[k], g[k], blocks=b[k], health=health[k], **draws(k))), FOLLOW_FIELDS, (6, 4))
    if kind in ('meda_plan', 'meda_plan_safe'):
        import meda_plan_helpers
        s, g = meda_plan_helpers.oracle_tasks(30, 30, 4, seed=1, B=10)
        return ((lambda: plan.MedaPlanner(30, 30, 4, device=DEV)), (lambda p, k: p.plan(s[k], g[k], safe=kind.endswith('safe'))),
                PLAN_FIELDS, (6, 4))
    if kind == 'meda_follow':
        import meda_follow_helpers
        c, s, g, health, uniforms = meda_follow_helpers.case('30x30_4')
        return ((lambda: plan.MedaPlanner(30, 30, 4, device=DEV)),
                (lambda p, k: p.follow(s[k], g[k], health=health[k], uniforms=uniforms[:, k])), FOLLOW_FIELDS, (6, 4))
    if kind == 'meda_wide_plan':        # lds_levels 8: most levels of every plan live in the `empty` workspace
        import meda_plan_wide_helpers
        c = meda_plan_wide_helpers.set_case('20x100_4')
        s, g = c['starts'], c['goals']
        return ((lambda: plan.MedaWidePlanner(20, 100, 4, device=DEV, lds_levels=8)), (lambda p, k: p.plan(s[k], g[k])), PLAN_FIELDS, (6, 4))
    if kind == 'meda_wide_follow':
        import meda_follow_wide_helpers
        c, s, g, health, uniforms = meda_follow_wide_helpers.case('20x72_3')
        return ((lambda: plan.MedaWideFollowPlanner(20, 72, 3, device=DEV, lds_levels=8)),
                (lambda p, k: p.follow(s[k], g[k], health=health[k], uniforms=uniforms[:, k])), FOLLOW_FIELDS, (4, 2))
    raise KeyError(kind)


PLANNER_SITES = {'dmfb_plan': {'_plan'}, 'dmfb_follow': set(), 'dmfb_follow_seeded': {'_follow'}, 'meda_plan': {'_plan'}, 'meda_plan_safe': {'_plan'}, 'meda_follow': set(),
                 'meda_wide_plan': {'_plan', '_launch'}, 'meda_wide_follow': {'MedaWideFollower'}}


@pytest.mark.parametrize('kind', list(PLANNER_SITES))
def test_planners_read_no_unwritten_memory(kind):
    """One planner object, three calls: B tasks, then another batch size, then the first B tasks again -- on the buffers the object
    keeps per batch size (the wide planners' byte workspaces, the followers' env handles) after other work has dirtied them.  The
    third call must also repeat the first."""
    make, call, fields, (B1, B2) = _planner_inputs(kind)

    def run(mode):
        with PA.run_mode(mode) as log:
            planner = make()
            out = {}
            for j, k in enumerate((slice(0, B1), slice(B1, B1 + B2), slice(0, B1))):
                res = call(planner, k)
                for f in fields:
                    out['call%d/%s' % (j, f)] = _host(getattr(res, f))
            for f in fields:
                assert PA.bits_equal(out['call0/' + f], out['call2/' + f]), 'the third call does not repeat the first: %s' % f
        return out, log
    print()
    _three('planner %s' % kind, run, {'plan.py': PLANNER_SITES[kind]} if PLANNER_SITES[kind] else {})
