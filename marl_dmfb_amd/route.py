"""Route GIVEN tasks with a trained policy and get every droplet's path back (the reference's evaluate.py shows the routes of
random tasks one chip at a time; here a batch of caller-given tasks is played in lock-step on the GPU).

    router = Router(agents, name='dmfb', width=20, length=20, n_agents=4, fov=9)
    res = router.route(starts, goals, blocks=None, health=None, tries=8, epsilon=0.1, seed=0)

Every task is played `tries` times side by side, task-major (chip = task * tries + try): try 0 greedily (epsilon 0, the route
`Evaluator` plays for the same injected task), tries 1 .. K-1 epsilon-greedy with the rollout's Philox stream, whose counter
range `seed` selects.
The best try of each task is picked and its rows gathered on the device (include/rollout_route.h: rollout_route_select): a
successful try beats a failed one, then fewer steps, then fewer constraints, then the lower try index.

A round is `Evaluator._play(..., route=True)`: the actions and, after the restart and after every lock-step, the droplet
positions of every chip are recorded on the device (include/dmfb_vec.h: dmfb_vec_route_append, include/meda_vec.h).  With
K > 1 the greedy tries and the epsilon tries play in two rounds over the same handle, the other tries frozen.

A round is replayed from a captured HIP graph, which holds every kernel argument as it was at capture.  So nothing that differs
between calls travels as a kernel argument: the Philox key of the epsilon-greedy picks is one fixed constant, and `seed` (with
the chunk and the round) sets the START of the device-side draw counter (Evaluator._draw, one step per lock-step), so that two
seeds read disjoint counter ranges of the same Philox stream; and a handle (with its graphs) serves exactly one count of
obstacle blocks, which the env's kernels take by value.  Moves can fail only on degraded electrodes (a `health` map below 1);
their draws then come from a device buffer filled from `seed` before each round.  The same inputs and seed therefore give the
same routes on every call, in eager mode and under graph replay alike.

`fallback='plan'` (off by default) hands the tasks whose kept try failed to the deterministic space-time planner
(marl_dmfb_amd.plan) and takes its route where it finds one; `lower_bound=True` asks only for the planner's lower bound on the
steps of every task.  A DMFB router builds its own `Planner` unless one is given through `planner=` (say
`plan.Planner(width, length, n_agents, reserve=1)`, for its rule with reservations); a MEDA router takes one through `planner=` (a
`plan.MedaPlanner` of the router's width, length and droplet count, or any object with such a `plan` method) and refuses the two
options without it.  Without either option, every returned array is what the policy alone gives.

`fallback='follow'` plays the tasks whose kept try failed closed-loop instead (marl_dmfb_amd.plan.Follower: plan, step,
replan where a move failed) under the same `health`, avoiding the cells below `min_health`, and takes its episode where it
brought every droplet home (`source` 2).  That is the fallback for worn chips, where the open-loop planner forbids every
electrode below 1.0 and routes nothing.  A DMFB router builds its own `Planner` or uses the given one, whose `reserve` /
`retries` then hold in every replan; a MEDA router takes a `plan.MedaPlanner` (chips up to 64 x 64), a
`plan.MedaWideFollowPlanner` (up to 128 x 128) or any object with such a `follow` method through `planner=` and refuses the
option without it."""
import numpy as np
import torch

from . import _lib

MAX_CHIPS = 32768   # the largest handle a Router creates unless told otherwise (ROLLOUT_STREAM_MAX_ENVS)
_MASK64 = 0xFFFFFFFFFFFFFFFF
ROUTE_KEY = 0x726F7574652D6B31   # the Philox key of every Router's epsilon-greedy picks (seed selects the counter range)


def _mix64(x):
    """splitmix64 finaliser: a well-spread 64-bit value of x."""
    x = (x + 0x9E3779B97F4A7C15) & _MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK64
    return x ^ (x >> 31)


def round_stream(seed, chunk, rnd):
    """(first draw counter, uint32; generator seed of the move draws) of round `rnd` (0 greedy, 1 epsilon) of chunk `chunk`."""
    h = _mix64(_mix64(_mix64(int(seed) & _MASK64) ^ int(chunk)) ^ int(rnd))
    return h & 0xFFFFFFFF, (h >> 1) & 0x7FFFFFFFFFFFFFFF


class RouteResult:
    """positions uint8 (B, T+1, n, 2): (x, y) per droplet after the restart (slot 0) and after every lock-step, the last position
    repeated after the episode ended; actions int8 (B, T, n), -1 after the episode ended; steps int64 (B,) steps played;
    success bool (B,); constraints (B,) (int64 for DMFB, float64 for MEDA); try_index int32 (B,): the try that was kept, -1 for
    a route of the planner or the follower; source int8 (B,): 0 policy, 1 planner, 2 closed-loop follower; lower_bound int32 (B,): the planner's lower bound on the steps
    (-1: some goal is out of reach), None unless a fallback or the bound was asked for; overrides int32 (B,): the picks the
    shield replaced in the kept try (0 for a route of the planner or the follower), None unless the router shields."""

    def __init__(self, positions, actions, steps, success, constraints, try_index, source=None, lower_bound=None,
                 overrides=None):
        self.positions, self.actions, self.steps = positions, actions, steps
        self.success, self.constraints, self.try_index = success, constraints, try_index
        self.source = np.zeros(len(steps), np.int8) if source is None else source
        self.lower_bound = lower_bound
        self.overrides = overrides

    def __len__(self):
        return len(self.steps)


def _fail(b, msg):
    raise ValueError('task %d: %s' % (b, msg))


def validate_tasks(name, width, length, n_agents, starts, goals, blocks=None, health=None, max_blocks=None):
    """Host-side checks before anything is launched; returns (starts, goals, blocks, health) as contiguous numpy arrays.
    Raises ValueError naming the first bad task.  DMFB positions are (x, y) with x < width, y < length; MEDA centres are
    (x_center, y_center) with x < length, y < width (the order of meda_vec_get_map), at least 2 from every edge."""
    starts = np.asarray(starts)
    goals = np.asarray(goals)
    if starts.ndim != 3 or starts.shape[1:] != (n_agents, 2):
        raise ValueError('starts must have shape (B, %d, 2), got %s' % (n_agents, starts.shape))
    if goals.shape != starts.shape:
        raise ValueError('goals must have the shape of starts %s, got %s' % (starts.shape, goals.shape))
    if not (np.issubdtype(starts.dtype, np.integer) and np.issubdtype(goals.dtype, np.integer)):
        raise ValueError('starts and goals must be integer arrays')
    B = starts.shape[0]
    if name == 'dmfb':
        lo, hi = np.array([0, 0]), np.array([width - 1, length - 1])
    else:
        lo, hi = np.array([2, 2]), np.array([length - 3, width - 3])
    if blocks is not None:
        if name != 'dmfb':
            raise ValueError('blocks are a DMFB feature')
        blocks = np.asarray(blocks)
        if blocks.ndim != 3 or blocks.shape[0] != B or blocks.shape[2] != 4 or not np.issubdtype(blocks.dtype, np.integer):
            raise ValueError('blocks must be an integer array of shape (B=%d, nb, 4), got %s' % (B, blocks.shape))
        if max_blocks is not None and blocks.shape[1] > max_blocks:
            raise ValueError('%d blocks per task, the router takes at most %d' % (blocks.shape[1], max_blocks))
    if health is not None:
        health = np.asarray(health, dtype=np.float64)
        if health.shape != (B, width, length):
            raise ValueError('health must have shape (B=%d, %d, %d), got %s' % (B, width, length, health.shape))
    for b in range(B):
        for what, pts in (('start', starts[b]), ('goal', goals[b])):
            bad = np.nonzero(np.any((pts < lo) | (pts > hi), axis=1))[0]
            if len(bad):
                edge = '' if name == 'dmfb' else ' (a MEDA centre keeps its 5x5 box on the chip)'
                _fail(b, '%s of droplet %d at %s is off the chip%s' % (what, bad[0], tuple(int(v) for v in pts[bad[0]]), edge))
            if len({tuple(p) for p in pts.tolist()}) != len(pts):
                _fail(b, 'two %ss on the same cell' % what)
        if blocks is not None:
            for k, (x0, x1, y0, y1) in enumerate(blocks[b].tolist()):
                if x0 > x1 or y0 > y1 or x0 < 0 or y0 < 0 or x1 >= width or y1 >= length:
                    _fail(b, 'block %d %s is not a box on the chip' % (k, (x0, x1, y0, y1)))
                for what, pts in (('start', starts[b]), ('goal', goals[b])):
                    inside = (pts[:, 0] >= x0) & (pts[:, 0] <= x1) & (pts[:, 1] >= y0) & (pts[:, 1] <= y1)
                    if inside.any():
                        _fail(b, '%s of droplet %d lies inside block %d' % (what, int(np.argmax(inside)), k))
    if health is not None and not np.all(np.isfinite(health)):
        _fail(int(np.argmax(~np.isfinite(health).reshape(B, -1).all(axis=1))), 'health is not finite')
    cont = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
    return cont(starts, np.int32), cont(goals, np.int32), cont(blocks, np.int32), cont(health, np.float64)


def select_reference(steps, success, constraints, tries):
    """The rule of rollout_route_select in numpy (tests and documentation): chosen try per task of a task-major batch."""
    steps = np.asarray(steps).reshape(-1, tries)
    success = (np.asarray(success).reshape(-1, tries) > 0)
    cons = np.asarray(constraints, dtype=np.float64).reshape(-1, tries)
    out = np.empty(steps.shape[0], np.int32)
    for b in range(steps.shape[0]):
        out[b] = min(range(tries), key=lambda k: (not success[b, k], steps[b, k], cons[b, k], k))
    return out


class Router:
    """Plays given tasks with the agent network of `agents` (VDN or QMIX: the mixer plays no part in acting) on handles of at most
    `max_chips` chips; larger batches are routed in chunks.  name 'dmfb' / 'meda'; n_blocks: the most obstacle blocks a DMFB task
    may carry (0 = no limit of the router's own); version: MEDA observation version ('0.2' or 2 = v0_2, anything else v0), as the
    training flags.  One handle (and its captured graphs) is kept per (chips, blocks per task, health given).
    shield (DMFB only, off by default): every try, greedy and epsilon alike, plays under the action shield (marl_dmfb_amd.shield),
    so a route that starts conflict-free has constraints 0; RouteResult.overrides counts the picks it replaced.
    meda_shield (MEDA only, off by default): the same under the MEDA rule (meda_shield_reference): a route whose starts are pairwise
    6 apart has constraints 0 and so is never `failed`."""

    def __init__(self, agents, name='dmfb', width=20, length=20, n_agents=4, fov=9, n_blocks=0, stall=True, version=None,
                 max_chips=MAX_CHIPS, use_graph=True, device=None, shield=False, meda_shield=False):
        if name not in ('dmfb', 'meda'):
            raise ValueError("name must be 'dmfb' or 'meda'")
        if shield and name != 'dmfb':
            raise ValueError('shield: the action shield is a DMFB feature (a MEDA droplet inside its goal disc is snapped '
                             'whatever its action, which needs a rule of its own)')
        if meda_shield and name != 'meda':
            raise ValueError('meda_shield: the MEDA action shield is a MEDA feature (the DMFB switch is shield)')
        self.shield, self.meda_shield = bool(shield), bool(meda_shield)
        self.shielded = self.shield or self.meda_shield
        self.agents, self.name = agents, name
        self.width, self.length, self.n_agents, self.fov = int(width), int(length), int(n_agents), int(fov)
        self.n_blocks, self.stall = int(n_blocks), bool(stall)
        self.version = 2 if str(version) in ('0.2', '2') else 0
        self.max_chips = int(max_chips)
        self.use_graph = bool(use_graph)
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.episode_limit = 2 * (self.width + self.length) if name == 'dmfb' else self.width + self.length
        self._slots = {}   # (chips, blocks per task, maps) -> handle, Evaluator, draw buffer
        self._planner = None
        self.rounds = 0    # rounds played so far (tests: tries=1 is one round per chunk)

    # ------------------------------------------------------------------ handles
    def _slot(self, E, nb, maps):
        key = (E, nb, maps)
        s = self._slots.get(key)
        if s is None:
            from .common.rollout import Evaluator
            if self.name == 'dmfb':
                from .env.dmfb import VecDMFB
                env = VecDMFB(self.width, self.length, self.n_agents, nb, fov=self.fov, stall=self.stall, n_envs=E, seed=0,
                              with_maps=maps, device=self.device)
            else:
                from .env.meda import VecMEDA
                env = VecMEDA(self.width, self.length, self.n_agents, fov=self.fov, n_envs=E, seed=0, with_maps=maps,
                              device=self.device, version=self.version)
            ev = Evaluator(env, self.agents, env.max_step)
            ev.use_graph = self.use_graph
            ev.shield, ev.meda_shield = self.shield, self.meda_shield
            ev.reset_fn = env.restart
            ev.rng_seed = ROUTE_KEY   # fixed for the handle's life: a captured graph holds it
            ev.route_active = torch.ones(E, dtype=torch.uint8, device=self.device)
            draws = None
            if maps:   # move draws of the degraded electrodes, refilled from the seed before every round
                draws = torch.zeros((env.max_step, E, self.n_agents), dtype=torch.float64, device=self.device)
                ev.uniforms_fn = lambda t, d=draws: d[t]
            s = {'env': env, 'ev': ev, 'draws': draws}
            self._slots[key] = s
        return s

    def _round(self, s, greedy, epsilon, active, stream):
        ev = s['ev']
        ev.route_active.copy_(active)
        ev._ops()
        # the share of live chips decides whether the Q-network walks the list of live chips (Evaluator._skip_finished)
        ev.live_share = float(active.sum().item()) / float(max(1, active.numel()))
        self.agents.policy.init_hidden(1)
        eps = 0.0 if greedy else float(epsilon)
        if ev.use_graph and ev.graph_key(greedy, False, route=True) not in ev._graphs:
            ev._play_graphed(eps, evaluate=greedy, record=False, route=True)   # warm-up and capture: their draws are not kept
        first_draw, gen_seed = stream
        # the round's epsilon-greedy draws start at this counter (uint32 on the device, stored through its int32 view)
        ev._draw.fill_(first_draw - (1 << 32) if first_draw >= (1 << 31) else first_draw)
        ev._n_alive.zero_()
        if s['draws'] is not None:
            g = torch.Generator(device=self.device)
            g.manual_seed(gen_seed)
            s['draws'].uniform_(0.0, 1.0, generator=g)
        play = ev._play_graphed if ev.use_graph else ev._play
        _, _, constraints, success, ep, _ = play(eps, evaluate=greedy, record=False, route=True)
        self.rounds += 1
        over = ev.shield_overrides.clone() if self.shielded else None
        return ep['steps'].clone(), success.clone(), constraints.clone(), ep['route'].clone(), ep['u'].clone(), over

    # ------------------------------------------------------------------ routing
    def _plan(self, res, starts, goals, blocks, health, substitute, planner=None):
        """The planner's lower bound for every task and, with `substitute`, its route for the tasks the policy failed."""
        if planner is not None:
            plan = planner.plan(starts, goals, health=health) if blocks is None else planner.plan(starts, goals, blocks=blocks,
                                                                                                  health=health)
        else:
            if self._planner is None:
                from .plan import Planner
                self._planner = Planner(self.width, self.length, self.n_agents, device=self.device)
            plan = self._planner.plan(starts, goals, blocks=blocks, health=health)
        res.lower_bound = plan.lower_bound
        take = (~res.success) & plan.success if substitute else np.zeros(len(res), bool)
        for k in ('positions', 'actions', 'steps', 'success', 'constraints'):
            getattr(res, k)[take] = getattr(plan, k)[take]
        res.try_index[take] = -1
        res.source[take] = 1
        if res.overrides is not None:
            res.overrides[take] = 0
        return res

    def _follow(self, res, starts, goals, blocks, health, min_health, seed, planner=None):
        """The tasks the policy failed, played closed-loop under the same health (plan.Planner.follow, or the `follow` of the
        planner a MEDA router was given): its episodes replace theirs where it brought every droplet home."""
        failed = np.nonzero(~res.success)[0]
        if len(failed) == 0:
            return res
        sub = lambda a: None if a is None else a[failed]
        gen_seed = round_stream(seed, 0, 2)[1]
        if planner is not None and self.name != 'dmfb':
            fol = planner.follow(starts[failed], goals[failed], health=sub(health), min_health=min_health, seed=gen_seed)
        else:
            if planner is None and self._planner is None:
                from .plan import Planner
                self._planner = Planner(self.width, self.length, self.n_agents, device=self.device)
            # a given DMFB planner brings its own rule (reserve, retries) to the follower it builds
            fol = (planner or self._planner).follow(starts[failed], goals[failed], blocks=sub(blocks), health=sub(health),
                                                    min_health=min_health, seed=gen_seed, stall=self.stall)
        take = failed[fol.success]
        for k in ('positions', 'actions', 'steps', 'success', 'constraints'):
            getattr(res, k)[take] = getattr(fol, k)[fol.success]
        res.try_index[take] = -1
        res.source[take] = 2
        if res.overrides is not None:
            res.overrides[take] = 0
        return res

    def route(self, starts, goals, blocks=None, health=None, tries=1, epsilon=0.1, seed=0, fallback=None, lower_bound=False,
              planner=None, min_health=0.0):
        if fallback not in (None, 'plan', 'follow'):
            raise ValueError("fallback must be None, 'plan' or 'follow', got %r" % (fallback,))
        if fallback == 'follow' and self.name != 'dmfb' and planner is None:
            raise ValueError('the closed-loop follower (fallback) routes DMFB only, unless a planner with a follow method is given')
        planned = fallback == 'plan' or bool(lower_bound)
        if planner is not None:
            if (planned or fallback != 'follow') and not callable(getattr(planner, 'plan', None)):
                raise ValueError('planner must have a plan(starts, goals, ...) method that returns a PlanResult')
            if fallback == 'follow' and not callable(getattr(planner, 'follow', None)):
                raise ValueError('planner must have a follow(starts, goals, ...) method that returns a FollowResult')
            theirs = tuple(getattr(planner, k, None) for k in ('width', 'length', 'n_agents'))
            if theirs != (self.width, self.length, self.n_agents):
                raise ValueError('planner is for width, length, droplets = %s, the router for %s'
                                 % (theirs, (self.width, self.length, self.n_agents)))
        elif planned and self.name != 'dmfb':
            raise ValueError('the planner (fallback, lower_bound) routes DMFB only')
        tries = int(tries)
        if tries < 1:
            raise ValueError('tries must be >= 1')
        if tries > self.max_chips:
            raise ValueError('tries (%d) larger than max_chips (%d)' % (tries, self.max_chips))
        starts, goals, blocks, health = validate_tasks(self.name, self.width, self.length, self.n_agents, starts, goals,
                                                       blocks, health, max_blocks=self.n_blocks or None)
        B, n, K, T = starts.shape[0], self.n_agents, tries, self.episode_limit
        if B == 0:
            return RouteResult(np.zeros((0, T + 1, n, 2), np.uint8), np.zeros((0, T, n), np.int8), np.zeros(0, np.int64),
                               np.zeros(0, bool), np.zeros(0, np.int64 if self.name == 'dmfb' else np.float64),
                               np.zeros(0, np.int32), lower_bound=np.zeros(0, np.int32) if planned else None,
                               overrides=np.zeros(0, np.int32) if self.shielded else None)
        nb = 0 if blocks is None else blocks.shape[1]
        per = max(1, self.max_chips // K)          # tasks per chunk
        Bc = min(B, per)
        E = Bc * K
        # the env's kernels take the count of blocks in force by value, so a captured graph holds it: one handle per count
        s = self._slot(E, nb, health is not None)
        env, dev = s['env'], self.device
        first = torch.zeros(E, dtype=torch.uint8, device=dev)
        first[::K] = 1
        lib = _lib.checked('rollout_route')
        stream = torch.cuda.current_stream(dev).cuda_stream
        out = {k: [] for k in ('pos', 'u', 'steps', 'success', 'cons', 'choice') + (('over',) if self.shielded else ())}
        for c, b0 in enumerate(range(0, B, Bc)):
            idx = np.arange(b0, b0 + Bc)
            idx = np.minimum(idx, B - 1)   # the last chunk is padded with copies of the last task (results dropped)
            rep = np.repeat(idx, K)
            env.set_task(starts[rep], goals[rep])
            if nb:   # (a handle without blocks never has any)
                env.set_blocks(blocks[rep])
            if health is not None:
                env.set_map('health', health[rep])
            steps, success, cons, route, u, over = self._round(s, True, 0.0, first if K > 1 else torch.ones_like(first),
                                                               round_stream(seed, c, 0))
            if K > 1:
                st2, su2, co2, ro2, u2, ov2 = self._round(s, False, epsilon, 1 - first, round_stream(seed, c, 1))
                m = first.bool()
                if self.shielded:
                    over = torch.where(m, over, ov2)
                steps, success, cons = torch.where(m, steps, st2), torch.where(m, success, su2), torch.where(m, cons, co2)
                route = torch.where(m.view(E, 1, 1, 1), route, ro2)
                u = torch.where(m.view(E, 1, 1, 1), u, u2)
            pos_out = torch.empty((Bc, T + 1, n, 2), dtype=torch.uint8, device=dev)
            u_out = torch.empty((Bc, T, n), dtype=torch.int8, device=dev)
            choice = torch.empty(Bc, dtype=torch.int32, device=dev)
            lib.rollout_route_select(Bc, K, n, T, steps.data_ptr(), success.data_ptr(), cons.data_ptr(), 1, route.data_ptr(),
                                     u.data_ptr(), pos_out.data_ptr(), u_out.data_ptr(), choice.data_ptr(), stream)
            chip = torch.arange(Bc, device=dev) * K + choice.long()
            keep = min(Bc, B - b0)
            out['pos'].append(pos_out[:keep])
            out['u'].append(u_out[:keep])
            out['steps'].append(steps[chip][:keep])
            out['success'].append(success[chip][:keep])
            out['cons'].append(cons[chip][:keep])
            out['choice'].append(choice[:keep])
            if self.shielded:
                out['over'].append(over[chip][:keep])
        cat = {k: torch.cat(v).cpu().numpy() for k, v in out.items()}
        steps = cat['steps'].astype(np.int64)
        actions = np.where(np.arange(T)[None, :, None] < steps[:, None, None], cat['u'], np.int8(-1)).astype(np.int8)
        cons = cat['cons'].astype(np.int64) if self.name == 'dmfb' else cat['cons'].astype(np.float64)
        res = RouteResult(cat['pos'], actions, steps, cat['success'] > 0, cons, cat['choice'].astype(np.int32),
                          overrides=cat['over'].astype(np.int32) if self.shielded else None)
        if planned:
            res = self._plan(res, starts, goals, blocks, health, fallback == 'plan', planner)
        if fallback == 'follow':
            res = self._follow(res, starts, goals, blocks, health, float(min_health), seed, planner)
        return res
