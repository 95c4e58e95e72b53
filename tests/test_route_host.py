"""Host side of routing given tasks (marl_dmfb_amd.route, marl_dmfb_amd.evaluate): task validation before anything is launched,
the best-of-K rule in numpy, the evaluate CLI's flags and file layout, and the C ABI of the new entry points.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from marl_dmfb_amd import _lib
from marl_dmfb_amd.route import Router, select_reference, validate_tasks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dmfb_task():
    starts = np.array([[[0, 0], [5, 5], [9, 9], [0, 9]]] * 3)
    goals = np.array([[[9, 0], [2, 7], [4, 4], [8, 8]]] * 3)
    return starts, goals


def test_valid_tasks_pass_and_are_made_contiguous_int32():
    s, g = _dmfb_task()
    s2, g2, b2, h2 = validate_tasks('dmfb', 10, 10, 4, s, g, blocks=np.array([[[2, 3, 0, 1]]] * 3),
                                    health=np.ones((3, 10, 10)))
    assert s2.dtype == np.int32 and g2.dtype == np.int32 and b2.dtype == np.int32 and h2.dtype == np.float64
    ms = np.array([[[2, 2], [27, 27], [2, 27], [27, 2]]])
    mg = np.array([[[15, 15], [10, 20], [20, 10], [5, 5]]])
    validate_tasks('meda', 30, 30, 4, ms, mg)


@pytest.mark.parametrize('mutate,msg', [
    (lambda s, g, b: s.__setitem__((2, 1, 0), 10), 'task 2: start of droplet 1'),          # x == width
    (lambda s, g, b: g.__setitem__((1, 3, 1), -1), 'task 1: goal of droplet 3'),           # negative
    (lambda s, g, b: s.__setitem__((1, 2), s[1, 0]), 'task 1: two starts on the same cell'),
    (lambda s, g, b: g.__setitem__((2, 0), g[2, 1]), 'task 2: two goals on the same cell'),
    (lambda s, g, b: b.__setitem__((1, 0), [5, 6, 5, 6]), 'task 1: start of droplet 1 lies inside block 0'),
    (lambda s, g, b: b.__setitem__((2, 0), [4, 4, 4, 4]), 'task 2: goal of droplet 2 lies inside block 0'),
    (lambda s, g, b: b.__setitem__((0, 0), [3, 2, 0, 1]), 'task 0: block 0'),
])
def test_dmfb_validation_names_the_first_bad_task(mutate, msg):
    s, g = _dmfb_task()
    b = np.array([[[2, 3, 0, 1]]] * 3)
    mutate(s, g, b)
    with pytest.raises(ValueError, match=re.escape(msg)):
        validate_tasks('dmfb', 10, 10, 4, s, g, blocks=b)


def test_dmfb_chip_axes_are_width_then_length():
    s = np.array([[[11, 0]]])
    g = np.array([[[0, 5]]])
    validate_tasks('dmfb', 12, 6, 1, s, g)            # x < width = 12, y < length = 6
    with pytest.raises(ValueError, match='task 0: start'):
        validate_tasks('dmfb', 6, 12, 1, s, g)


@pytest.mark.parametrize('bad', [[1, 15], [15, 1], [28, 15], [15, 28]])
def test_meda_centres_keep_their_box_on_the_chip(bad):
    s = np.array([[[15, 15], [5, 5]], [[5, 5], [20, 20]]])
    g = np.array([[[25, 25], [10, 20]], [[25, 25], [10, 20]]])
    s[1, 1] = bad
    with pytest.raises(ValueError, match=re.escape('task 1: start of droplet 1')):
        validate_tasks('meda', 30, 30, 2, s, g)
    s[1, 1] = [2, 27]
    validate_tasks('meda', 30, 30, 2, s, g)


def test_meda_centre_axes_follow_the_map_order():
    # meda_vec_get_map order (y < width, x < length): a 30 x 60 chip takes x up to 57 and y up to 27
    s = np.array([[[57, 27]]])
    g = np.array([[[2, 2]]])
    validate_tasks('meda', 30, 60, 1, s, g)
    with pytest.raises(ValueError, match='task 0: start'):
        validate_tasks('meda', 60, 30, 1, s, g)


@pytest.mark.parametrize('kw,msg', [
    (dict(starts=np.zeros((2, 3, 2), int)), 'starts must have shape'),
    (dict(goals=np.zeros((2, 4, 2), int)), 'goals must have the shape'),
    (dict(blocks=np.zeros((2, 1, 3), int)), 'blocks must be'),
    (dict(health=np.ones((3, 10, 9))), 'health must have shape'),
    (dict(starts=np.zeros((3, 4, 2)) + 0.5), 'integer'),
])
def test_shapes_are_checked(kw, msg):
    s, g = _dmfb_task()
    args = dict(starts=s, goals=g)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        validate_tasks('dmfb', 10, 10, 4, **args)


def test_router_validates_before_it_touches_a_device():
    s, g = _dmfb_task()
    s[1, 0] = [-3, 0]
    r = Router(agents=None, name='dmfb', width=10, length=10, n_agents=4, fov=9, device='cpu')
    with pytest.raises(ValueError, match='task 1'):
        r.route(s, g)
    with pytest.raises(ValueError, match='blocks are a DMFB feature'):
        Router(None, name='meda', width=30, length=30, n_agents=4, fov=19, device='cpu').route(
            np.array([[[5, 5]] * 4]), np.array([[[9, 9]] * 4]), blocks=np.zeros((1, 1, 4), int))
    with pytest.raises(ValueError, match='tries'):
        r.route(*_dmfb_task(), tries=0)
    assert r.rounds == 0 and not r._slots


def test_empty_batch_returns_an_empty_result():
    r = Router(agents=None, name='dmfb', width=10, length=10, n_agents=4, fov=9, device='cpu')
    res = r.route(np.zeros((0, 4, 2), int), np.zeros((0, 4, 2), int), tries=3)
    assert len(res) == 0 and res.positions.shape == (0, 41, 4, 2) and res.actions.shape == (0, 40, 4)
    assert res.constraints.dtype == np.int64 and r.rounds == 0 and not r._slots
    m = Router(None, name='meda', width=30, length=30, n_agents=4, fov=19, device='cpu').route(np.zeros((0, 4, 2), int),
                                                                                               np.zeros((0, 4, 2), int))
    assert m.positions.shape == (0, 61, 4, 2) and m.constraints.dtype == np.float64


def test_round_streams_are_distinct_per_seed_chunk_and_round():
    from marl_dmfb_amd.route import round_stream
    starts = {round_stream(seed, c, r)[0] for seed in range(50) for c in range(4) for r in range(2)}
    assert len(starts) == 400
    assert round_stream(3, 1, 1) == round_stream(3, 1, 1)
    # the counter ranges of one round (at most 2 * (255 + 255) lock-steps) do not overlap
    ordered = sorted(starts)
    assert min(b - a for a, b in zip(ordered, ordered[1:])) > 1020


def test_router_block_limit():
    s, g = _dmfb_task()
    r = Router(agents=None, name='dmfb', width=10, length=10, n_agents=4, fov=9, n_blocks=1, device='cpu')
    with pytest.raises(ValueError, match='at most 1'):
        r.route(s, g, blocks=np.array([[[2, 3, 0, 1], [6, 7, 0, 1]]] * 3))


def test_select_rule_on_hand_built_ties():
    K = 4
    # (success, steps, constraints) per try -> expected winner
    cases = [
        ([0, 1, 0, 0], [5, 40, 3, 2], [0, 0, 0, 0], 1),      # the only success wins whatever its steps
        ([0, 0, 0, 0], [40, 40, 40, 40], [3, 1, 1, 2], 1),   # all failed: constraints, then the lower index
        ([1, 1, 1, 1], [9, 7, 7, 8], [0, 5, 4, 0], 2),       # steps tie between 1 and 2: fewer constraints
        ([1, 1, 1, 1], [7, 7, 7, 7], [2, 2, 2, 2], 0),       # full tie: the lowest try index
        ([2, 1, 0, 1], [8, 6, 1, 6], [1, 1, 0, 0], 3),       # success counts as a flag; steps tie -> constraints
        ([0, 0, 1, 1], [3, 3, 9, 9], [0.5, 0.25, 1.5, 1.25], 3),   # float constraints (MEDA)
    ]
    su = np.array([c[0] for c in cases]).ravel()
    st = np.array([c[1] for c in cases]).ravel()
    co = np.array([c[2] for c in cases], dtype=np.float64).ravel()
    assert select_reference(st, su, co, K).tolist() == [c[3] for c in cases]
    assert select_reference([4, 2], [0, 0], [1, 0], 1).tolist() == [0, 0]   # K = 1: nothing to choose


def test_evaluate_parser_defaults_and_files():
    from marl_dmfb_amd.common.arguments import get_route_args
    a = get_route_args(['dmfb'])
    assert (a.name, a.width, a.length, a.fov, a.evaluate_task, a.n_envs) == ('dmfb', 10, 10, 9, 100, 4096)
    assert a.load_model is True and a.model_dir == './model' and a.load_model_name == '' and a.alg == 'vdn'
    assert a.routes == '' and a.tasks == '' and a.tries == 1 and a.route_epsilon == 0.1 and a.seed == 12
    a = get_route_args(['dmfb', '--chip_size', '20', '--tasks', 't.npz', '--routes', 'r.npz', '--tries', '8', '--epsilon', '0.2',
                        '--seed', '3'])
    assert (a.width, a.length, a.tasks, a.routes, a.tries, a.route_epsilon, a.seed) == (20, 20, 't.npz', 'r.npz', 8, 0.2, 3)
    m = get_route_args(['meda', '--alg', 'qmix', '--meda_state', '-d', '4'])
    assert (m.width, m.length, m.fov, m.version, m.alg, m.meda_state) == (30, 60, 19, '0.2', 'qmix', True)
    assert m.hyper_hidden_dim == 32


def test_get_evaluate_args_is_unchanged():
    from marl_dmfb_amd.common.arguments import get_evaluate_args
    a = get_evaluate_args(['dmfb', '--chip_size', '20', '-d', '10'])
    assert (a.width, a.length, a.drop_num, a.fov, a.evaluate_epoch, a.evaluate_task, a.n_envs) == (20, 20, 10, 9, 20, 100, 5)
    assert a.load_model is True and a.b_degrade is True and a.per_degrade == 0 and a.hyper_hidden_dim == 24
    assert not hasattr(a, 'routes') and not hasattr(a, 'tasks') and not hasattr(a, 'tries') and not hasattr(a, 'route_epsilon')
    assert a.epsilon == 1.0


def test_evaluate_cli_writes_the_documented_route_file(tmp_path, monkeypatch):
    """The --routes layout of a --tasks run, with the router stubbed (the routes themselves are tested on the GPU)."""
    from marl_dmfb_amd import evaluate, route
    from marl_dmfb_amd.common.arguments import get_route_args
    B, T, n = 3, 80, 4
    s, g = _dmfb_task()
    np.savez(tmp_path / 'tasks.npz', starts=s, goals=g, blocks=np.array([[[2, 3, 0, 1]]] * 3))
    seen = {}

    class FakeRouter:
        def __init__(self, agents, **kw):
            seen['kw'] = kw

        def route(self, starts, goals, blocks=None, health=None, tries=1, epsilon=0.1, seed=0):
            seen['call'] = (starts.shape, goals.shape, None if blocks is None else blocks.shape, health, tries, epsilon, seed)
            return route.RouteResult(np.zeros((B, T + 1, n, 2), np.uint8), np.full((B, T, n), -1, np.int8),
                                     np.array([5, 80, 7]), np.array([True, False, True]), np.array([0, 2, 1]),
                                     np.array([0, 3, 1], np.int32))

    class FakeEnv:
        state_shape, device = 300, 'cuda:0'

        def get_env_info(self):
            return {'n_actions': 5, 'n_agents': 4, 'obs_shape': (3, 9, 9, 2, 245), 'episode_limit': 80}

        def close(self):
            pass

    monkeypatch.setattr(route, 'Router', FakeRouter)
    monkeypatch.setattr(evaluate, '_make_env', lambda args, n_envs: FakeEnv())
    monkeypatch.setattr('marl_dmfb_amd.agent.agent.Agents', lambda args: None)
    out = tmp_path / 'routes.npz'
    evaluate.main(['dmfb', '--chip_size', '10', '--block_num', '1', '--tasks', str(tmp_path / 'tasks.npz'), '--routes', str(out),
                   '--tries', '4', '--epsilon', '0.3', '--seed', '5'])
    assert seen['call'] == ((3, 4, 2), (3, 4, 2), (3, 1, 4), None, 4, 0.3, 5)
    assert seen['kw']['n_blocks'] == 1 and seen['kw']['name'] == 'dmfb'
    with np.load(out) as f:
        assert sorted(f.files) == sorted(['positions', 'actions', 'steps', 'success', 'constraints', 'try_index', 'starts',
                                          'goals', 'blocks', 'cfg'])
        assert f['positions'].shape == (B, T + 1, n, 2) and f['actions'].shape == (B, T, n)
        assert f['cfg'].tolist() == [10, 10, 4, 9, 1, 1]
        np.testing.assert_array_equal(f['starts'], s)


def test_new_entry_points_are_declared_and_bound():
    """dmfb / meda route append in their headers and binding tables (the tables must equal the headers, tests/test_cabi_exports.py),
    rollout_route_select in include/rollout_route.h with its own table; argument guards before any launch."""
    def protos(header):
        txt = open(os.path.join(ROOT, 'include', header)).read()
        txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
        txt = re.sub(r'^\s*#.*$', '', txt, flags=re.M)
        return {name: (0 if p.strip() in ('', 'void') else p.count(',') + 1)
                for name, p in re.findall(r'\b([a-z][a-z_0-9]*)\s*\(([^()]*)\)\s*;', txt)}
    assert protos('dmfb_vec.h')['dmfb_vec_route_append'] == 5 and protos('meda_vec.h')['meda_vec_route_append'] == 5
    assert 'dmfb_vec_route_append' in _lib.DMFB_VEC_SYMBOLS and 'meda_vec_route_append' in _lib.MEDA_VEC_SYMBOLS
    declared = protos('rollout_route.h')
    assert declared == {'rollout_route_select': 14}
    lib = _lib.rollout_route()
    assert len(lib.rollout_route_select.argtypes) == 14
    assert lib.rollout_route_select(-1, 1, 4, 40, None, None, None, 0, None, None, None, None, None, None) == -1
    assert lib.rollout_route_select(4, 0, 4, 40, None, None, None, 0, None, None, None, None, None, None) == -1
    host = C.create_string_buffer(64)
    p = C.addressof(host)
    assert lib.rollout_route_select(4, 2, 4, 40, p, p, p, 0, p, None, None, None, p, None) == -1   # route without route_out
    assert lib.rollout_route_select(4, 2, 4, 0, p, p, p, 0, None, None, None, None, p, None) == -1  # T < 1
    assert lib.rollout_route_select(0, 2, 4, 40, p, p, p, 0, None, None, None, None, p, None) == 0   # nothing to do
    assert _lib.dmfb_vec().dmfb_vec_route_append(None, 0, 40, None, None) == -1
    assert _lib.meda_vec().meda_vec_route_append(None, 0, 40, None, None) == -1
