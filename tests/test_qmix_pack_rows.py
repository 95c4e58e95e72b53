"""Host side of the packed QMIX learn (policy/qmix.py), no device work: QMIX.pack_state_rows against a brute-force loop over
(episode, step), and the --qmix_packed flag (parser, make_args, packed_ok on nothing, the Trainer's refusal outside stream mode)."""
import types

import numpy as np
import pytest
import torch

from marl_dmfb_amd.common.arguments import get_train_args, make_args
from marl_dmfb_amd.policy.qmix import QMIX
from marl_dmfb_amd.policy.vdn import VDN


def _brute(idx, lens, t_ring):
    """(units, rows, target_row) by walking step after step over the episodes longer than the step, as the packed layout is
    defined (include/vdn_ops.h: vdn_td_forward_packed; include/qmix_packed.h)."""
    B = len(idx)
    where = {}
    units, rows = [], []
    for t in range(int(max(lens))):
        for k in range(B):
            if lens[k] > t:
                where[(k, t)] = len(units)
                units.append(idx[k] * t_ring + t)
                rows.append(idx[k] * (t_ring + 1) + t)
    U = len(units)
    for k in range(B):
        rows.append(idx[k] * (t_ring + 1) + lens[k])
    target = [where[(k, t + 1)] if lens[k] > t + 1 else U + k for (k, t) in sorted(where, key=where.get)]
    return np.asarray(units), np.asarray(rows), np.asarray(target)


def _draw(idx, lens):
    idx, lens = np.asarray(idx), np.asarray(lens)
    order = np.argsort(-lens, kind='stable')           # ReplayBuffer.draw
    return idx[order], lens[order]


_RNG = np.random.default_rng(5)
CASES = {
    'one_episode': ([7], [5], 8),
    'all_length_1': ([3, 0, 9, 4], [1, 1, 1, 1], 6),
    'all_equal': ([2, 5, 1], [4, 4, 4], 6),
    'length_equals_t_ring': ([4, 1, 6], [6, 2, 6], 6),
    'repeated_slots': ([3, 3, 8, 3, 8], [5, 5, 2, 5, 2], 7),
    'random_64': (_RNG.integers(0, 500, 64).tolist(), _RNG.integers(1, 41, 64).tolist(), 40),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_pack_state_rows_against_brute_force(name):
    idx, lens, t_ring = CASES[name]
    if name == 'repeated_slots':
        assert len(set(idx)) < len(idx)
    if name == 'length_equals_t_ring':
        assert max(lens) == t_ring
    idx, lens = _draw(idx, lens)
    counts, units = VDN.pack_units(idx, lens, t_ring)
    rows, target = QMIX.pack_state_rows(idx, lens, counts, t_ring)
    U, B = len(units), len(idx)
    assert U == int(np.sum(lens)) and rows.dtype == np.int32 and target.dtype == np.int32
    assert rows.shape == (U + B,) and target.shape == (U,)
    want_units, want_rows, want_target = _brute(idx, lens, t_ring)
    np.testing.assert_array_equal(units, want_units)
    np.testing.assert_array_equal(rows, want_rows)
    np.testing.assert_array_equal(target, want_target)
    # what the layout means: the target row of a unit holds the state one slot behind the unit's own, in the same ring slot
    np.testing.assert_array_equal(rows[target], rows[:U] + 1)
    np.testing.assert_array_equal(rows[:U] // (t_ring + 1), units // t_ring)
    np.testing.assert_array_equal(rows[:U] % (t_ring + 1), units % t_ring)
    if name == 'length_equals_t_ring':
        assert int((rows[U:] % (t_ring + 1) == t_ring).sum()) == 2        # the closing row is slot T of the ring


def test_flag_parses_and_defaults_off():
    assert get_train_args([]).qmix_packed is False
    assert make_args().qmix_packed is False and make_args(alg='qmix').qmix_packed is False
    a = get_train_args(['dmfb', '--alg', 'qmix', '--stream_state', '--qmix_packed'])
    assert a.qmix_packed is True and a.stream_state is True


KW = dict(cuda=False, device='cpu', n_actions=5, n_agents=4, obs_shape=(3, 9, 9, 2, 245), episode_limit=40, state_shape=300)


def test_packed_ok_stays_false_on_nothing():
    from marl_dmfb_amd.agent.agent import Agents
    for flag in (False, True):
        pol = Agents(make_args(alg='qmix', qmix_packed=flag, **KW)).policy
        assert pol.packed_ok({}) is False
        cpu = {'o': torch.zeros((4, 40, 4, 245), dtype=torch.int8)}
        assert pol.packed_ok(cpu) is False
    assert Agents(make_args(alg='vdn', qmix_packed=True, **KW)).policy.packed_ok({}) is False


def _env():
    return types.SimpleNamespace(device=torch.device('cpu'), n_envs=6, seed=0, env_id0=0, obs_len=245, max_step=40, width=10,
                                 length=10, state_shape=300)


def test_trainer_refuses_the_flag_outside_stream_mode(tmp_path):
    from marl_dmfb_amd.train import Trainer
    kw = dict(KW, n_envs=6, batch_size=4, buffer_size=24, model_dir=str(tmp_path / 'model'), result_dir=str(tmp_path / 'result'))
    with pytest.raises(ValueError, match='--stream_state'):
        Trainer(_env(), make_args(alg='qmix', qmix_packed=True, **kw))
    with pytest.raises(ValueError, match='--stream_state'):
        Trainer(_env(), make_args(alg='qmix', qmix_packed=True, stream=False, stream_state=True, **kw))
    assert not Trainer(_env(), make_args(alg='qmix', **kw)).stream            # without the flag: as before
    assert not Trainer(_env(), make_args(alg='vdn', qmix_packed=True, **kw)).stream   # VDN ignores the flag


def test_padded_learn_refuses_to_run_under_the_flag():
    """With the flag set a learn on the padded batch means packed_ok was False: it raises at that first learn."""
    from marl_dmfb_amd.agent.agent import Agents
    pol = Agents(make_args(alg='qmix', qmix_packed=True, **KW)).policy
    with pytest.raises(RuntimeError, match='qmix_packed'):
        pol.learn({}, 1, 0)
