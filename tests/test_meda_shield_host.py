"""The MEDA shield rule on the CPU (marl_dmfb_amd.shield.meda_shield_reference): in lock-step with the CPU oracle it leaves no
proximity penalty where the unshielded picks leave many, no subset of failed moves brings two centres within 6 and the next
state is safe again, and the unsafe, forced, pick, tie and inactive rules hold case by case.  Every comparison is exact."""
import itertools

import numpy as np
import pytest

from marl_dmfb_amd import plan
from marl_dmfb_amd.shield import MEDA_DELTAS, meda_anchors, meda_shield_reference, meda_targets
from meda_shield_helpers import CONFIGS, d2, next_anchors, pairwise_clear, play_oracle, random_safe_states

FAR = [[25, 25], [25, 5]]     # goals out of everybody's way


def _q(best, n=1):
    """q (1, n, 9) whose descending order starts with `best`; the actions not named follow in ascending order."""
    rest = [a for a in range(9) if a not in best]
    q = np.zeros((1, n, 9), np.float32)
    for rank, a in enumerate(list(best) + rest):
        q[0, :, a] = 20.0 - rank
    return q


def test_the_moves_are_those_of_the_planner():
    assert MEDA_DELTAS.tolist() == [list(d) for d in plan.MEDA_DELTA]
    rng = np.random.default_rng(0)
    pos = np.stack([rng.integers(2, 10, (5, 3)), rng.integers(2, 17, (5, 3))], -1)       # 20 wide (y), 12 long (x)
    cells = meda_targets(20, 12, pos)
    for e, i, u in itertools.product(range(5), range(3), range(9)):
        assert tuple(cells[e, i, u]) == plan.meda_move(tuple(pos[e, i]), u, 20, 12)


# ------------------------------------------------------------------------------------------ lock-step against the oracle
@pytest.mark.parametrize('health', [False, True], ids=['healthy', 'health'])
@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_shielded_play_has_no_proximity_penalty_in_the_oracle(name, health):
    events, penalty, overrides, unsafe = play_oracle(name, shielded=True, health=health)
    print('%s health=%s shielded: events %d, penalty %.1f, overrides %d, unsafe %d' % (name, health, events, penalty, overrides, unsafe))
    assert events == 0 and penalty == 0.0        # `events`: not at any lock-step of any chip
    assert unsafe == 0
    assert overrides > 0


@pytest.mark.parametrize('health', [False, True], ids=['healthy', 'health'])
@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_the_same_seeds_unshielded_do_come_too_close(name, health):
    events, penalty, _, _ = play_oracle(name, shielded=False, health=health)
    print('%s health=%s unshielded: events %d, penalty %.1f' % (name, health, events, penalty))
    assert events > 0 and penalty > 0.0


# ------------------------------------------------------------------------------------------ failed moves
@pytest.mark.parametrize('n', [3, 4])
def test_no_subset_of_failed_moves_brings_two_centres_within_six(n):
    """1 000 safe states (crowded ones: the chips are 15 to 24 wide), free droplets, droplets one move from their disc, inside it
    and done.  After the shield, under every one of the 2^n masks of failed moves the env's step reports no penalty and the
    anchors of the next state are pairwise 6 apart."""
    rng = np.random.default_rng(10 + n)
    count, replaced, kinds = 0, 0, np.zeros(3, np.int64)
    for W, L in ((15, 16), (18, 15), (20, 24), (24, 20)):
        pos, goals, done = random_safe_states(rng, 250, W, L, n)
        forced, anchor = meda_anchors(pos, goals, done)
        assert pairwise_clear(anchor).all()
        kinds += [int(done.sum()), int((forced & ~done).sum()), int((~forced).sum())]
        q = rng.integers(0, 3, (250, n, 9)).astype(np.float32)
        picked = rng.integers(0, 9, (250, n))
        act, over, unsafe = meda_shield_reference(W, L, pos, goals, done, q, picked)
        assert not unsafe.any()
        assert (act[forced] == picked[forced]).all()
        replaced += int(over.sum())
        for e in range(250):
            g = [tuple(x) for x in goals[e].tolist()]
            for failed in itertools.product((False, True), repeat=n):
                p, d = [tuple(x) for x in pos[e].tolist()], done[e].tolist()
                u = [2.0 if f else 0.0 for f in failed]             # no health map: a move succeeds iff u <= 1
                fail = plan._meda_env_step(W, L, p, g, d, act[e].tolist(), u, None)
                assert fail == 0.0, (e, failed)
                assert pairwise_clear(next_anchors(p, g, d)).all(), (e, failed)
        count += 250
    assert count == 1000 and replaced > 0
    assert (kinds > 100).all(), kinds       # done, inside the disc, free


# ------------------------------------------------------------------------------------------ unsafe pre-states
def test_an_unsafe_pre_state_keeps_the_pick_and_sets_the_byte():
    # two free droplets 5 apart, droplet 0 in the corner of a 12 x 12 chip: every centre it can reach is within 6 of droplet 1
    pos = np.array([[[2, 2], [5, 6]]])
    goals = np.array([[[9, 9], [9, 2]]])
    assert d2(pos[0, 0], pos[0, 1]) == 25
    q = _q([5, 1, 2], n=2)
    act, ov, un = meda_shield_reference(12, 12, pos, goals, np.zeros((1, 2), bool), q, np.array([[5, 8]]))
    # droplet 0 keeps SE (new centre (4, 4)); every centre droplet 1 can reach is within 6 of (2, 2) or of (4, 4), so it keeps
    # its STALL too: no override, and the byte is set
    assert act.tolist() == [[5, 8]] and ov.tolist() == [0] and un.tolist() == [1]
    # the same with an out-of-range pick of droplet 0: kept, and it counts as staying on (2, 2)
    act, ov, un = meda_shield_reference(12, 12, pos, goals, np.zeros((1, 2), bool), q, np.array([[11, 5]]))
    assert act.tolist() == [[11, 5]] and ov.tolist() == [0] and un.tolist() == [1]
    # in the open both droplets of such a pair have a way out (W to (7, 10), E to (18, 10)): each flees the other's anchor, and
    # the byte stays clear -- it tells that a droplet had no safe action, not that two anchors were close
    pos = np.array([[[10, 10], [15, 10]]])
    act, ov, un = meda_shield_reference(30, 30, pos, np.array([FAR]), np.zeros((1, 2), bool), np.zeros((1, 2, 9), np.float32),
                                        np.array([[8, 8]]))
    assert act.tolist() == [[3, 1]] and ov.tolist() == [2] and un.tolist() == [0]


# ------------------------------------------------------------------------------------------ rule details
def test_forced_droplets_are_never_overridden_and_constrain_from_their_goal():
    # droplet 1 is inside its disc (goal (20, 10)): whatever it picks it is snapped to its goal, and its pick stays; droplet 2 is
    # done on its goal.  Droplet 0 at (12, 10) may not go E to (15, 10), 5 from the goal, although droplet 1's centre (22, 12)
    # is far enough from it
    pos = np.array([[[12, 10], [22, 12], [5, 25]]])
    goals = np.array([[[25, 25], [20, 10], [5, 25]]])
    done = np.array([[False, False, True]])
    assert d2(pos[0, 1], goals[0, 1]) < 16 and d2([15, 10], pos[0, 1]) >= 36 and d2([15, 10], goals[0, 1]) < 36
    q = _q([1, 5, 2], n=3)
    act, ov, un = meda_shield_reference(30, 30, pos, goals, done, q, np.array([[1, 3, 0]]))
    assert act.tolist() == [[5, 3, 0]] and ov.tolist() == [1] and un.tolist() == [0]
    # forced droplets keep even an out-of-range pick, and one that would be unsafe for a free droplet
    act, ov, un = meda_shield_reference(30, 30, pos, goals, done, q, np.array([[8, -4, 99]]))
    assert act.tolist() == [[8, -4, 99]] and ov.tolist() == [0] and un.tolist() == [0]


def test_a_move_into_the_own_disc_is_judged_by_the_goal_too():
    # droplet 0 at (10, 10) with goal (14, 10): E reaches (13, 10), inside its disc, so one step later it stands on (14, 10).
    # Droplet 1 rests on (20, 10): 7 from (13, 10) but 6 from (14, 10) -- still safe; on (19, 10) it is 5 from the goal -- unsafe
    goals = np.array([[[14, 10], [25, 25]]])
    q = _q([1, 0], n=2)
    for x1, want in ((20, 1), (19, 0)):
        pos = np.array([[[10, 10], [x1, 10]]])
        act, _, un = meda_shield_reference(30, 30, pos, goals, np.zeros((1, 2), bool), q, np.array([[1, 8]]))
        assert act.tolist() == [[want, 8]] and un.tolist() == [0]


def test_a_later_droplet_yields_to_the_new_centre_of_an_earlier_one():
    pos = np.array([[[10, 10], [19, 10]]])      # both move towards one another: 0 goes first, 1 must give way
    q = np.stack([_q([1, 8])[0, 0], _q([3, 8])[0, 0]])[None]
    act, ov, un = meda_shield_reference(30, 30, pos, np.array([FAR]), np.zeros((1, 2), bool), q, np.array([[1, 3]]))
    assert act.tolist() == [[1, 8]] and ov.tolist() == [1] and un.tolist() == [0]


def test_pick_nan_and_tie_orders():
    pos = np.array([[[10, 10], [16, 10]]])      # droplet 0: E, NE and SE come within 6 of droplet 1
    none = np.zeros((1, 2), bool)
    run = lambda q, picked: meda_shield_reference(30, 30, pos, np.array([FAR]), none, q, np.array([picked]))[0].tolist()
    # a safe pick stays even when it is not the arg-max
    assert run(_q([2, 0], n=2), [6, 8]) == [[6, 8]]
    # an unsafe pick gives way to the best safe q
    assert run(_q([1, 4, 7, 0], n=2), [1, 8]) == [[7, 8]]
    # an out-of-range pick gives way to the arg-max when that is safe
    assert run(_q([3, 0], n=2), [9, 8]) == [[3, 8]]
    assert run(_q([3, 0], n=2), [-1, 8]) == [[3, 8]]
    # equal q: the lower action
    assert run(np.zeros((1, 2, 9), np.float32), [1, 8]) == [[0, 8]]
    q = np.zeros((1, 2, 9), np.float32)
    q[0, 0] = [-1, 5, 2, 2, 9, 9, -1, -1, -1]
    assert run(q, [1, 8]) == [[2, 8]]
    # a NaN orders below every number, and -0.0 ties with 0.0
    q[0, 0] = [np.nan, 5, np.nan, -np.inf, 9, 9, np.nan, np.nan, np.nan]
    assert run(q, [1, 8]) == [[3, 8]]
    q[0, 0] = [np.nan] * 9
    assert run(q, [1, 8]) == [[0, 8]]
    q[0, 0] = [-5, 5, 0.0, -0.0, -5, -5, -5, -5, -5]
    assert run(q, [1, 8]) == [[2, 8]]
    q[0, 0] = [-5, 5, -0.0, 0.0, -5, -5, -5, -5, -5]
    assert run(q, [1, 8]) == [[2, 8]]


def test_the_clamps_count():
    # droplet 0 in the corner (2, 2) of a chip 12 wide and 20 long: N, W and NW leave it where it is, NE and SW move along one
    # axis only; droplet 1 on (10, 2) forbids E (5, 2), 5 away, and not NE (4, 2), 6 away
    pos = np.array([[[2, 2], [10, 2]]])
    goals = np.array([[[9, 9], [17, 9]]])
    assert meda_targets(12, 20, pos)[0, 0].tolist() == [[2, 2], [5, 2], [2, 5], [2, 2], [4, 2], [4, 4], [2, 4], [2, 2], [2, 2]]
    assert meda_targets(12, 20, np.array([[[17, 9]]]))[0, 0].tolist() == [[17, 6], [17, 9], [17, 9], [14, 9], [17, 7], [17, 9],
                                                                         [15, 9], [15, 7], [17, 9]]
    act, _, _ = meda_shield_reference(12, 20, pos, goals, np.zeros((1, 2), bool), _q([1, 4], n=2), np.array([[1, 8]]))
    assert act.tolist() == [[4, 8]]


def test_inactive_chips_are_untouched():
    pos = np.tile(np.array([[[10, 10], [16, 10]]]), (3, 1, 1))
    goals = np.tile(np.array([FAR]), (3, 1, 1))
    q = np.tile(_q([1, 3], n=2), (3, 1, 1))
    picked = np.tile(np.array([[1, 8]]), (3, 1))
    act, ov, un = meda_shield_reference(30, 30, pos, goals, np.zeros((3, 2), bool), q, picked, active=np.array([1, 0, 2]))
    assert act.tolist() == [[3, 8], [1, 8], [3, 8]] and ov.tolist() == [1, 0, 1] and un.tolist() == [0, 0, 0]
    corner = np.tile(np.array([[[2, 2], [5, 6]]]), (2, 1, 1))
    _, _, un = meda_shield_reference(12, 12, corner, np.tile(np.array([[[9, 9], [9, 2]]]), (2, 1, 1)), np.zeros((2, 2), bool),
                                     q[:2], picked[:2], active=np.array([0, 1]))
    assert un.tolist() == [0, 1]
