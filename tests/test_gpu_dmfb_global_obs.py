"""The global state on the env (include/dmfb_vec.h: dmfb_vec_global_obs / _append), RoutingTaskManager.getglobalobs()
(dmfb.py:368-391): bit-exact against the reference's fixtures, against a numpy restatement over many chips and autoreset steps,
the episode append rule of the rollout, and the graphed QMIX episode against the eager one."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def numpy_state(W, L, pos, ends, blocks):
    """getglobalobs() restated: (E, n, 2) positions, (E, n, 2) goals, (E, nb, 4) blocks -> int8 (E, 3, W, L)."""
    E, n = pos.shape[:2]
    out = np.zeros((E, 3, W, L), np.int8)
    for e in range(E):
        for x0, x1, y0, y1 in blocks[e]:
            out[e, 2, x0:x1 + 1, y0:y1 + 1] = 1
        for i in range(n):
            out[e, 0, pos[e, i, 0], pos[e, i, 1]] = i + 1
            out[e, 1, ends[e, i, 0], ends[e, i, 1]] = i + 1
    return out


@pytest.mark.parametrize('name', ['A_12x9_3d_fov7', 'F_20x20_10d_fov9_12blocks', 'D_50x50_10d_fov9'])
def test_reference_fixtures_bit_exact(name):
    from marl_dmfb_amd.env.dmfb import VecDMFB
    g = np.load(os.path.join(GOLDEN, 'dmfb_%s.npz' % name))
    ref = np.load(os.path.join(GOLDEN, 'globalobs_%s.npz' % name))
    W, L, n, fov, stall, _ = [int(v) for v in g['cfg']]
    ep_len = g['ep_len'].astype(int)
    E = len(ep_len)
    nb = g['blocks'].shape[1] if 'blocks' in g else 0
    env = VecDMFB(W, L, n, nb, fov=fov, stall=bool(stall), n_envs=E, with_maps='health' in g, device='cuda:0')
    assert env.state_shape == 3 * W * L
    if 'health' in g:
        env.set_map('health', g['health'])
    if nb:
        env.set_blocks(g['blocks'])
    env.set_task(g['starts'], g['ends'])
    np.testing.assert_array_equal(env.global_obs().cpu().numpy(), ref['gobs0'])
    first = np.concatenate([[0], np.cumsum(ep_len)[:-1]])
    for t in range(ep_len.max()):
        active = np.nonzero(t < ep_len)[0]
        idx = first[active] + t
        actions = np.zeros((E, n), np.int32)
        uniforms = np.full((E, n), 2.0)
        actions[active] = g['actions'][idx]
        u = g['uniforms'][idx]
        uniforms[active] = np.where(np.isnan(u), 2.0, u)
        act = np.zeros(E, np.uint8)
        act[active] = 1
        env.step(actions, uniforms=uniforms, active=act)
        np.testing.assert_array_equal(env.global_obs().cpu().numpy()[active], ref['gobs'][idx], err_msg='t=%d' % t)


def test_facade_getglobalobs():
    from marl_dmfb_amd.env.dmfb import DMFBenv
    env = DMFBenv(12, 9, 3, fov=7, device='cuda:0')
    env.reset()
    g = env.routing_manager.getglobalobs()
    assert g.shape == (3, 12, 9) and g.dtype.kind == 'i'
    pos = env._vec.get_state()['pos'].cpu().numpy()
    _, ends = env._vec.get_task()
    np.testing.assert_array_equal(g, numpy_state(12, 9, pos, ends.cpu().numpy(), np.zeros((1, 0, 4), int))[0])


def test_many_chips_autoreset_against_numpy():
    from marl_dmfb_amd.env.dmfb import VecDMFB
    E, W, L, n, nb = 4096, 20, 20, 10, 6
    env = VecDMFB(W, L, n, nb, fov=9, n_envs=E, seed=3, device='cuda:0')
    env.reset(new=True)
    gen = torch.Generator(device='cuda:0').manual_seed(1)
    blocks = env.get_blocks().cpu().numpy()
    for t in range(200):
        a = torch.randint(0, 5, (E, n), device='cuda:0', generator=gen, dtype=torch.int32)
        env.step(a, autoreset=True)
        if t % 20 == 19 or t < 3:
            pos = env.get_state()['pos'].cpu().numpy()
            ends = env.get_task()[1].cpu().numpy()
            blocks = env.get_blocks().cpu().numpy()
            np.testing.assert_array_equal(env.global_obs().cpu().numpy(), numpy_state(W, L, pos, ends, blocks), err_msg='t=%d' % t)
    # the masked form leaves the other rows alone
    out = torch.full((E, 3, W, L), 77, dtype=torch.int8, device='cuda:0')
    mask = (torch.arange(E, device='cuda:0') % 3 == 0).to(torch.uint8)
    env.global_obs(mask=mask, out=out)
    full = env.global_obs()
    m = mask.bool()
    assert torch.equal(out[m], full[m]) and bool((out[~m] == 77).all())


def test_append_rule():
    from marl_dmfb_amd.env.dmfb import VecDMFB
    E, W, L, n, T = 64, 10, 10, 4, 6
    env = VecDMFB(W, L, n, fov=9, n_envs=E, seed=2, device='cuda:0')
    env.reset()
    S = env.state_shape
    s = torch.zeros((E, T, S), dtype=torch.int8, device='cuda:0')
    sn = torch.zeros_like(s)
    alive = (torch.arange(E, device='cuda:0') % 4 != 0).to(torch.uint8)
    term = (torch.arange(E, device='cuda:0') % 4 == 1).to(torch.uint8)
    cur = env.global_obs().view(E, S)
    for t in (2, T - 1):
        env.global_obs_append(alive, term, t, s, sn)
        a, tm = alive.bool(), term.bool()
        assert torch.equal(sn[a, t], cur[a]) and bool((sn[~a, t] == 0).all())
        if t + 1 < T:
            keep = a & ~tm
            assert torch.equal(s[keep, t + 1], cur[keep]) and bool((s[~keep, t + 1] == 0).all())
    assert int(s[:, :2].abs().sum()) == 0 and int(s[:, 4:].abs().sum()) == 0   # nothing else written (t = T - 1 writes no s)


def _qmix_trainer(use_graph):
    from marl_dmfb_amd.common.arguments import make_args
    from marl_dmfb_amd.env.dmfb import VecDMFB
    from marl_dmfb_amd.train import Trainer
    env = VecDMFB(10, 10, 4, fov=9, n_envs=256, seed=11, device='cuda:0')
    torch.manual_seed(5)
    args = make_args(alg='qmix', device='cuda:0', n_envs=256, batch_size=64, train_time=2, buffer_size=1024, anneal_steps=20000,
                     use_graph=use_graph, **env.get_env_info())
    return Trainer(env, args)


def test_qmix_episode_graphed_equals_eager_and_padding():
    a, b = _qmix_trainer(False), _qmix_trainer(True)
    assert not a.stream and not b.stream   # QMIX plays episode by episode
    b.agents.policy.eval_rnn.load_state_dict(a.agents.policy.eval_rnn.state_dict())
    b.agents.policy.target_rnn.load_state_dict(a.agents.policy.target_rnn.state_dict())
    b.agents.policy.eval_qmix_net.load_state_dict(a.agents.policy.eval_qmix_net.state_dict())
    a.agents.policy.init_hidden(1)
    a.rolloutWorker._play(a.rolloutWorker.epsilon.clone(), False, True)   # the graph's warm-up episode
    for rnd in range(2):
        ea = a.rolloutWorker.generate_episode()[4]
        eb = b.rolloutWorker.generate_episode()[4]
        for k in ea:
            assert torch.equal(ea[k], eb[k]), (rnd, k)
        s, sn, pad = ea['s'], ea['s_next'], ea['padded'][:, :, 0]
        assert s.shape == (256, 40, 300) and s.dtype == torch.int8
        assert bool((sn[pad] == 0).all()) and int((s[:, 1:][pad[:, :-1] | ea['terminated'][:, :-1, 0]]).abs().sum()) == 0
        valid_next = ~pad[:, 1:]
        assert torch.equal(sn[:, :-1][valid_next], s[:, 1:][valid_next])
        assert bool((s[:, 0].abs().sum(1) > 0).all())
        # the same learn on both sides keeps the two rollouts' weights equal for the next round
        for tr, ep in ((a, ea), (b, eb)):
            tr.buffer.store_episode(ep)
            tr.buffer.generator = torch.Generator(device='cuda:0').manual_seed(rnd)
            tr.agents.train(tr.buffer.sample(64), rnd)
