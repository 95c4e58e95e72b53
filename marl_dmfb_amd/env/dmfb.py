"""Host side of the vectorised DMFB environment.

`VecDMFB` drives E lock-step chips through the C ABI in include/dmfb_vec.h (HIP kernels in
marl_dmfb_amd/csrc/dmfb_vec.hip); every array it hands back is a torch tensor living in HBM.
`DMFBenv` is the reference-shaped single-chip facade with the object protocol of the
reference's `DMFBenv` (env/DMFB/dmfb.py:474-640), so code written against the reference
(`RolloutWorker`, `evaDegre.py`, ...) can drive the HIP path unchanged.  PyTorch is used
only for device memory and streams.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ._vec import VecEnv, _ptr


class VecDMFB(VecEnv):
    """E independent DMFB chips advanced in lock-step on one MI355X.

    Constructor arguments are those of the reference's DMFBenv (dmfb.py:487) plus the batch:
    n_envs, seed (Philox key), env_id0 (global index of env 0 when a batch is sharded over
    ranks), with_maps (keep health/usage/degrade maps although b_degrade is False)."""
    LIB, NAME, STEP_RECORD, CONSTRAINTS = 'dmfb_vec', 'VecDMFB', 1, 'constraints'
    STATE_LAYERS = 3   # routing_manager.getglobalobs() (dmfb.py:368-391): droplets, goals, blocks (include/dmfb_vec.h)
    SHIELD_FLAG, N_ACTIONS = 'shield', 5   # the action shield (_vec.py: shield; include/dmfb_vec.h: dmfb_vec_shield)

    def __init__(self, width, length, n_agents, n_blocks=0, fov=5, stall=True, b_degrade=False,
                 per_degrade=0.1, n_envs=1, seed=0, with_maps=False, env_id0=0, device=None):
        self.seed, self.env_id0 = int(seed), int(env_id0)
        self.width, self.length, self.n_agents, self.fov = width, length, n_agents, fov
        self.n_envs, self.stall, self.b_degrade = n_envs, bool(stall), bool(b_degrade)
        self.n_blocks = n_blocks
        self.has_maps = bool(b_degrade or with_maps)
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.cfg = _lib.DmfbVecConfig(width, length, n_agents, n_blocks, fov, int(bool(stall)), int(bool(b_degrade)),
                                      int(bool(with_maps)), float(per_degrade), n_envs, env_id0, seed, dev.index or 0)
        self._create(dev)
        self.obs_len = 3 * fov * fov + 2
        self.max_step = 2 * (width + length)
        E, n, dev = n_envs, n_agents, self.device
        # outputs of a transition, allocated once and reused every step
        self.obs = torch.zeros((E, n, self.obs_len), dtype=torch.int8, device=dev)
        self.rewards = torch.zeros((E, n), dtype=torch.float64, device=dev)
        self.dones = torch.zeros((E, n), dtype=torch.uint8, device=dev)
        self.constraints = torch.zeros((E,), dtype=torch.int32, device=dev)
        self.success = torch.zeros((E,), dtype=torch.uint8, device=dev)
        self.team_reward = torch.zeros((E,), dtype=torch.float64, device=dev)
        self.terminated = torch.zeros((E,), dtype=torch.uint8, device=dev)
        self._out = _lib.DmfbVecStepOut(self.rewards.data_ptr(), self.dones.data_ptr(), self.constraints.data_ptr(),
                                        self.success.data_ptr(), self.obs.data_ptr(), self.team_reward.data_ptr(),
                                        self.terminated.data_ptr(), None)

    def get_env_info(self):
        """DMFBenv.get_env_info (dmfb.py:633-640)."""
        return {'n_actions': 5, 'n_agents': self.n_agents,
                'obs_shape': (3, self.fov, self.fov, 2, self.obs_len), 'episode_limit': self.max_step}

    def reset(self, mask=None, new=False, obs=None):
        """DMFBenv.reset(new) for the masked envs (all when mask is None); returns self.obs with
        the rows of the reset envs refreshed."""
        obs = self.obs if obs is None else obs
        self.lib.dmfb_vec_reset(self.h, _ptr(self._mask(mask)), int(bool(new)), _ptr(obs), self._stream())
        return obs

    def set_blocks(self, blocks):
        """Obstacle injection: blocks [E, nb, 4] = (x_min, x_max, y_min, y_max) (dmfb.py:34-41)."""
        b = self._dev(blocks, torch.int32).reshape(self.n_envs, -1, 4)
        self.lib.dmfb_vec_set_blocks(self.h, _ptr(b) if b.shape[1] else None, b.shape[1], self._stream())

    def get_blocks(self):
        nb = C.c_int(0)
        buf = torch.zeros((self.n_envs, max(1, self.n_blocks), 4), dtype=torch.int32, device=self.device)
        self.lib.dmfb_vec_get_blocks(self.h, _ptr(buf), C.byref(nb), self._stream())
        return buf[:, :nb.value]

    def get_state(self):
        E, n, dev = self.n_envs, self.n_agents, self.device
        pos = torch.empty((E, n, 2), dtype=torch.int32, device=dev)
        dist = torch.empty((E, n), dtype=torch.int32, device=dev)
        sc = torch.empty((E,), dtype=torch.int32, device=dev)
        cons = torch.empty((E,), dtype=torch.int64, device=dev)
        self.lib.dmfb_vec_get_state(self.h, _ptr(pos), _ptr(dist), _ptr(sc), _ptr(cons), self._stream())
        return {'pos': pos, 'dist': dist, 'step_count': sc, 'constraints': cons}

    def launch_shape(self):
        """Chips per workgroup of the launches the handle makes (include/dmfb_vec.h: dmfb_vec_launch_shape)."""
        out = self._launch_shape(6)
        return {'fused_tile': out[0], 'observe_tile': out[1], 'split_min_envs': out[2], 'step_only_tile': out[3],
                'observe_workgroups': out[4], 'observe_block': out[5]}

    def zoom_lut(self):
        out = np.zeros((2, 511), np.int8)
        self.lib.dmfb_vec_zoom_lut(self.h, out.ctypes.data_as(C.c_void_p))
        return out


class _RoutingManagerView:
    """What callers read from `env.routing_manager` in the reference (evaDegre.py:21 reads
    m_health; the golden harness assigns starts/ends and the maps)."""

    def __init__(self, env):
        self._env = env

    def _map(self, which):
        return self._env._vec.get_map(which)[0].cpu().numpy()

    m_health = property(lambda self: self._map('health'), lambda self, v: self._env._vec.set_map('health', v))
    m_usage = property(lambda self: self._map('usage'), lambda self, v: self._env._vec.set_map('usage', v))
    m_degrade = property(lambda self: self._map('degrade'), lambda self, v: self._env._vec.set_map('degrade', v))

    @property
    def starts(self):
        return self._env._vec.get_task()[0][0].cpu().numpy().astype(int)

    @property
    def ends(self):
        return self._env._vec.get_task()[1][0].cpu().numpy().astype(int)

    @property
    def distances(self):
        return self._env._vec.get_state()['dist'][0].cpu().numpy().astype(int)

    @property
    def blocks(self):
        """(x_min, x_max, y_min, y_max) per block, like the reference's Block objects (dmfb.py:34-41)."""
        return [tuple(int(v) for v in b) for b in self._env._vec.get_blocks()[0].cpu().numpy()]

    @blocks.setter
    def blocks(self, value):
        rows = [(b.x_min, b.x_max, b.y_min, b.y_max) if hasattr(b, 'x_min') else tuple(b) for b in value]
        self._env._vec.set_blocks(np.asarray(rows, np.int32).reshape(1, -1, 4))

    def set_task(self, starts, ends):
        """starts/ends assignment + restartforall (dmfb.py:185-190)."""
        self._env._vec.set_task(np.asarray(starts)[None], np.asarray(ends)[None])

    def getTaskStatus(self):
        return [bool(d == 0) for d in self.distances]

    def getglobalobs(self):
        """dmfb.py:368-391: int array (3, width, length)."""
        return self._env._vec.global_obs()[0].cpu().numpy().astype(int)


class DMFBenv:
    """Single-chip facade over the HIP path with the reference's protocol
    (env/DMFB/dmfb.py:474-640): same constructor, reset/step/restart/get_env_info, `.agents`,
    `.width/.length`, `.max_step`, `.routing_manager.m_health`.  One chip = a batch of one, so
    every call synchronises; use VecDMFB for throughput."""

    def __init__(self, width, length, n_agents, n_blocks=0, fov=5, stall=True, b_degrade=False,
                 per_degrade=0.1, show=False, savemp4=False, seed=0, with_maps=True, device=None):
        assert width >= 5 and length >= 5
        assert n_agents > 0
        if show or savemp4:
            raise NotImplementedError('rendering is out of scope (SURVEY.md section 2, rows 3-4)')
        self.agents = ['player_{}'.format(i) for i in range(n_agents)]
        self.possible_agents = self.agents[:]
        self.width, self.length = width, length
        self.max_step = (width + length) * 2
        self._vec = VecDMFB(width, length, n_agents, n_blocks, fov, stall, b_degrade, per_degrade, n_envs=1,
                            seed=seed, with_maps=with_maps, device=device)
        self.routing_manager = _RoutingManagerView(self)
        self.rewards = {i: 0. for i in self.agents}
        self.dones = {i: False for i in self.agents}
        self.step_count = 0
        self.constraints = 0

    def _obs_list(self, obs):
        o = obs[0].cpu().numpy()
        return [o[i].copy() for i in range(len(self.agents))]

    def step(self, actions, record=True):
        if isinstance(actions, dict):
            acts = [actions[a] for a in self.agents]
        elif isinstance(actions, list):
            acts = actions
        else:
            raise TypeError('wrong actions')
        if len(acts) != len(self.agents):
            raise RuntimeError('The number of actions is not the same as n_droplets')
        if any(int(a) < 0 or int(a) > 4 for a in acts):
            raise TypeError('action is illegal')
        obs, rewards, dones, info = self._vec.step(np.asarray(acts, np.int32)[None], record=record)
        r = rewards[0].cpu().numpy()
        d = dones[0].cpu().numpy()
        self.step_count += 1
        c = int(info['constraints'][0].item())
        self.constraints += c
        for k, a in enumerate(self.agents):
            self.rewards[a] = np.float64(r[k])
            self.dones[a] = bool(d[k])
        return self._obs_list(obs), self.rewards, self.dones, {'constraints': c, 'success': int(info['success'][0].item())}

    def reset(self, new=False):
        self.rewards = {i: 0 for i in self.agents}
        self.dones = {i: False for i in self.agents}
        self.step_count = 0
        self.constraints = 0
        return self._obs_list(self._vec.reset(new=new))

    def restart(self, index=None):
        self.rewards = {i: 0.0 for i in self.agents}
        self.dones = {i: False for i in self.agents}
        self.step_count = 0
        self.constraints = 0
        return self._obs_list(self._vec.restart())

    def getObs(self):
        return self._obs_list(self._vec.observe())

    def get_env_info(self):
        return self._vec.get_env_info()

    def seed(self, seed=None):
        pass

    def render(self, close=False):
        pass

    def close(self):
        pass
