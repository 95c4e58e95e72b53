"""Host side of the vectorised MEDA environment: `VecMEDA` drives E lock-step chips through the C
ABI in include/meda_vec.h (kernels in marl_dmfb_amd/csrc/meda_*.h*); `MEDAEnv` is the
reference-shaped single-chip facade (env/MEDA/meda.py:457-681).

Two deliberate differences from the reference, both stated by SURVEY.md 8(d)/(f3):
  * observations are int8 (the reference builds float64 arrays whose values are small integers);
    the facade widens them back to float64 so callers see the reference's dtype;
  * `get_env_info()['obs_shape']` of the facade is the reference's (an int, meda.py:676-681);
    `VecMEDA.get_env_info()` returns the tuple shape the networks need."""
import numpy as np
import torch

from .. import _lib
from ._vec import VecEnv, _ptr


class VecMEDA(VecEnv):
    """E independent MEDA chips advanced in lock-step on one MI355X (ctor of MEDAEnv, meda.py:469,
    plus n_envs / seed / env_id0 / with_maps).  step: MEDAEnv.step (meda.py:513-539) for all envs,
    info['constraints'] is `fail` (float64)."""
    LIB, NAME, CONSTRAINTS = 'meda_vec', 'VecMEDA', 'fail'
    STATE_LAYERS = 2   # droplet boxes, destination boxes: the project's own state (include/meda_vec.h), QMIX with --meda_state
    SHIELD_FLAG, N_ACTIONS = 'meda_shield', 9   # the action shield (_vec.py: shield; include/meda_vec.h: meda_vec_shield)

    def __init__(self, width, length, n_agents, n_blocks=0, fov=19, stall=True, b_degrade=False, per_degrade=0.1,
                 n_envs=1, seed=0, with_maps=False, env_id0=0, device=None, version=0):
        self.seed, self.env_id0 = int(seed), int(env_id0)
        self.width, self.length, self.n_agents, self.fov, self.n_envs = width, length, n_agents, fov, n_envs
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.cfg = _lib.MedaVecConfig(width, length, n_agents, fov, int(bool(b_degrade)), int(bool(with_maps)),
                                      float(per_degrade), n_envs, env_id0, seed, dev.index or 0, int(version))
        self.version = int(version)
        self.has_maps = bool(b_degrade or with_maps)
        self._create(dev)
        self.obs_len = (3 if self.version == 2 else 4) * fov * fov + 2
        self.max_step = width + length
        E, n, dev = n_envs, n_agents, self.device
        self.obs = torch.zeros((E, n, self.obs_len), dtype=torch.int8, device=dev)
        self.rewards = torch.zeros((E, n), dtype=torch.float64, device=dev)
        self.dones = torch.zeros((E, n), dtype=torch.uint8, device=dev)
        self.fail = torch.zeros((E,), dtype=torch.float64, device=dev)
        self.success = torch.zeros((E,), dtype=torch.uint8, device=dev)
        self.team_reward = torch.zeros((E,), dtype=torch.float64, device=dev)
        self.terminated = torch.zeros((E,), dtype=torch.uint8, device=dev)
        self._out = _lib.MedaVecStepOut(self.rewards.data_ptr(), self.dones.data_ptr(), self.fail.data_ptr(),
                                        self.success.data_ptr(), self.obs.data_ptr(), self.team_reward.data_ptr(),
                                        self.terminated.data_ptr())

    def get_env_info(self):
        return {'n_actions': 9, 'n_agents': self.n_agents,
                'obs_shape': (3 if self.version == 2 else 4, self.fov, self.fov, 2, self.obs_len),
                'episode_limit': self.max_step}

    def reset(self, mask=None, new=False, obs=None):
        obs = self.obs if obs is None else obs
        self.lib.meda_vec_reset(self.h, _ptr(self._mask(mask)), _ptr(obs), self._stream())
        return obs

    def launch_shape(self):
        """Chips per workgroup of the launches the handle makes (include/meda_vec.h: meda_vec_launch_shape)."""
        out = self._launch_shape(4)
        return {'step_tile': out[0], 'observe_tile': out[1], 'observe_block': out[2], 'observe_workgroups': out[3]}

    def get_state(self):
        E, n, dev = self.n_envs, self.n_agents, self.device
        pos = torch.empty((E, n, 2), dtype=torch.int32, device=dev)
        status = torch.empty((E, n), dtype=torch.uint8, device=dev)
        sc = torch.empty((E,), dtype=torch.int32, device=dev)
        failed = torch.empty((E,), dtype=torch.uint8, device=dev)
        self.lib.meda_vec_get_state(self.h, _ptr(pos), _ptr(status), _ptr(sc), _ptr(failed), self._stream())
        return {'pos': pos, 'status': status, 'step_count': sc, 'failed': failed}


class MEDAEnv:
    """Single-chip facade with the reference's protocol (env/MEDA/meda.py:457-681)."""
    VERSION = 0

    def __init__(self, w, l, n_agents, n_blocks=0, fov=19, stall=True, b_degrade=False, per_degrade=0.1, show=False,
                 savemp4=False, seed=0, device=None):
        assert w > 0 and l > 0
        assert n_agents > 0
        if show or savemp4:
            raise NotImplementedError('rendering is out of scope (SURVEY.md section 2, row 4)')
        self.agents = ['player_{}'.format(i) for i in range(n_agents)]
        self.possible_agents = self.agents[:]
        self.width, self.length, self.fov = w, l, fov
        self.max_step = w + l
        self._vec = VecMEDA(w, l, n_agents, fov=fov, b_degrade=b_degrade, per_degrade=per_degrade, n_envs=1, seed=seed,
                            with_maps=True, device=device, version=self.VERSION)
        self.rewards = {i: 0. for i in self.agents}
        self.dones = {i: False for i in self.agents}
        self.step_count = 0
        self.fails = 0

    m_health = property(lambda self: self._vec.get_map('health')[0].cpu().numpy(),
                        lambda self, v: self._vec.set_map('health', np.asarray(v)))
    m_usage = property(lambda self: self._vec.get_map('usage')[0].cpu().numpy(),
                       lambda self, v: self._vec.set_map('usage', np.asarray(v)))
    m_degrade = property(lambda self: self._vec.get_map('degrade')[0].cpu().numpy(),
                         lambda self, v: self._vec.set_map('degrade', np.asarray(v)))

    def _obs_list(self, obs):
        o = obs[0].cpu().numpy()
        if self.VERSION == 0:
            o = o.astype(np.float64)   # the base env returns float64 rows; v0_2 returns int8 (meda.py:860)
        return [o[i].copy() for i in range(len(self.agents))]

    def step(self, actions):
        acts = [actions[a] for a in self.agents] if isinstance(actions, dict) else list(actions)
        if len(acts) != len(self.agents):
            raise RuntimeError('The number of actions is not the same as n_droplets')
        obs, rewards, dones, info = self._vec.step(np.asarray(acts, np.int32)[None])
        r, d = rewards[0].cpu().numpy(), dones[0].cpu().numpy()
        self.step_count += 1
        fail = float(info['constraints'][0].item())
        self.fails += fail
        for k, a in enumerate(self.agents):
            self.rewards[a] = float(r[k])
            self.dones[a] = bool(d[k])
        return self._obs_list(obs), self.rewards, self.dones, {'constraints': fail, 'success': int(info['success'][0].item())}

    def reset(self):
        self.rewards = {i: 0. for i in self.agents}
        self.dones = {i: False for i in self.agents}
        self.step_count = 0
        self.fails = 0
        return self._obs_list(self._vec.reset())

    def restart(self, index=None):
        self.rewards = {i: 0. for i in self.agents}
        self.dones = {i: False for i in self.agents}
        self.step_count = 0
        return self._obs_list(self._vec.restart())

    def getObs(self):
        return self._obs_list(self._vec.observe())

    def get_env_info(self):
        return {'n_actions': 9, 'n_agents': len(self.agents), 'obs_shape': self._vec.obs_len,
                'episode_limit': self.max_step}

    def seed(self, seed=None):
        pass

    def render(self, close=False):
        pass

    def close(self):
        pass


class MEDAEnv_v0_2(MEDAEnv):
    """env/MEDA/meda.py:846-897: 3-layer int8 observation with the direction zoomed to 30x30."""
    VERSION = 2
