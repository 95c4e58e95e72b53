"""What `VecDMFB` and `VecMEDA` do identically: the handle's life cycle, episode control, the lock-step
transition, the map accessors and the observation-kernel timing, all through the checked view of the
library (marl_dmfb_amd._lib.checked), whose errors are the reference's exceptions.

A subclass sets LIB (the library's name, also the prefix of its functions), NAME, ACTIONS_FLAGS,
STEP_RECORD and STATE_LAYERS, builds self.cfg before calling `_create`, and allocates the step outputs."""
import ctypes as C

import numpy as np
import torch

from .. import _lib

MAPS = {'health': 0, 'usage': 1, 'degrade': 2}
ACT_I32, ACT_I8, ACT_I64 = 0, 16, 32
STEP_AUTORESET = 2


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class VecEnv:
    LIB = NAME = None
    STEP_RECORD = 0      # flag bit of `record` (0: the library has none)
    CONSTRAINTS = None   # attribute that info['constraints'] returns
    STATE_LAYERS = None  # layers of the global state QMIX mixes on, int8 [STATE_LAYERS][width][length] per chip
    SHIELD_FLAG = None   # the switch that plays this env under its action shield ('shield' for DMFB, 'meda_shield' for MEDA)
    N_ACTIONS = None     # actions per droplet: the width of a q row and of a one-hot row

    def _create(self, device):
        self.lib = _lib.checked(self.LIB)
        self._fn = {k[len(self.LIB) + 1:]: getattr(self.lib, k) for k in _lib.SIGNATURES[self.LIB]}
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('%s runs on the GPU only (no CPU fallback)' % self.NAME)
        self._fn['check_config'](C.byref(self.cfg))
        self.h = C.c_void_p()
        with torch.cuda.device(self.device):
            self._fn['create'](C.byref(self.cfg), self._stream(), C.byref(self.h))
        self.timing = None  # set to [] to collect (start, end) HIP event pairs around every step launch

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, 'h', None) is not None and self.h:
            self._fn['destroy'](self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def state_bytes(self):
        return int(self._fn['state_bytes'](self.h))

    def _dev(self, a, dtype):
        if a is None:
            return None
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a))
        return t.to(device=self.device, dtype=dtype).contiguous()

    def _mask(self, mask):
        return self._dev(mask, torch.uint8)

    # ------------------------------------------------------------------ episode control
    def restart(self, mask=None, obs=None):
        obs = self.obs if obs is None else obs
        self._fn['restart'](self.h, _ptr(self._mask(mask)), _ptr(obs), self._stream())
        return obs

    def set_task(self, starts, ends):
        s = self._dev(starts, torch.int32).reshape(self.n_envs, self.n_agents, 2)
        e = self._dev(ends, torch.int32).reshape(self.n_envs, self.n_agents, 2)
        self._fn['set_task'](self.h, _ptr(s), _ptr(e), self._stream())

    def get_task(self):
        s = torch.empty((self.n_envs, self.n_agents, 2), dtype=torch.int32, device=self.device)
        e = torch.empty_like(s)
        self._fn['get_task'](self.h, _ptr(s), _ptr(e), self._stream())
        return s, e

    # ------------------------------------------------------------------ transition
    def step(self, actions, uniforms=None, record=True, autoreset=False, active=None, out=None):
        """The reference's step for all envs.  `actions`: int8/int32/int64 tensor [E, n] on the device (or
        anything array-like); `active` (uint8/bool [E], optional) freezes the envs whose entry is 0.  Returns
        (obs, rewards, dones, info) as device tensors that are REUSED by the next call;
        info = dict(constraints, success, team_reward, terminated)."""
        if not isinstance(actions, torch.Tensor) or actions.device != self.device:
            actions = self._dev(actions, torch.int32)
        flag = {torch.int64: ACT_I64, torch.int8: ACT_I8, torch.int32: ACT_I32}.get(actions.dtype)
        if flag is None:
            actions, flag = actions.to(torch.int32), ACT_I32
        actions = actions.contiguous()
        if actions.numel() != self.n_envs * self.n_agents:
            raise RuntimeError('The number of actions is not the same as n_droplets')  # dmfb.py:272-274, meda.py:242-244
        u = self._dev(uniforms, torch.float64)
        flags = flag | (self.STEP_RECORD if record else 0) | (STEP_AUTORESET if autoreset else 0)
        act = self._mask(active)
        if self.timing is not None:  # bench.py: HIP events on the launch stream around the kernel
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        self._fn['step'](self.h, _ptr(actions), _ptr(u), _ptr(act), flags, C.byref(out or self._out), self._stream())
        if self.timing is not None:
            ev1.record()
            self.timing.append((ev0, ev1))
        info = {'constraints': getattr(self, self.CONSTRAINTS), 'success': self.success, 'team_reward': self.team_reward,
                'terminated': self.terminated}
        return self.obs, self.rewards, self.dones, info

    def observe(self, mask=None, obs=None):
        obs = self.obs if obs is None else obs
        self._fn['observe'](self.h, _ptr(self._mask(mask)), _ptr(obs), self._stream())
        return obs

    # ------------------------------------------------------------------ global state (QMIX)
    @property
    def state_shape(self):
        """Length of the flattened global state (STATE_LAYERS * width * length, *_state_len): what QMIX's mixer reads as
        args.state_shape.  Not part of get_env_info(), whose dict is the reference's (its 'state_shape' is commented out,
        dmfb.py:637)."""
        return self.STATE_LAYERS * self.width * self.length

    def global_obs(self, mask=None, out=None):
        """The global state of every chip: int8 (E, STATE_LAYERS, width, length) on the device (*_global_obs; DMFB:
        routing_manager.getglobalobs(), dmfb.py:368-391); rows of chips whose mask entry is 0 are left as they are in `out`."""
        if out is None:
            out = torch.zeros((self.n_envs, self.STATE_LAYERS, self.width, self.length), dtype=torch.int8, device=self.device)
        self._fn['global_obs'](self.h, _ptr(self._mask(mask)), _ptr(out), self._stream())
        return out

    def global_obs_append(self, alive, terminated, t, s, s_next):
        """The state appends of lock-step t of a recorded episode (*_global_obs_append): s_next[:, t] of the chips alive before
        the step, s[:, t + 1] of those that also did not terminate.  s / s_next: int8 (E, T, state)."""
        self._fn['global_obs_append'](self.h, _ptr(alive), _ptr(terminated), int(t), int(s.shape[1]), _ptr(s), _ptr(s_next),
                                      self._stream())

    def global_obs_stage_first(self, mask, stage):
        """stage[e, 0] = the state of every chip whose mask entry is set (all when mask is None): the first state of the episodes
        the continuous rollout starts (*_global_obs_stage_first).  stage: int8 (E, T + 1, state)."""
        self._fn['global_obs_stage_first'](self.h, _ptr(self._mask(mask)), int(stage.shape[1]) - 1, _ptr(stage), self._stream())

    def global_obs_stage_close(self, t_ep, close_slot, stage, ring_states):
        """stage[e, t_ep[e] + 1] = the state of chip e, then the staged rows of the chips whose close_slot is set copied into their
        slots of ring_states, int8 (slots, T + 1, state), rows past the episode zeroed (*_global_obs_stage_close).  t_ep /
        close_slot: int32 (E,) as rollout_stream_step leaves them."""
        self._fn['global_obs_stage_close'](self.h, _ptr(t_ep), _ptr(close_slot), int(stage.shape[1]) - 1, _ptr(stage),
                                           _ptr(ring_states), int(ring_states.shape[0]), self._stream())

    # ------------------------------------------------------------------ route record
    def route_append(self, t, T, route):
        """route[:, t + 1] = every chip's droplet positions now (t == -1: slot 0), route uint8 (E, T + 1, n, 2) on the device
        (*_route_append: DMFB (x, y), MEDA (x_center, y_center))."""
        self._fn['route_append'](self.h, int(t), int(T), _ptr(route), self._stream())

    # ------------------------------------------------------------------ action shield
    def shield(self, q, actions, last_action, ep_u=None, ep_onehot=None, t=0, t_ep=None, active=None, overrides=None,
               unsafe=None):
        """Between the pick and `step`: every pick that could break a constraint is replaced, in place, by that droplet's best-Q
        action that cannot (*_shield; the rule: marl_dmfb_amd.shield.shield_reference for DMFB, meda_shield_reference for
        MEDA).  With A = N_ACTIONS: q float32 (E, n, A); actions int32 (E, n) in/out; last_action int8 (E, n, A) gets the one-hot
        rows; ep_u int8 (E, T, n[, 1]) / ep_onehot int8 (E, T, n, A) get slot t (t_ep int32 (E,): every chip its own slot) too;
        chips whose `active` byte is 0 are not touched; overrides int32 (E,) += the changed picks, unsafe uint8 (E,) = 1 where
        the chip was not safe before the step.  The tensors are written through, so they must be contiguous device tensors of
        exactly these types."""
        E, n, A = self.n_envs, self.n_agents, self.N_ACTIONS

        def need(name, x, dtype, numel):
            if x is None:
                return
            if not isinstance(x, torch.Tensor) or x.device != self.device or x.dtype != dtype or not x.is_contiguous():
                raise TypeError('shield: %s must be a contiguous %s tensor on %s' % (name, dtype, self.device))
            if x.numel() != numel:
                raise ValueError('shield: %s has %d elements, expected %d' % (name, x.numel(), numel))
        if (ep_u is None) != (ep_onehot is None):
            raise ValueError('shield: ep_u and ep_onehot go together')
        T = int(ep_u.shape[1]) if ep_u is not None else 0
        need('q', q, torch.float32, E * n * A)
        need('actions', actions, torch.int32, E * n)
        need('last_action', last_action, torch.int8, E * n * A)
        need('ep_u', ep_u, torch.int8, E * T * n)
        need('ep_onehot', ep_onehot, torch.int8, E * T * n * A)
        need('t_ep', t_ep, torch.int32, E)
        need('overrides', overrides, torch.int32, E)
        need('unsafe', unsafe, torch.uint8, E)
        self._fn['shield'](self.h, _ptr(q), _ptr(self._mask(active)), _ptr(actions), _ptr(last_action), _ptr(ep_u),
                           _ptr(ep_onehot), T, int(t), _ptr(t_ep), _ptr(overrides), _ptr(unsafe), self._stream())
        return actions

    # ------------------------------------------------------------------ introspection
    def get_map(self, which):
        buf = torch.empty((self.n_envs, self.width, self.length), dtype=torch.float64, device=self.device)
        self._fn['get_map'](self.h, MAPS[which], _ptr(buf), self._stream())
        return buf

    def set_map(self, which, arr):
        t = self._dev(arr, torch.float64).expand(self.n_envs, self.width, self.length).contiguous()
        self._fn['set_map'](self.h, MAPS[which], _ptr(t), self._stream())

    def _launch_shape(self, n):
        out = (C.c_int32 * n)()
        self._fn['launch_shape'](self.h, C.byref(out))
        return out

    def observe_timing(self, enable):
        """Start/stop collecting the dispatch time stamps of the observation kernel (*_observe_timing)."""
        self._fn['observe_timing'](self.h, int(bool(enable)))

    def observe_timing_read(self):
        """(summed kernel duration in microseconds, launches) since the last read; synchronises the host."""
        us, n = C.c_double(0.0), C.c_int(0)
        self._fn['observe_timing_read'](self.h, C.byref(us), C.byref(n))
        return us.value, n.value
