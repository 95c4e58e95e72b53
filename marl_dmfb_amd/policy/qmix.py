"""QMIX learner with the reference's API surface (policy/qmix.py): QMIX(args) with .learn(batch, max_episode_len, train_step,
epsilon=None), .get_q_values, .init_hidden, .eval_rnn / .target_rnn, .eval_qmix_net / .target_qmix_net, .save_model.

The agent network, its inputs (observation + last action, no agent-id one-hot) and its kernels are VDN's (policy/vdn.py, whose
learner this one extends), so `rnn_net_params.pkl` files of the two algorithms are interchangeable.  What differs is the mixer
(network/qmix_net.py), conditioned on the global state `s` / `s_next` the rollout records (include/dmfb_vec.h: getglobalobs;
include/meda_vec.h: the project's MEDA state, opted into with args.meda_state),
and the TD rule of policy/qmix.py:104-122:
    q_tot_eval = QMixNet(q_evals gathered by u, s);  q_tot_target = QMixNet(max over available actions of q_targets, s_next)
    targets = r + gamma * q_tot_target * (1 - terminated);  td = q_tot_eval - targets.detach()
    loss = sum((mask * td) ** 2) / sum(mask)
followed by VDN's clip + Adam step and hard target sync (network and mixer) every target_update_cycle learns.

On the GPU, with replay-ring tensors, the four hypernetwork first layers are one GEMM per network against their concatenated
[F][S] weight and everything after it (second layers, abs, the two bmm's, ELU, the target's max, TD, mask) is ONE HIP launch each
way (include/qmix_ops.h); the loss is differentiated un-normalised and divided by the mask count inside the clip + Adam kernel,
as VDN does, so the data-parallel path is unchanged.  The CPU, `two_hyper_layers=False` and other batches take the torch-op path
through QMixNet.

With args.qmix_lambda (--qmix_lambda, in [0, 1], default 0) the targets are the episodes' lambda-returns (policy/td_lambda.py, the
rule of VDN's --td_lambda with the mixers in the place of the sums): on the fused paths the mixing kernel leaves the two q_tot of
every row and a second launch walks the episodes (include/qmix_lambda.h); the torch-op path walks in torch ops.

With args.qmix_packed (--qmix_packed, continuous rollout only) `learn_packed` learns on the VALID steps of the drawn episodes, as
VDN.learn_packed does: the agent networks run on the packed units (VDN._packed_q_values), the state rows of those units are
fetched from the ring by index (include/qmix_packed.h: qmix_gather_states), and the same mixing + TD kernels run per unit.

With args.qmix_double_q (--qmix_double_q, default off, read at learn time) each agent's value that goes into the TARGET mixer is a
double-Q value (policy/double_q.py): the eval network one step ahead picks the action, the target network values it.  The fused
paths pass the selector to the mixing kernel (include/qmix_double.h); the selector, its extra step behind an episode and the
`double_picks` diagnostics are VDN's.  It composes with qmix_lambda and qmix_packed; args.double_q stays VDN's knob."""
import torch
import torch.nn.functional as F

from ..network.qmix_net import QMixNet
from .vdn import VDN, _episode_slots, _t


def _mixer(second_layers):
    """include/qmix_ops.h: qmix_mixer, the six second-layer tensors of one mixer."""
    from .. import _lib
    return _lib.QmixMixer(*[t.data_ptr() for t in second_layers])


def _mix_forward(ctx, rows, dev, entry, head, bad, lam, lam_tail=(), sel=None):
    """Forward tail of the two nodes: `entry` is the one-step entry point's name and `head` its arguments up to gamma.  With
    lam != 0 the call goes to the entry point's lambda form (include/qmix_lambda.h: 'qmix_mix_td_lambda_' + the rest of the name),
    which takes lam, the two q_tot scratch tensors (the hand-off between its two launches) and a NULL d_targets behind the
    counter, then `lam_tail` (packed form: n_steps, counts).  sel = (what the double-Q entry point of the form takes from d_q_sel
    up to d_picks' place, n_agents, picks list or None): with it the call goes to include/qmix_double.h ('qmix_mix_td_double_' +
    the rest of the name), lam passed through (the scratch tensors only when lam != 0), and the picks (rows, n_agents) int8 are
    appended to the list -> mtd, mask, num, mask.sum()."""
    from .. import _lib
    mtd = torch.empty(rows, dtype=torch.float32, device=dev)
    mask = torch.empty(rows, dtype=torch.float32, device=dev)
    out = (mtd.data_ptr(), mask.data_ptr(), None if bad is None else bad.data_ptr())
    stream = torch.cuda.current_stream(dev).cuda_stream
    if sel is not None:
        sel_args, n, picks_out = sel
        picks = None if picks_out is None else torch.empty((rows, n), dtype=torch.int8, device=dev)
        tot = torch.empty((2, rows), dtype=torch.float32, device=dev) if lam else None
        getattr(_lib.checked('qmix_double'), entry.replace('qmix_mix_td_', 'qmix_mix_td_double_'))(
            *head, *out, float(lam), None if tot is None else tot[0].data_ptr(), None if tot is None else tot[1].data_ptr(), None,
            *lam_tail, *sel_args, None if picks is None else picks.data_ptr(), stream)
        if picks is not None:
            picks_out.append(picks)
    elif lam:
        tot = torch.empty((2, rows), dtype=torch.float32, device=dev)
        getattr(_lib.checked('qmix_lambda'), entry.replace('qmix_mix_td_', 'qmix_mix_td_lambda_'))(
            *head, *out, float(lam), tot[0].data_ptr(), tot[1].data_ptr(), None, *lam_tail, stream)
    else:
        getattr(_lib.checked('qmix_packed' if entry.endswith('_packed') else 'qmix_ops'), entry)(*head, *out, stream)
    num, mask_sum = (mtd * mtd).sum(), mask.sum()
    ctx.mark_non_differentiable(mask_sum)
    return mtd, mask, num, mask_sum


def _mix_backward(rows, n, H, M, g_num, gq, gp, launch, wide=False):
    """Backward tail of the two nodes: launch(g, z, x) has the kernel write gq, gp and the per-row factors z / x; the second-layer
    weight + bias gradients are GEMMs over those (deterministic; x carries a ones column per factor) -> the eight gradients.
    wide (the lambda learn): the hyper_b2[2] product, whose left factor is the single column g = d num / d q_tot, is accumulated in
    float64.  It is a plain reduction of signed TD errors over every row of the batch (its bias entry is sum(g)); on lambda-returns
    the float32 GEMM's summation order alone moved that one number by two float32 steps (profiles/qmix_lambda/NOTES.md).  33 rows-long
    dot products: the cost is three small launches.  The one-step learn keeps its float32 product and its bits."""
    nM = n * M
    z = torch.empty((rows, nM + M + 1), dtype=torch.float32, device=gq.device)
    x = torch.empty((rows, 2 * H + M + 3), dtype=torch.float32, device=gq.device)
    g = g_num.reshape(1).to(torch.float32).contiguous()
    launch(g.data_ptr(), z.data_ptr(), x.data_ptr())
    g1 = z[:, :nM].t().mm(x[:, :H + 1])
    g2 = z[:, nM:nM + M].t().mm(x[:, H + 1:2 * H + 2])
    zb, xb = z[:, nM + M:], x[:, 2 * H + 2:]
    g3 = zb.double().t().mm(xb.double()).float() if wide else zb.t().mm(xb)
    return gq, gp, g1[:, :H], g1[:, H], g2[:, :H], g2[:, H], g3[:, :M], g3[:, M]


class _MixTD(torch.autograd.Function):
    """qmix_mix_td_forward / _backward (include/qmix_ops.h): (time-major Q values of both networks, the first-layer outputs P of
    both mixers, the eval mixer's second-layer weights, the replay tensors) -> num = sum(mtd ** 2), mask.sum().  Gradients for the
    eval Q values, the eval P and the eval second-layer weights.  lam > 0: the targets are the episodes' lambda-returns
    (include/qmix_lambda.h), two launches forward; the backward is the same.  q_sel (time-major like q_t, no gradient): double-Q
    targets (include/qmix_double.h), the selector picks and the target network values; picks: a list that then receives the (B*T, n)
    int8 picks."""

    @staticmethod
    def forward(ctx, q_e, p_e, w1, b1, w2, b2, wb, bb, q_t, p_t, tgt, u, r, avail_next, terminated, padded, dims, gamma, bad, lam=0.0,
                q_sel=None, picks=None):
        B, T, n, A, H, M, pe_rows, pe_off, pt_rows, pt_off = dims
        t_limit = _episode_slots(u)
        q_e, q_t = q_e.contiguous(), q_t.contiguous()
        head = [q_e.data_ptr(), q_t.data_ptr(), u.data_ptr(), r.data_ptr(), avail_next.data_ptr(), terminated.data_ptr(), padded.data_ptr(),
                B, T, t_limit, n, A, p_e.data_ptr(), pe_rows, pe_off, p_t.data_ptr(), pt_rows, pt_off, H, M,
                _mixer((w1, b1, w2, b2, wb, bb)), _mixer(tgt), float(gamma)]
        sel = None
        if q_sel is not None:
            q_sel = q_sel.contiguous()
            sel = ((q_sel.data_ptr(),), n, picks)
        mtd, mask, num, mask_sum = _mix_forward(ctx, B * T, u.device, 'qmix_mix_td_forward', head, bad, lam, (), sel)
        ctx.save_for_backward(mtd, mask, q_e, p_e, u, w1, b1, w2, b2, wb, bb)
        ctx.dims = (B, T, t_limit, n, A, H, M, pe_rows, pe_off)
        ctx.wide = bool(lam)
        return num, mask_sum

    @staticmethod
    def backward(ctx, g_num, _g_mask):
        from .. import _lib
        lib = _lib.checked('qmix_ops')
        mtd, mask, q_e, p_e, u, w1, b1, w2, b2, wb, bb = ctx.saved_tensors
        B, T, t_limit, n, A, H, M, pe_rows, pe_off = ctx.dims
        dev = u.device
        gq = torch.empty((T, B * n, A), dtype=torch.float32, device=dev)
        # rows of P outside steps 0..T-1 (the extra state slot of the ring layout) get no gradient
        gp = (torch.empty_like if pe_rows == T else torch.zeros_like)(p_e)
        return _mix_backward(B * T, n, H, M, g_num, gq, gp, lambda g, z, x: lib.qmix_mix_td_backward(
            mtd.data_ptr(), mask.data_ptr(), q_e.data_ptr(), u.data_ptr(), B, T, t_limit, n, A, p_e.data_ptr(), pe_rows, pe_off, H, M,
            _mixer((w1, b1, w2, b2, wb, bb)), g, gq.data_ptr(), gp.data_ptr(), z, x, torch.cuda.current_stream(dev).cuda_stream), ctx.wide) + (None,) * 14


class _MixTDPacked(torch.autograd.Function):
    """`_MixTD` on packed (episode, step) units (include/qmix_packed.h): q_e / q_t hold the valid steps of the length-sorted batch
    (rows j*n .. of unit j), p_e the eval mixer's first-layer rows of the units, p_t the target mixer's rows of the gathered
    states with `target_row` naming each unit's; the replay tensors are indexed in place through `units`.  Same outputs and
    gradients as `_MixTD`.  lam > 0: lambda-returns (include/qmix_lambda.h); `counts` is then the host list of units per step that
    laid the units out (VDN.pack_units).  q_sel (units of n x A rows, no gradient) with sel_units (device int32, unit j -> its
    selector unit): double-Q targets (include/qmix_double.h); picks: a list that then receives the (n_units, n) int8 picks."""

    @staticmethod
    def forward(ctx, q_e, p_e, w1, b1, w2, b2, wb, bb, q_t, p_t, tgt, units, n_units, target_row, u, r, avail_next, terminated,
                padded, dims, gamma, bad, lam=0.0, counts=None, q_sel=None, sel_units=None, picks=None):
        import ctypes as C
        n, A, H, M = dims
        steps = [int(c) for c in counts] if lam else []
        q_e, q_t, p_e, p_t = q_e.contiguous(), q_t.contiguous(), p_e.contiguous(), p_t.contiguous()
        head = [q_e.data_ptr(), q_t.data_ptr(), units.data_ptr(), n_units, u.data_ptr(), r.data_ptr(), avail_next.data_ptr(),
                terminated.data_ptr(), padded.data_ptr(), n, A, p_e.data_ptr(), p_t.data_ptr(), target_row.data_ptr(), H, M,
                _mixer((w1, b1, w2, b2, wb, bb)), _mixer(tgt), float(gamma)]
        sel = None
        if q_sel is not None:
            q_sel = q_sel.contiguous()
            sel = ((q_sel.data_ptr(), q_sel.shape[0] // n, None if sel_units is None else sel_units.data_ptr()), n, picks)
        mtd, mask, num, mask_sum = _mix_forward(ctx, n_units, u.device, 'qmix_mix_td_forward_packed', head, bad, lam,
                                                (len(steps), (C.c_int32 * len(steps))(*steps)), sel)
        ctx.save_for_backward(mtd, mask, q_e, p_e, units, u, w1, b1, w2, b2, wb, bb)
        ctx.dims = (n_units, n, A, H, M)
        ctx.wide = bool(lam)
        return num, mask_sum

    @staticmethod
    def backward(ctx, g_num, _g_mask):
        from .. import _lib
        lib = _lib.checked('qmix_packed')
        mtd, mask, q_e, p_e, units, u, w1, b1, w2, b2, wb, bb = ctx.saved_tensors
        U, n, A, H, M = ctx.dims
        dev = u.device
        gq = torch.empty((q_e.shape[0], A), dtype=torch.float32, device=dev)   # the kernel writes the zero padding rows as well
        gp = torch.empty_like(p_e)
        return _mix_backward(U, n, H, M, g_num, gq, gp, lambda g, z, x: lib.qmix_mix_td_backward_packed(
            mtd.data_ptr(), mask.data_ptr(), q_e.data_ptr(), units.data_ptr(), U, u.data_ptr(), n, A, q_e.shape[0], p_e.data_ptr(), H, M,
            _mixer((w1, b1, w2, b2, wb, bb)), g, gq.data_ptr(), gp.data_ptr(), z, x, torch.cuda.current_stream(dev).cuda_stream), ctx.wide) + (None,) * 19


class QMIX(VDN):
    MIXER = 'qmix'
    needs_state = True   # the rollout records s / s_next, the replay buffer stores them (args.alg == 'qmix')

    def __init__(self, args):
        name = getattr(args, 'name', 'dmfb')
        if name == 'meda' and not getattr(args, 'meda_state', False):
            raise ValueError("QMIX needs a global state, and the reference's MEDA env defines none (MEDA has no getglobalobs): "
                             "set args.meda_state (--meda_state) for the project's MEDA state (include/meda_vec.h), or use "
                             "alg='vdn'")
        if name not in ('dmfb', 'meda'):
            raise ValueError("QMIX needs a global state, which env %r does not provide: use alg='vdn'" % name)
        if getattr(args, 'state_shape', None) is None:
            raise ValueError('QMIX needs args.state_shape (the flattened global state, env.state_shape: 3 * width * length on DMFB, '
                             '2 * width * length on MEDA); set it from the env')
        if getattr(args, 'td_lambda', 0.0):
            raise ValueError('args.td_lambda (--td_lambda) = %r: lambda-returns are VDN-only; the QMIX target lives inside the fused '
                             'mixing block (include/qmix_ops.h).  Use td_lambda 0 or alg=\'vdn\'' % (args.td_lambda,))
        if getattr(args, 'double_q', False):
            raise ValueError('args.double_q (--double_q): double-Q targets are VDN-only; the QMIX target lives inside the fused mixing '
                             'block (include/qmix_ops.h).  Use double_q False or alg=\'vdn\'')
        super().__init__(args)
        self._mix_bad = None

    def _build_mixers(self, args):
        self.eval_qmix_net = QMixNet(args)
        self.target_qmix_net = QMixNet(args)

    def packed_ok(self, buffers):
        """learn_packed is opt-in (args.qmix_packed).  With the flag it applies where VDN's agent-network half does
        (VDN._packed_front_ok), within the fused block's limits (`_mix_fused_ok`), on a ring whose s / s_next are the two views of
        one contiguous int8 (slots, T + 1, S) tensor (common/replay_buffer.py) with int32 row ids."""
        if not getattr(self.args, 'qmix_packed', False) or not self._packed_front_ok(buffers):
            return False
        s, s_next, o = buffers.get('s'), buffers.get('s_next'), buffers['o']
        if not (isinstance(s, torch.Tensor) and isinstance(s_next, torch.Tensor) and s.dim() == 3):
            return False
        slots, T, S = o.shape[0], o.shape[1], s.shape[-1]
        ring = (s.is_cuda and s.dtype == torch.int8 and s_next.dtype == torch.int8 and tuple(s.shape) == (slots, T, S)
                and s_next.shape == s.shape and s.stride() == ((T + 1) * S, S, 1) and s_next.stride() == s.stride()
                and s_next.data_ptr() == s.data_ptr() + S)
        return bool(ring and self._mixer_limits_ok(self.n_actions) and slots * (T + 1) < 2 ** 31)

    def _mixer_limits_ok(self, n_actions):
        """The build limits of the fused mixing block (include/qmix_ops.h), and the switch that turns it off."""
        a = self.args
        return bool(a.two_hyper_layers and a.qmix_hidden_dim == 32 and a.hyper_hidden_dim in (24, 32) and self.n_agents <= 16
                    and n_actions <= 16 and getattr(a, 'fused_mix', True))

    @staticmethod
    def pack_state_rows(idx, lens, counts, t_ring):
        """Host side of learn_packed, beside VDN.pack_units: the state rows of a length-sorted draw in the ring's
        (slots * (t_ring + 1), S) state tensor -> (rows int32[U + B], target_row int32[U]).  off[t] = counts[:t].sum(); unit
        j = off[t] + k (episode k at step t) reads s[t] = rows[j] = idx[k] * (t_ring + 1) + t; the closing state of episode k is
        rows[U + k] = idx[k] * (t_ring + 1) + lens[k].  s_next of unit j is s[t + 1] of the same episode (a valid step,
        common/replay_buffer.py): target_row[j] = off[t + 1] + k where the episode goes on, else U + k."""
        import numpy as np
        idx, lens, counts = np.asarray(idx, np.int64), np.asarray(lens, np.int64), np.asarray(counts, np.int64)
        off = np.concatenate([[0], np.cumsum(counts)])
        U, base = int(off[-1]), idx * (t_ring + 1)
        rows, target_row = np.empty(U + len(idx), np.int64), np.empty(U, np.int64)
        for t, c in enumerate(counts):
            k = np.arange(c)
            rows[off[t]:off[t] + c] = base[:c] + t
            target_row[off[t]:off[t] + c] = np.where(lens[:c] > t + 1, off[t + 1] + k, U + k)
        rows[U:] = base + lens
        return rows.astype(np.int32), target_row.astype(np.int32)

    def learn_packed(self, buffers, idx, lens, train_step, plan=None):
        """QMIX.learn on the episodes in slots `idx` of the replay ring WITHOUT their padded steps (see VDN.learn_packed; idx / lens
        sorted by length, longest first).  plan: (counts, units, rows, target_row) with the three lists already on the device.

        With double-Q targets (args.qmix_double_q) the selector tensor is VDN's (VDN._learn_packed_double): the U units of q_eval,
        detached, then one more eval step behind every episode's last unit.  Unit (e, t) selects with unit (e, t + 1) where the episode
        goes on and with tail unit U + e otherwise: element for element the `target_row` list, which is therefore the selector list
        too.  The one new upload is the B last units (double_q.selector_units): part of the single copy without a plan, one small
        copy of its own when the caller brings the plan."""
        import numpy as np
        a, dev, n, A = self.args, self.device, self.n_agents, self.n_actions
        B, T_ring = len(idx), buffers['o'].shape[1]
        double = self._double_q()
        last = None
        if plan is None:   # the unit list, the state rows and the target rows go up in ONE copy
            counts, units_np = self.pack_units(idx, lens, T_ring)
            rows_np, target_np = self.pack_state_rows(idx, lens, counts, T_ring)
            U = len(units_np)
            parts = [units_np, rows_np, target_np]
            if double:
                from .double_q import selector_units
                parts.append(selector_units(counts)[1])
            lists = torch.from_numpy(np.concatenate(parts)).to(dev, non_blocking=True)
            units, rows, target_row = lists[:U], lists[U:2 * U + B], lists[2 * U + B:3 * U + B]
            if double:
                last = lists[3 * U + B:]
        else:
            counts, units, rows, target_row = plan
            if double:
                from .double_q import selector_units
                last = torch.from_numpy(selector_units(counts)[1]).to(dev, non_blocking=True)
        sel = ()
        if double:
            q_e, q_t, units, U, (hs_e, obs_next, oh_next) = self._packed_q_values(buffers, B, (counts, units), eval_state=True)
            unit_rows = (last.long().unsqueeze(1) * n + torch.arange(n, device=dev)).view(-1)   # the n rows of every episode's last unit
            q_tail = self._eval_tail(obs_next.index_select(0, unit_rows), oh_next.index_select(0, unit_rows),
                                     hs_e.index_select(0, unit_rows))
            picks = None if self.double_picks is None else []
            sel = (torch.cat([q_e.detach()[:U * n], q_tail], dim=0), target_row, picks)
        else:
            q_e, q_t, units, U = self._packed_q_values(buffers, B, (counts, units))
        from .. import _lib
        s = buffers['s']
        states = torch.empty((U + B, s.shape[-1]), dtype=torch.float32, device=dev)
        _lib.checked('qmix_packed').qmix_gather_states(s.data_ptr(), s.shape[0] * (T_ring + 1), s.shape[-1], rows.data_ptr(), U + B,
                                                       states.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        p_e = self._first_layers(self.eval_qmix_net, states[:U])
        with torch.no_grad():
            p_t = self._first_layers(self.target_qmix_net, states)
        tgt = tuple(t.detach() for t in self.target_qmix_net.second_layers())
        num, mask_sum = _MixTDPacked.apply(q_e, p_e, *self.eval_qmix_net.second_layers(), q_t, p_t, tgt, units, U, target_row,
                                           buffers['u'], buffers['r'], buffers['avail_u_next'], buffers['terminated'],
                                           buffers['padded'], (n, A, a.hyper_hidden_dim, a.qmix_hidden_dim), a.gamma,
                                           self._bad_counter('_mix_bad'), self._td_lambda(), counts, *sel)
        if double and picks:
            self.double_picks.append(self._picks_by_episode(picks[0], counts))
        return self._backward_and_step(num, mask_sum, train_step)

    @staticmethod
    def _first_layers(net, rows):
        """The four hypernetwork first layers as ONE GEMM against the concatenated [F][S] weight (include/qmix_ops.h: P)."""
        layers = net.first_layers()
        return F.linear(rows, torch.cat([m.weight for m in layers]), torch.cat([m.bias for m in layers]))

    def _td_fused_ok(self, batch):
        return False

    # ------------------------------------------------------------------ learn (policy/qmix.py:79-128)
    def learn(self, batch, max_episode_len, train_step, epsilon=None):
        T = max_episode_len
        if getattr(self.args, 'qmix_packed', False):
            raise RuntimeError('args.qmix_packed (--qmix_packed) is set, but the padded learn was asked for: the packed learn does not '
                               'apply to this run (QMIX.packed_ok: the continuous rollout\'s replay ring on the GPU, a HIP front end, '
                               'two hypernetwork layers, qmix_hidden_dim 32, hyper_hidden_dim 24 or 32, at most 16 droplets and actions)')
        self.init_hidden(batch['o'].shape[0])
        if self._mix_fused_ok(batch):
            if not self._double_q():
                q_e, q_t = self.get_q_values(batch, T, time_major=True)
                num, mask_sum = self._mix_td_fused(q_e, q_t, batch, T)
                return self._backward_and_step(num, mask_sum, train_step)
            # double-Q targets (policy/double_q.py): the selector of step t is the eval network at input t + 1, detached
            q_e, q_t, q_tail = self.get_q_values(batch, T, time_major=True, tail=True)
            q_sel = torch.cat([q_e.detach()[1:], q_tail.unsqueeze(0)], dim=0)
            picks = None if self.double_picks is None else []
            num, mask_sum = self._mix_td_fused(q_e, q_t, batch, T, q_sel, picks)
            if picks:
                self.double_picks.append(picks[0].view(batch['u'].shape[0], T, self.n_agents))
            return self._backward_and_step(num, mask_sum, train_step)
        return self._learn_tensor_ops(batch, T, train_step)

    def _q_totals(self, q_evals, q_targets, batch, T):
        """The mixers of policy/qmix.py:112-113 on the global states of the steps and of their successors."""
        s = _t(batch['s'], self.device, torch.float32)[:, :T]
        s_next = _t(batch['s_next'], self.device, torch.float32)[:, :T]
        with torch.no_grad():
            q_total_target = self.target_qmix_net(q_targets, s_next)
        return self.eval_qmix_net(q_evals, s), q_total_target

    def _td_lambda(self):
        """args.qmix_lambda, read at learn time (0 = the reference's one-step targets; an args without the attribute is 0).
        args.td_lambda stays VDN's knob (__init__ refuses it)."""
        from .td_lambda import check_lambda
        return check_lambda(getattr(self.args, 'qmix_lambda', 0.0), 'qmix_lambda')

    def _double_q(self):
        """args.qmix_double_q, read at learn time (an args without the attribute is off).  args.double_q stays VDN's knob: __init__
        refuses it, and every learn refuses it if it was set later."""
        if getattr(self.args, 'double_q', False):
            raise ValueError('args.double_q (--double_q): double-Q targets are VDN-only; QMIX\'s knob is args.qmix_double_q '
                             '(--qmix_double_q)')
        return bool(getattr(self.args, 'qmix_double_q', False))

    def _mix_fused_ok(self, batch):
        """The fused block applies to replay-buffer tensors on the GPU (the dtypes ReplayBuffer stores), the CRNN's time-major
        sequence path, two hypernetwork layers and the kernel's build limits (include/qmix_ops.h)."""
        return (self._replay_layout_ok(batch, states=('s', 's_next')) and hasattr(self.eval_rnn, 'recurrent_seq')
                and self._mixer_limits_ok(batch['avail_u_next'].shape[3]))

    @staticmethod
    def _state_rows(s, s_next, T):
        """float32 state rows for the first-layer GEMMs and their layout: ((eval rows, rows per episode, offset), (target ...)).
        When s / s_next are the two views of one (B, T' + 1, S) tensor (the replay ring, include/qmix_ops.h) the T + 1 slots are
        converted once and shared; otherwise each is converted on its own."""
        B, S = s.shape[0], s.shape[-1]
        shared = (s.dim() == 3 and s.stride(2) == 1 and s.stride(1) == S and s_next.stride() == s.stride()
                  and s_next.data_ptr() == s.data_ptr() + S and s.shape[1] >= T and s_next.shape[1] >= T)
        if shared:
            full = torch.as_strided(s, (B, T + 1, S), s.stride()).float().contiguous().view(B * (T + 1), S)
            return (full, T + 1, 0), (full, T + 1, 1)
        return ((s[:, :T].float().reshape(B * T, S), T, 0), (s_next[:, :T].float().reshape(B * T, S), T, 0))

    def _mix_td_fused(self, q_e, q_t, batch, T, *sel):
        a = self.args
        B, n, A = batch['u'].shape[0], self.n_agents, batch['avail_u_next'].shape[3]
        H, M = a.hyper_hidden_dim, a.qmix_hidden_dim
        (se, pe_rows, pe_off), (st, pt_rows, pt_off) = self._state_rows(batch['s'], batch['s_next'], T)
        p_e = self._first_layers(self.eval_qmix_net, se)
        with torch.no_grad():
            p_t = self._first_layers(self.target_qmix_net, st)
        tgt = tuple(t.detach() for t in self.target_qmix_net.second_layers())
        dims = (B, T, n, A, H, M, pe_rows, pe_off, pt_rows, pt_off)
        return _MixTD.apply(q_e, p_e, *self.eval_qmix_net.second_layers(), q_t, p_t, tgt, batch['u'], batch['r'],
                            batch['avail_u_next'], batch['terminated'], batch['padded'], dims, a.gamma, self._bad_counter('_mix_bad'),
                            self._td_lambda(), *sel)
