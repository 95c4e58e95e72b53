"""Double-Q targets of the VDN learn (args.double_q, --double_q); DESIGN.md has the why.

Every learn bootstraps on Q'[t], the target side's value of the next observation, summed over the agents.  With double_q off that is
the reference's max_a Q_target(o', a) per agent (policy/vdn.py:104-123).  With double_q on the EVAL network chooses the action and the
target network values it (double Q-learning; PyMARL's `double_q: True`).  Nothing behind Q'[t] changes: the one-step target
r + (gamma * Q') * nt, the lambda walk of policy/td_lambda.py, mask, loss and backward.

The rule.  Per (episode, step) slot and agent i, with q_sel the selector's row (the eval network's Q at the next observation,
detached), q_target the target network's and A actions:

    s(a)  = -9999999 if avail_next[i][a] == 0 else q_sel[i][a]
    a* = 0; m = s(0); for a = 1 .. A-1: if s(a) > m: m = s(a); a* = a
    v_i   = -9999999 if avail_next[i][a*] == 0 else q_target[i][a*]
    Q'    = the sum of v_i over i in index order, in the working precision

The first maximum wins, a NaN never displaces an earlier value, a row with no available action picks 0.  With q_sel == q_target, Q' is
the current rule's value bit for bit: the value at a row's own first maximum is its maximum.

`double_pick_reference` is this rule in numpy: with dtype=np.float32 it is the result of the HIP kernels of include/vdn_double.h bit
for bit, with np.float64 the ground truth.  `double_pick_torch` is the same rule in torch ops for the learn path that does not run the
fused TD block (CPU tensors)."""
import numpy as np

UNAVAILABLE = -9999999.0


def double_pick_reference(q_sel, q_target, avail_next, dtype=np.float32):
    """(picks int8 (..., n), Q' `dtype` (...)) of the rule above.  q_sel, q_target, avail_next: (..., n, A) arrays of one shape; every
    operation is an operation of `dtype`."""
    q_sel, q_target = np.asarray(q_sel, dtype), np.asarray(q_target, dtype)
    off = np.asarray(avail_next) == 0
    assert q_sel.shape == q_target.shape == off.shape and q_sel.ndim >= 2
    n, A = q_sel.shape[-2:]
    fill = dtype(UNAVAILABLE)
    s = np.where(off, fill, q_sel).astype(dtype)
    best = np.zeros(s.shape[:-1], np.int64)
    m = s[..., 0].copy()
    with np.errstate(invalid='ignore'):
        for a in range(1, A):
            take = s[..., a] > m               # False for a NaN on either side: it never displaces, and is never displaced
            m = np.where(take, s[..., a], m)
            best = np.where(take, a, best)
    v = np.where(off, fill, q_target).astype(dtype)
    v = np.take_along_axis(v, best[..., None], axis=-1)[..., 0]
    q_next = np.zeros(v.shape[:-1], dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(n):
            q_next = (q_next + v[..., i]).astype(dtype)
    return best.astype(np.int8), q_next


def double_pick_torch(q_sel, q_target, avail_next):
    """The rule in torch ops: q_sel, q_target (..., n, A) tensors of one dtype, avail_next the same shape (0 = unavailable) ->
    (picks int64 (..., n), the picked target values (..., n)); the caller's mixer adds the agents.  No graph is kept.  The walk over the
    actions is written out (torch.argmax does not promise the first maximum, nor this treatment of NaN)."""
    import torch
    with torch.no_grad():
        off = avail_next == 0
        s = q_sel.masked_fill(off, UNAVAILABLE)
        best = torch.zeros(s.shape[:-1], dtype=torch.long, device=s.device)
        m = s[..., 0].clone()
        for a in range(1, s.shape[-1]):
            take = s[..., a] > m
            m = torch.where(take, s[..., a], m)
            best = torch.where(take, torch.full_like(best, a), best)
        v = q_target.masked_fill(off, UNAVAILABLE)
        return best, torch.gather(v, -1, best.unsqueeze(-1)).squeeze(-1)


def selector_units(counts):
    """Host side of the packed learn's selector (VDN.learn_packed).  counts[t] = the episodes longer than t of a length-sorted batch of
    B = counts[0] episodes, unit (e, t) = off[t] + e as VDN.pack_units lays them out, U units in all.  The selector tensor holds the U
    units of the eval network's Q followed by B tail units (one more step of every episode behind its last valid one).  Returns
    (sel_units int32[U]: unit (e, t) -> off[t+1] + e where episode e is longer than t + 1, else U + e;
     last_units int32[B]: the last unit of every episode)."""
    counts = np.asarray(counts, np.int64)
    B, T = int(counts[0]), len(counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    U = int(off[-1])
    sel = np.empty(U, np.int32)
    last = np.empty(B, np.int32)
    for t in range(T):
        c = int(counts[t])
        nxt = int(counts[t + 1]) if t + 1 < T else 0
        e = np.arange(c)
        sel[off[t]:off[t] + c] = np.where(e < nxt, off[t + 1] + e, U + e)
        last[nxt:c] = off[t] + e[nxt:]
    return sel, last
