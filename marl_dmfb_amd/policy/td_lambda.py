"""TD(lambda) targets of the VDN learn (args.td_lambda, --td_lambda) and of the QMIX learn (args.qmix_lambda, --qmix_lambda); DESIGN.md
has the why.

The learn regresses Q_tot(t) onto a target G[t].  With td_lambda == 0 that is the reference's one-step target
r_t + gamma * Q'_tot(t) * (1 - terminated_t) (policy/vdn.py:104-123); with td_lambda > 0 it is the lambda-return of the episode, the
quantity the reference's unused `td_lambda_target` (common/utils.py:33-79) computes, as a backward recurrence.

The rule.  Per episode, T = the steps the learn sees, L = the count of leading steps with padded == 0, Q'[t] = the target network's
Q_tot of step t (the sum over the agents of the best available next Q), nt[t] = 1 - terminated[t], om = 1 - lam formed once.  For
t = T-1 down to 0, every operation in the working precision and in this order:

    y[t] = Q'[t]                              if t >= L-1   (a padded slot, or the episode's last valid step: the one-step target)
    y[t] = (om * Q'[t]) + (lam * G[t+1])      otherwise
    G[t] = r[t] + (gamma * y[t]) * nt[t]

`lambda_targets_reference` is this rule in numpy: with dtype=np.float32 it is the result of the HIP kernels of
include/vdn_lambda.h bit for bit, with np.float64 the ground truth.  `lambda_targets_torch` is the same walk in torch ops for the
learn path that does not run the fused TD block (CPU tensors).

On an episode whose last valid step is terminated, G equals the reference's `td_lambda_target` up to float32 rounding.  For an
episode that is shorter than the batch and whose last valid step is NOT terminated the reference drops the bootstrap of the n-step
returns that run past the episode's end (they are multiplied by the padding mask); the rule keeps Q'[L-1] there."""
import numpy as np


def check_lambda(lam, name='td_lambda'):
    """lam (args.<name>) as a float in [0, 1]; ValueError otherwise (NaN included)."""
    try:
        value = float(lam)
    except (TypeError, ValueError):
        raise ValueError('%s must be a number in [0, 1], got %r' % (name, lam))
    if not 0.0 <= value <= 1.0:
        raise ValueError('%s must lie in [0, 1], got %r' % (name, lam))
    return value


def _leading_valid(padded):
    """(B,) count of leading steps with padded == 0 of a (B, T) array."""
    pad = np.asarray(padded) != 0
    T = pad.shape[1]
    return np.where(pad.any(axis=1), pad.argmax(axis=1), T)


def lambda_targets_reference(q_tot_target, r, terminated, padded, gamma, lam, dtype=np.float32):
    """G of the rule above.  q_tot_target, r, terminated, padded: (B, T) or (B, T, 1) arrays; returns G in `dtype` and the shape of
    q_tot_target.  Every operation is an operation of `dtype`."""
    lam = check_lambda(lam)
    shape = np.shape(q_tot_target)
    B, T = shape[0], shape[1]
    q = np.asarray(q_tot_target, dtype).reshape(B, T)
    r = np.asarray(r, dtype).reshape(B, T)
    nt = dtype(1) - (np.asarray(terminated).reshape(B, T) != 0).astype(dtype)
    L = _leading_valid(np.asarray(padded).reshape(B, T))
    gamma, lam = dtype(gamma), dtype(lam)
    om = dtype(1) - lam
    G = np.zeros((B, T), dtype)
    g_next = np.zeros(B, dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        for t in range(T - 1, -1, -1):
            mixed = (om * q[:, t]) + (lam * g_next)
            y = np.where(t >= L - 1, q[:, t], mixed).astype(dtype)
            g_next = (r[:, t] + (gamma * y) * nt[:, t]).astype(dtype)
            G[:, t] = g_next
    return G.reshape(shape)


def lambda_targets_torch(q_tot_target, r, terminated, padded, gamma, lam):
    """The same walk in torch ops over (B, T, 1) tensors (terminated / padded as 0 / 1 in the tensors' dtype); no graph is kept."""
    import torch
    lam = check_lambda(lam)
    with torch.no_grad():
        q = q_tot_target
        T = q.shape[1]
        pad = padded != 0
        steps = torch.arange(T, device=q.device).view(1, T, 1)
        L = torch.where(pad, steps, torch.full_like(steps, T)).amin(dim=1, keepdim=True)    # leading steps with padded == 0
        own = steps >= L - 1                                                                 # slots that keep the one-step target
        nt = 1 - terminated
        if q.dtype == torch.float32:   # lam and 1 - lam as the kernels hold them: rounded to float32, then subtracted
            lam, om = float(np.float32(lam)), float(np.float32(1) - np.float32(lam))
        else:
            om = 1.0 - lam
        G = torch.empty_like(q)
        g_next = torch.zeros_like(q[:, 0])
        for t in range(T - 1, -1, -1):
            y = torch.where(own[:, t], q[:, t], (om * q[:, t]) + (lam * g_next))
            g_next = r[:, t] + (gamma * y) * nt[:, t]
            G[:, t] = g_next
    return G
