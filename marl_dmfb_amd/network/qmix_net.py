"""QMIX mixing network (reference network/qmix_net.py): hypernetworks conditioned on the global state produce the weights of a
monotonic two-layer mixer of the agents' Q values.  Same constructor arguments, module layout and state_dict keys as the
reference, so its checkpoints load unchanged.

This is the plain-torch form: the CPU path and the fallback of policy/qmix.py.  On the GPU the learner runs the first layers of
the four hypernetworks as one GEMM and everything after them as one HIP launch each way (include/qmix_ops.h)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class QMixNet(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        S, hh, M, n = args.state_shape, args.hyper_hidden_dim, args.qmix_hidden_dim, args.n_agents
        if args.two_hyper_layers:
            self.hyper_w1 = nn.Sequential(nn.Linear(S, hh), nn.ReLU(), nn.Linear(hh, n * M))
            self.hyper_w2 = nn.Sequential(nn.Linear(S, hh), nn.ReLU(), nn.Linear(hh, M))
        else:
            self.hyper_w1 = nn.Linear(S, n * M)
            self.hyper_w2 = nn.Linear(S, M)
        self.hyper_b1 = nn.Linear(S, M)
        self.hyper_b2 = nn.Sequential(nn.Linear(S, M), nn.ReLU(), nn.Linear(M, 1))

    def forward(self, q_values, states):
        """q_values (B, T, n), states (B, T, state_shape) -> q_total (B, T, 1)."""
        B = q_values.size(0)
        n, M, S = self.args.n_agents, self.args.qmix_hidden_dim, self.args.state_shape
        q = q_values.reshape(-1, 1, n)
        s = states.reshape(-1, S)
        w1 = torch.abs(self.hyper_w1(s)).view(-1, n, M)
        b1 = self.hyper_b1(s).view(-1, 1, M)
        hidden = F.elu(torch.bmm(q, w1) + b1)
        w2 = torch.abs(self.hyper_w2(s)).view(-1, M, 1)
        b2 = self.hyper_b2(s).view(-1, 1, 1)
        return (torch.bmm(hidden, w2) + b2).view(B, -1, 1)

    # ---- the split the fused GPU path uses (policy/qmix.py)
    def first_layers(self):
        """The four Linear layers that read the state, in the row order of the concatenated [F][S] weight
        (F = 2 * hyper_hidden_dim + 2 * qmix_hidden_dim): hyper_w1[0], hyper_w2[0], hyper_b1, hyper_b2[0]."""
        return [self.hyper_w1[0], self.hyper_w2[0], self.hyper_b1, self.hyper_b2[0]]

    def second_layers(self):
        """(weight, bias) tensors of hyper_w1[2], hyper_w2[2], hyper_b2[2] (include/qmix_ops.h: qmix_mixer)."""
        return [self.hyper_w1[2].weight, self.hyper_w1[2].bias, self.hyper_w2[2].weight, self.hyper_w2[2].bias,
                self.hyper_b2[2].weight, self.hyper_b2[2].bias]
