"""The fused QMIX mixing / TD block (include/qmix_ops.h) against float64 autograd of QMixNet + the TD rule of policy/qmix.py:104-122:
every gradient the learner uses (eval Q values, the first-layer weights and biases through the GEMM, the second-layer weights and
biases) at relative L2 5e-6 per tensor (GRAD_TOL of tests/test_gpu_crnn_ops.py); bad actions; bit-identical repeat launches."""
import types

import pytest
import torch

from marl_dmfb_amd.network.qmix_net import QMixNet

GRAD_TOL = 5e-6


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _case(n, hh, B, T, seed, A=5, S=300):
    g = torch.Generator().manual_seed(seed)
    args = types.SimpleNamespace(state_shape=S, hyper_hidden_dim=hh, qmix_hidden_dim=32, n_agents=n, two_hyper_layers=True)
    torch.manual_seed(seed)
    ev, tg = QMixNet(args), QMixNet(args)
    with torch.no_grad():
        for p in list(ev.parameters()) + list(tg.parameters()):
            p.mul_(3.0)   # wider spread of the hypernetwork outputs: both signs inside abs / relu / elu
    Tl = T + 3
    st = torch.zeros((B, Tl + 1, S), dtype=torch.int8)
    nz = torch.rand((B, Tl + 1, S), generator=g) < 0.04
    st[nz] = torch.randint(1, n + 1, (int(nz.sum()),), generator=g, dtype=torch.int8)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    t = torch.arange(Tl)[None, :]
    padded = (t >= lens[:, None]).unsqueeze(-1)
    term = (t >= lens[:, None] - 1).unsqueeze(-1) & (torch.rand((B, 1, 1), generator=g) < 0.7)
    term = term | padded
    batch = {'u': torch.randint(0, A, (B, Tl, n, 1), generator=g, dtype=torch.int8),
             'r': torch.randn((B, Tl, 1), generator=g),
             'avail_u_next': (torch.rand((B, Tl, n, A), generator=g) < 0.8).to(torch.int8),
             'terminated': term, 'padded': padded}
    q_e = torch.randn((T, B * n, A), generator=g) * 2
    q_t = torch.randn((T, B * n, A), generator=g) * 2
    return args, ev, tg, st, batch, q_e, q_t


def _reference64(args, ev, tg, st, batch, q_e, q_t, T, gamma=0.99):
    ev64, tg64 = QMixNet(args).double(), QMixNet(args).double()
    ev64.load_state_dict(ev.state_dict()); tg64.load_state_dict(tg.state_dict())
    B, n = batch['u'].shape[0], args.n_agents
    qe = q_e.double().clone().requires_grad_(True)
    qev = qe.view(T, B, n, -1).permute(1, 0, 2, 3)
    qtv = q_t.double().view(T, B, n, -1).permute(1, 0, 2, 3)
    u = batch['u'][:, :T].long()
    qg = torch.gather(qev, 3, u).squeeze(3)
    qm = qtv.masked_fill(batch['avail_u_next'][:, :T] == 0, -9999999).max(3)[0]
    s, s_next = st[:, :T].double(), st[:, 1:T + 1].double()
    tot_e, tot_t = ev64(qg, s), tg64(qm, s_next)
    targets = batch['r'][:, :T].double() + gamma * tot_t * (1 - batch['terminated'][:, :T].double())
    mask = 1 - batch['padded'][:, :T].double()
    num = ((mask * (tot_e - targets.detach())) ** 2).sum()
    num.backward()
    return num, qe.grad, {k: p.grad for k, p in ev64.named_parameters()}


def _fused(args, ev, tg, st, batch, q_e, q_t, T, bad=None):
    from marl_dmfb_amd.policy.qmix import QMIX
    dev = 'cuda:0'
    pol = QMIX.__new__(QMIX)
    pol.args = types.SimpleNamespace(hyper_hidden_dim=args.hyper_hidden_dim, qmix_hidden_dim=32, gamma=0.99)
    pol.n_agents, pol.device = args.n_agents, torch.device(dev)
    pol.eval_qmix_net, pol.target_qmix_net = ev.to(dev), tg.to(dev)
    pol._mix_bad = bad
    if bad is not None:
        pol._td_bad = bad
    b = {k: v.to(dev) for k, v in batch.items()}
    stg = st.to(dev)
    b['s'], b['s_next'] = stg[:, :-1], stg[:, 1:]
    b = {k: v[:, :T] for k, v in b.items()}
    for p in ev.parameters():
        p.grad = None
    qe = q_e.to(dev).requires_grad_(True)
    if bad is None:
        pol._mix_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    num, mask_sum = pol._mix_td_fused(qe, q_t.to(dev), b, T)
    num.backward()
    return num, qe.grad, {k: p.grad for k, p in ev.named_parameters()}, pol._mix_bad


CASES = [(2, 24, 64, 12), (4, 24, 512, 40), (10, 32, 256, 80), (16, 32, 128, 20), (4, 32, 512, 40), (10, 24, 20480 // 80, 80)]


@pytest.mark.gpu
@pytest.mark.parametrize('n,hh,B,T', CASES, ids=['n%d_hh%d_B%d_T%d' % c for c in CASES])
def test_fused_mix_td_matches_float64_autograd(n, hh, B, T):
    args, ev, tg, st, batch, q_e, q_t = _case(n, hh, B, T, seed=n * 100 + hh)
    num64, gq64, g64 = _reference64(args, ev, tg, st, batch, q_e, q_t, T)
    num, gq, gw, bad = _fused(args, ev, tg, st, batch, q_e, q_t, T)
    assert abs(float(num) - float(num64)) <= 1e-5 * abs(float(num64))
    assert _rel(gq.cpu(), gq64) < GRAD_TOL, _rel(gq.cpu(), gq64)
    for k, ref in g64.items():
        assert _rel(gw[k].cpu(), ref) < GRAD_TOL, (k, _rel(gw[k].cpu(), ref))
    assert int(bad.item()) == 0


@pytest.mark.gpu
def test_bad_action_gives_nan_and_counts():
    args, ev, tg, st, batch, q_e, q_t = _case(4, 24, 32, 10, seed=5)
    batch['u'][3, 2, 1, 0] = 7
    batch['u'][5, 0, 0, 0] = -1
    num, gq, _, bad = _fused(args, ev, tg, st, batch, q_e, q_t, 10)
    assert torch.isnan(num).item()
    assert int(bad.item()) == 2


@pytest.mark.gpu
def test_two_launches_bitwise_equal():
    args, ev, tg, st, batch, q_e, q_t = _case(10, 32, 256, 80, seed=9)
    a = _fused(args, ev, tg, st, batch, q_e, q_t, 80)
    b = _fused(args, ev, tg, st, batch, q_e, q_t, 80)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
