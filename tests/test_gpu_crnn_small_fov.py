"""The fov 5 / 7 front end (include/crnn_fov.h) against float64 torch on the CPU: forward (conv features, the vector branch
relu(mlp1(vec)), the zero tail of a padded row) and the conv weight gradients of the backward.  fov 7: conv1 7x7->5x5 and
conv2 5x5->3x3; fov 5: conv1 5x5->3x3 (network/base_net.py:23-33)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRAD_TOL = 5e-6   # relative L2 of an fp32 gradient tensor against float64 autograd (as for fov 9, tests/test_gpu_crnn_ops.py)


def _net(fov, od, seed):
    from marl_dmfb_amd.network.base_net import CRNN
    a = types.SimpleNamespace(obs_shape=(3, fov, fov, 2, 3 * fov * fov + 2), hyper_hidden_dim=od, rnn_hidden_dim=128, n_actions=5, fov=fov)
    torch.manual_seed(seed)
    net = CRNN(a).cuda()
    assert net._hip_geometry() == fov
    return net


def _obs(fov, rows, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randint(-10, 11, (rows, 3 * fov * fov + 2), dtype=torch.int8, generator=g)
    onehot = torch.nn.functional.one_hot(torch.randint(0, 5, (rows,), generator=g), 5).to(torch.int8)
    onehot[::3] = 0   # first steps of episodes: no last action
    return obs, onehot


def _ref_pixels(net, obs, fov):
    x = obs[:, :3 * fov * fov].double().view(-1, 3, fov, fov)
    zs = []
    for conv in net.convs:
        z = torch.nn.functional.conv2d(x, conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu())
        zs.append(z)
        x = torch.relu(z)
    return x.reshape(obs.shape[0], -1), zs


@pytest.mark.parametrize('rows', [1, 7, 4097, 16384])
@pytest.mark.parametrize('od', [24, 32])
@pytest.mark.parametrize('fov', [5, 7])
def test_front_forward_matches_float64(fov, od, rows):
    net = _net(fov, od, fov * 100 + od + rows)
    obs, onehot = _obs(fov, rows, rows)
    P = 3 * fov * fov
    with torch.no_grad():
        pix = net._pixel_features_hip(obs.cuda()).cpu()
        padded = net._front_features_hip(obs.cuda(), onehot.cuda(), padded=True).cpu()
        plain = net._front_features_hip(obs.cuda(), None).cpu()
    ref, _ = _ref_pixels(net, obs, fov)
    vec = torch.cat([obs[:, P:].double(), onehot.double()], dim=1)
    ref_vec = torch.relu(vec @ net.mlp1.weight.detach().double().cpu().t() + net.mlp1.bias.detach().double().cpu())
    ref_vec0 = torch.relu(obs[:, P:].double() @ net.mlp1.weight.detach().double().cpu()[:, :2].t() + net.mlp1.bias.detach().double().cpu())
    assert pix.shape == (rows, od * 9) and padded.shape == (rows, net.padded_cols()) and plain.shape == (rows, od * 9 + 10)
    assert net.padded_cols() == (256 if od == 24 else 320)
    np.testing.assert_allclose(pix.numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(padded[:, :od * 9].numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(padded[:, od * 9:od * 9 + 10].numpy(), ref_vec.numpy(), rtol=1e-5, atol=1e-5)
    assert torch.all(padded[:, od * 9 + 10:] == 0)
    np.testing.assert_allclose(plain[:, :od * 9].numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(plain[:, od * 9:].numpy(), ref_vec0.numpy(), rtol=1e-5, atol=1e-5)   # NULL one-hot = zeros


def _rel_l2(g, r):
    return float(np.linalg.norm(g.astype(np.float64) - r) / max(np.linalg.norm(r), 1e-30))


@pytest.mark.parametrize('rows', [11, 5003, 20000])
@pytest.mark.parametrize('od', [24, 32])
@pytest.mark.parametrize('fov', [5, 7])
def test_front_backward_matches_float64_autograd(fov, od, rows):
    """Gradients of every CRNN front-end parameter through the HIP forward + backward (_FrontFovTrain) against float64 autograd.
    Rows with a pre-activation within 2e-5 of zero get a zero upstream gradient (their fp32 ReLU mask may differ from float64's):
    what is compared is summation error only."""
    from marl_dmfb_amd.network.base_net import _FrontFovTrain
    net = _net(fov, od, fov * 7 + od + rows)
    obs, onehot = _obs(fov, rows, rows + 1)
    _, zs = _ref_pixels(net, obs, fov)
    safe = torch.ones(rows, dtype=torch.bool)
    for z in zs:
        safe &= z.abs().reshape(rows, -1).min(dim=1).values > 2e-5
    assert safe.float().mean() > 0.8 or rows < 100
    cols = net.padded_cols()
    gen = torch.Generator().manual_seed(rows)
    gout = torch.randn(rows, cols, generator=gen, dtype=torch.float64) * safe[:, None]
    params = [net.mlp1.weight, net.mlp1.bias] + [t for c in net.convs for t in (c.weight, c.bias)]
    x = _FrontFovTrain.apply(obs.cuda(), onehot.cuda(), fov, net.mlp1.weight, net.mlp1.bias, cols, *params[2:])
    (x * gout.float().cuda()).sum().backward()
    got = [p.grad.detach().cpu().double().numpy() for p in params]
    ref_params = [p.detach().cpu().double().requires_grad_(True) for p in params]
    P = 3 * fov * fov
    h = obs[:, :P].double().view(rows, 3, fov, fov)
    for k in range(len(net.convs)):
        h = torch.relu(torch.nn.functional.conv2d(h, ref_params[2 + 2 * k], ref_params[3 + 2 * k]))
    vec = torch.cat([obs[:, P:].double(), onehot.double()], dim=1)
    v = torch.relu(vec @ ref_params[0].t() + ref_params[1])
    (h.reshape(rows, -1) * gout[:, :od * 9]).sum().add_((v * gout[:, od * 9:od * 9 + 10]).sum()).backward()
    for name, g, r in zip(['mlp_w', 'mlp_b', 'w1', 'b1', 'w2', 'b2'], got, ref_params):
        err = _rel_l2(g, r.grad.numpy())
        print('fov %d od %d rows %d %s rel_l2 %.2e' % (fov, od, rows, name, err))
        assert err <= GRAD_TOL, (name, err)


def test_backward_is_deterministic():
    from marl_dmfb_amd.network.base_net import _FrontFovTrain
    net = _net(7, 24, 3)
    obs, onehot = _obs(7, 9001, 4)
    outs = []
    for _ in range(2):
        for p in net.parameters():
            p.grad = None
        x = _FrontFovTrain.apply(obs.cuda(), onehot.cuda(), 7, net.mlp1.weight, net.mlp1.bias, 256,
                                 net.convs[0].weight, net.convs[0].bias, net.convs[1].weight, net.convs[1].bias)
        (x * x).sum().backward()
        outs.append([p.grad.clone() for p in (net.convs[0].weight, net.convs[1].weight)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
