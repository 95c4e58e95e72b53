"""Records tests/golden/crnn_front9_od24_rows33.npz: one seeded real-valued od-24 network and 33 observation rows, and what
crnn_front9_forward of the library in use computes for them (640 padded columns).  tests/test_gpu_crnn_pairtile.py compares later
builds with it bit for bit.  The committed file was recorded on an MI355X with the build of the commit BEFORE conv2's pair tiles
(marl_dmfb_amd/csrc/crnn_mfma.h); run it again only from a build whose bits are meant to become the new record.

    python tools/record_conv_fixture.py OUT.npz        (MARL_DMFB_VARIANT_CRNN_OPS=_tag picks a variant library)"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ROWS, OD, A, PAD = 33, 24, 5, 640


def make_inputs():
    torch.manual_seed(20240924)
    conv1, conv2, mlp = torch.nn.Conv2d(3, OD, 3), torch.nn.Conv2d(OD, OD, 3), torch.nn.Linear(2 + A, 10)
    obs = torch.randint(-10, 11, (ROWS, 245), dtype=torch.int8)
    obs[:, 243:] = torch.randint(-2, 3, (ROWS, 2), dtype=torch.int8)
    onehot = torch.zeros((ROWS, A), dtype=torch.int8)
    onehot[torch.arange(ROWS), torch.randint(0, A, (ROWS,))] = 1
    p = dict(w1=conv1.weight, b1=conv1.bias, w2=conv2.weight, b2=conv2.bias, mlp_w=mlp.weight, mlp_b=mlp.bias)
    return obs, onehot, {k: v.detach().contiguous() for k, v in p.items()}


def main(path):
    from marl_dmfb_amd import _lib
    obs, onehot, p = make_inputs()
    d = {k: v.cuda() for k, v in p.items()}
    d_obs, d_oh = obs.cuda(), onehot.cuda()
    out = torch.full((ROWS, PAD), -1.0, device='cuda')
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = _lib.crnn_ops().crnn_front9_forward(ptr(d_obs), 245, ptr(d_oh), A, ROWS, ptr(d['w1']), ptr(d['b1']), ptr(d['w2']), ptr(d['b2']),
                                             ptr(d['mlp_w']), ptr(d['mlp_b']), OD, ptr(out), PAD, PAD, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    np.savez_compressed(path, obs=obs.numpy(), onehot=onehot.numpy(), out=out.cpu().numpy(), **{k: v.numpy() for k, v in p.items()})
    print('recorded', path, os.path.getsize(path), 'bytes; positive outputs: %.2f' % float((out[:, :600] > 0).float().mean()))


if __name__ == '__main__':
    main(sys.argv[1])
