"""vdn_gather_units_batch (include/vdn_tail.h) with four destination words per thread, against an index_select on the host, byte
for byte.  A thread's four words may lie in two units (980-byte units = 245 words), in up to four (a 4-byte unit), behind the last
unit (the zero tail) or behind the destination (nothing written): every case below checks the units, the zero tail and the guard
bytes in front of and behind the destination.  Destination starts: 16-byte aligned (one 16-byte store per thread), 4-byte aligned
only (word stores) and odd (the byte kernel, whatever the unit size)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
vp = C.c_void_p
GUARD = 64
N_SRC = 80           # source units


def _unit_list(kind, U, g):
    if kind == 'repeats':
        return torch.randint(1, 6, (U,), generator=g, dtype=torch.int32)
    return torch.arange(N_SRC - 1, N_SRC - 1 - U, -1, dtype=torch.int32)   # descending, all >= 1 (shift -1 stays inside the source)


def _want(src, units, shift, zero_below, dst_bytes):
    """src (N_SRC, unit_bytes) uint8 on the host -> the dst_bytes bytes the kernel has to leave."""
    rows = torch.index_select(src, 0, (units.long() + shift).clamp(min=0)).clone()
    rows[:zero_below] = 0
    out = torch.zeros(dst_bytes, dtype=torch.uint8)
    out[:rows.numel()] = rows.view(-1)
    return out


@pytest.mark.parametrize('start', [0, 4, 1], ids=['aligned16', 'aligned4', 'odd'])
@pytest.mark.parametrize('kind', ['repeats', 'descending'])
@pytest.mark.parametrize('padded', [True, False], ids=['pad64', 'nopad'])
@pytest.mark.parametrize('U', [1, 3, 67])
def test_gather_batch_equals_host_index_select(U, padded, kind, start):
    """One launch of four gathers over one unit list: 980-byte units (o of four agents), 20-byte units (u_onehot), the 20-byte units
    with shift -1 and zero_below = 2 (the last action), and 4-byte units (a thread's four words = four units).  Row = unit / 4."""
    from marl_dmfb_amd import _lib
    lib = _lib.vdn_tail()
    g = torch.Generator().manual_seed(1000 * U + 10 * start + padded)
    units = _unit_list(kind, U, g)
    unit_bytes = [980, 20, 20, 4]
    shifts, zbs = [0, 0, -1, 0], [0, 0, 2, 0]
    srcs = [torch.randint(0, 256, (N_SRC, ub), generator=g, dtype=torch.int32).to(torch.uint8) for ub in unit_bytes]
    V = 4 * U
    rows = -(-V // 64) * 64 if padded else V
    dst_bytes = [rows * ub // 4 for ub in unit_bytes]
    bufs = [torch.full((GUARD + db + GUARD,), 0x7f, dtype=torch.uint8, device='cuda') for db in dst_bytes]
    off = GUARD + start
    d_srcs = [s.cuda() for s in srcs]
    d_units = units.cuda()
    k = 4
    rc = lib.vdn_gather_units_batch(k, (vp * k)(*[s.data_ptr() for s in d_srcs]), (C.c_int32 * k)(*unit_bytes), (C.c_int32 * k)(*shifts),
                                    (C.c_int32 * k)(*zbs), (vp * k)(*[b.data_ptr() + off for b in bufs]), (C.c_int64 * k)(*dst_bytes),
                                    vp(d_units.data_ptr()), U, None)
    assert rc == 0
    torch.cuda.synchronize()
    for i in range(k):
        got = bufs[i].cpu()
        assert bool((got[:off] == 0x7f).all()) and bool((got[off + dst_bytes[i]:] == 0x7f).all()), 'gather %d wrote outside its destination' % i
        want = _want(srcs[i], units, shifts[i], zbs[i], dst_bytes[i])
        assert torch.equal(got[off:off + dst_bytes[i]], want), 'gather %d' % i


def test_gather_batch_of_the_learn_rows_is_what_the_single_gather_gives():
    """The shapes of a learn: o / o_next / u_onehot / shifted u_onehot into fresh (16-byte aligned) allocations of Vp rows, against
    vdn_gather_units (one word per thread) on the same inputs."""
    from marl_dmfb_amd import _lib
    lib, one = _lib.vdn_tail(), _lib.vdn_ops()
    g = torch.Generator().manual_seed(7)
    n, U, B = 4, 331, 9
    units = torch.randint(1, N_SRC, (U,), generator=g, dtype=torch.int32).cuda()
    row_bytes = [245, 245, 5, 5]
    srcs = [torch.randint(0, 256, (N_SRC * n, rb), generator=g, dtype=torch.int32).to(torch.uint8).cuda() for rb in row_bytes[:3]]
    srcs.append(srcs[2])
    shifts, zbs = [0, 0, 0, -1], [0, 0, 0, B]
    Vp = -(-U * n // 64) * 64
    outs = [torch.full((Vp, rb), 0x7f, dtype=torch.uint8, device='cuda') for rb in row_bytes]
    k = 4
    rc = lib.vdn_gather_units_batch(k, (vp * k)(*[s.data_ptr() for s in srcs]), (C.c_int32 * k)(*[n * rb for rb in row_bytes]),
                                    (C.c_int32 * k)(*shifts), (C.c_int32 * k)(*zbs), (vp * k)(*[o.data_ptr() for o in outs]),
                                    (C.c_int64 * k)(*[o.numel() for o in outs]), vp(units.data_ptr()), U, None)
    assert rc == 0
    for i in range(k):
        want = torch.zeros_like(outs[i])
        assert one.vdn_gather_units(vp(srcs[i].data_ptr()), n * row_bytes[i], vp(units.data_ptr()), U, shifts[i], zbs[i],
                                    vp(want.data_ptr()), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(outs[i], want), i
