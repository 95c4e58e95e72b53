"""Record what the reference's task, block and degrade-map GENERATORS accept (container-only).

Every other env golden injects its tasks, blocks and maps; here the reference draws them itself:
  DMFB  RoutingTaskManager._Generate_Start_End, GenRandomBlocks, _random_health_statue   (env/DMFB/dmfb.py:157-251)
  MEDA  RoutingTaskManager.addTask, _genLegalDroplet, getRandomYX and the degrade map of
        MEDAEnv.__init__                                                                 (env/MEDA/meda.py:175-233, :497-502)
The build's RNG contract says which Philox4x32-10 word is which candidate.  A feeder per
chip computes that candidate stream here, in plain Python, and hands exactly those candidates to the unmodified
reference generators through `ref_shim.patch_generators` (np.random.randint, np.random.rand, random.randrange,
random.randint).  What the reference then ACCEPTS is recorded; oracle/dmfb_oracle.c, oracle/meda_oracle.c and the HIP
kernels must accept the same (tests/test_generator_golden.py, tests/test_gpu_generator_golden.py).  The feeder
asserts the bound and the shape of every call, so a reference that drew in another order or range fails here.

tests/golden/gen_<dmfb|meda>_<case>.npz, 64 chips (chip k = global env id k), three task generations
p = 0 (constructor), 1 (refresh()), 2 (DMFB: refresh(new=True), MEDA: refresh()), i.e. rng_ep = p:
  cfg              DMFB (W, L, n, fov, n_blocks, b_degrade), MEDA (W, L, n, fov, version, b_degrade)   int64
  per_degrade, seed                                                                                  float64, uint64
  p<p>_starts, p<p>_ends     (64, n, 2)  DMFB (x, y); MEDA (x_center, y_center)                       uint8
  p<p>_blocks                (64, n_blocks or 0, 4)  x_min, x_max, y_min, y_max                       uint8   (DMFB)
  p<p>_task_attempts         (64,)  attempts _Generate_Start_End consumed (accepted index + 1)        int32   (DMFB)
  p<p>_block_attempts        (64, n_blocks or 0)  attempts per block                                  int32   (DMFB)
  p<p>_draws                 (64,)  getRandomYX draws consumed                                        int32   (MEDA)
  p<p>_overlap_redraws       (64,)  destinations redrawn by addTask's isDropletOverlap loop           int32   (MEDA)
  p<p>_dest_redraws          (64,)  candidates _genLegalDroplet rejected for a destination            int32   (MEDA)
  p0_degrade, p2_degrade     (8, W, L) float64, chips 0..7; b_degrade cases only (p2: DMFB, rng_map 1)

The reference's rejection loops are unbounded (the build's stop at 2^22 attempts / 2^20 draws), so the feeder raises
after LOOP_LIMIT attempts of one loop; main() asserts that no committed case comes near it, and that the situations
the kernels treat differently occur (DMFB: accepted attempt index >= 64 for tasks and for blocks -- the kernels test
64 attempts per wave round -- and a chip accepted at attempt 0; MEDA: both redraw loops taken).

Run:  python tools/oracle/gen_generator_golden.py        (rewrites the committed files byte for byte)
"""
import contextlib
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'tests', 'golden')

N_CHIPS = 64          # chip k is global env id k
N_MAP_CHIPS = 8       # degrade maps are stored for the first chips only (file size)
LOOP_LIMIT = 4096     # the feeder gives up on a rejection loop here; committed cases stay well under it
LOOP_MARGIN = 2048    # "well under": asserted in main()
STREAM_TASK, STREAM_DEGRADE, STREAM_BLOCK, STREAM_MEDA_TASK = 2, 3, 4, 5
MEDA_R = 2            # RoutingTaskManager.r (meda.py:150)

# (W, L, n, fov, n_blocks, b_degrade, per_degrade, seed).  A block accepted at attempt >= 64 is rare at these sizes: none
# of the seeds 1..119 gives one with 4 blocks on 10x10, so a case with 5 blocks (20 % exactly, the densest the density rule
# lets through) is added, with the first seed from 1 up that holds one (chip 51, generation 2, block 4: 75 attempts).
DMFB_CASES = [
    (10, 10, 4, 9, 0, False, 0.1, 7),
    (10, 10, 4, 9, 4, False, 0.1, 2),
    (12, 9, 3, 7, 2, False, 0.1, 3),
    (20, 20, 10, 9, 12, True, 0.1, 4),
    (50, 50, 10, 9, 0, True, 0.5, 5),
    (10, 10, 4, 9, 5, False, 0.1, 1),
    (10, 10, 4, 9, 6, False, 0.1, 6),      # 6 blocks on 10x10 = 24 % > 20 %: the density rule leaves no blocks at all
]
# (W, L, n, fov, version, b_degrade, per_degrade, seed).  addTask / _genLegalDroplet / getRandomYX are the same code for
# MEDAEnv and MEDAEnv_v0_2 (only getOneObs differs), so one v0_2 case stands for the class.
MEDA_CASES = [
    (30, 30, 4, 19, 0, False, 0.1, 11),
    (30, 60, 8, 19, 2, False, 0.1, 12),
    (45, 30, 6, 9, 0, False, 0.1, 13),
    (80, 80, 10, 19, 0, True, 0.1, 14),
]


def dmfb_name(W, L, n, fov, nb, deg, per, seed):
    return 'gen_dmfb_%dx%d_%dd_fov%d_%db%s_s%d' % (W, L, n, fov, nb, '_deg%02d' % round(per * 100) if deg else '', seed)


def meda_name(W, L, n, fov, version, deg, per, seed):
    return 'gen_meda_v%d_%dx%d_%dd_fov%d%s_s%d' % (version, W, L, n, fov, '_deg%02d' % round(per * 100) if deg else '', seed)


# ---------------------------------------------------------------- the build's RNG contract, in plain Python
M32 = 0xFFFFFFFF


def philox(seed, c0, c1, c2, c3):
    """Philox4x32-10, key = the 64-bit seed (low word k0, high word k1); returns the four output words."""
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def mulhi(w, n):
    return (w * n) >> 32


def u53(hi, lo):
    return float(((hi << 32) | lo) >> 11) * 2.0 ** -53     # exact: a 53-bit integer times a power of two


class _Feeder:
    """What both envs share: the counter layout and the two np.random.rand(W, L) of a degrade map."""

    def __init__(self, seed, env_id, W, L):
        self.seed, self.e, self.W, self.L = seed, env_id, W, L
        self._map_words, self.map_calls = None, 0

    def words(self, c1, c2, stream, sub=0):
        return philox(self.seed, self.e, c1, c2, (stream << 8) | sub)

    def begin_map(self, rng_map):
        """rng_map None: no map may be drawn until the next begin_map."""
        self._map_words = None if rng_map is None else [self.words(rng_map, c, STREAM_DEGRADE) for c in range(self.W * self.L)]
        self.map_calls = 0

    def np_rand(self, *shape):
        assert shape == (self.W, self.L), 'np.random.rand%r, expected (W, L)' % (shape,)
        assert self._map_words is not None and self.map_calls < 2, 'a third np.random.rand for one map'
        a, b = (0, 1) if self.map_calls == 0 else (2, 3)       # first call: the factor, second: the selection
        self.map_calls += 1
        return np.array([u53(w[a], w[b]) for w in self._map_words], dtype=np.float64).reshape(self.W, self.L)

    def _refuse(self, *a, **k):
        raise AssertionError('the reference drew from a function this generator is not known to use')

    np_randint = randrange = randint = _refuse


class DmfbFeeder(_Feeder):
    def __init__(self, seed, env_id, W, L, n):
        super().__init__(seed, env_id, W, L)
        self.n = n
        self.begin_task(0)

    def begin_task(self, rng_ep):
        self.rng_ep = rng_ep
        self.task_attempts, self.block_attempts = 0, []
        self._task_x, self._block_x = None, None

    def idle(self):
        return self._task_x is None and self._block_x is None

    def np_randint(self, lo, hi=None, size=None):
        assert lo == 0
        if size is None:                                          # GenRandomBlocks, first candidate of a block
            return self._block(hi, 'first')
        assert tuple(size) == (2 * self.n, 1) and self._block_x is None
        if self._task_x is None:                                  # randomXY: y first, bound `l`
            assert hi == self.L, 'first randint of randomXY has bound %r, expected L' % hi
            assert not self.block_attempts, 'a task attempt after the blocks'
            assert self.task_attempts < LOOP_LIMIT, '_Generate_Start_End: %d attempts rejected' % LOOP_LIMIT
            w = [self.words(self.rng_ep, self.task_attempts, STREAM_TASK, b) for b in range(self.n)]
            self.task_attempts += 1
            self._task_x = [mulhi(v, self.W) for q in w for v in (q[1], q[3])]
            return np.array([mulhi(v, self.L) for q in w for v in (q[0], q[2])], dtype=np.int64).reshape(-1, 1)
        assert hi == self.W, 'second randint of randomXY has bound %r, expected W' % hi
        x, self._task_x = self._task_x, None
        return np.array(x, dtype=np.int64).reshape(-1, 1)

    def randrange(self, lo, hi):
        assert lo == 0
        return self._block(hi, 'redraw')

    def _block(self, hi, kind):
        assert self._task_x is None
        if self._block_x is None:                                 # y position: bound length - 3
            assert hi == self.L - 3, 'y draw of a block has bound %r, expected L - 3' % hi
            if kind == 'first':
                self.block_attempts.append(0)                     # a scalar np.random.randint here starts the next block
            assert self.block_attempts, 'a block redraw before any block'
            b = len(self.block_attempts) - 1
            assert self.block_attempts[b] < LOOP_LIMIT, 'GenRandomBlocks: %d candidates rejected' % LOOP_LIMIT
            w = self.words(self.rng_ep, self.block_attempts[b], STREAM_BLOCK, b)
            self.block_attempts[b] += 1
            self._block_x = (mulhi(w[1], self.W - 3), kind)
            return mulhi(w[0], self.L - 3)
        assert hi == self.W - 3, 'x draw of a block has bound %r, expected W - 3' % hi
        (x, was), self._block_x = self._block_x, None
        assert was == kind, 'y and x of one block candidate come from different functions'
        return x

    randint = _Feeder._refuse


class MedaFeeder(_Feeder):
    def __init__(self, seed, env_id, W, L):
        super().__init__(seed, env_id, W, L)
        self.begin_task(0)

    def begin_task(self, rng_ep):
        self.rng_ep, self.draws, self._x = rng_ep, 0, None

    def idle(self):
        return self._x is None

    def randint(self, lo, hi):                                    # random.randint is inclusive
        r = MEDA_R
        assert lo == r
        if self._x is None:
            assert hi == self.W - r - 1, 'y draw of getRandomYX has bound %r, expected W - r - 1' % hi
            assert self.draws < LOOP_LIMIT, 'addTask: %d draws' % LOOP_LIMIT
            w = self.words(self.rng_ep, self.draws, STREAM_MEDA_TASK)
            self.draws += 1
            self._x = r + mulhi(w[1], self.L - 2 * r)
            return r + mulhi(w[0], self.W - 2 * r)
        assert hi == self.L - r - 1, 'x draw of getRandomYX has bound %r, expected L - r - 1' % hi
        x, self._x = self._x, None
        return x

    np_randint = randrange = _Feeder._refuse


# ---------------------------------------------------------------- running the reference
def _u8(a, shape):
    a = np.asarray(a, dtype=np.int64).reshape(shape)
    assert a.min(initial=0) >= 0 and a.max(initial=0) <= 255
    return a.astype(np.uint8)


def record_dmfb(rd, case, chips=N_CHIPS, map_chips=N_MAP_CHIPS):
    """Run the reference generators of `chips` DMFB chips on the oracle's candidate stream; returns the arrays of the
    golden file (see the module docstring)."""
    W, L, n, fov, nb, deg, per, seed = case
    rec = {}
    for e in range(chips):
        f = DmfbFeeder(seed, e, W, L, n)
        for p in range(3):
            f.begin_task(p)
            new_map = deg and p in (0, 2)
            f.begin_map(p // 2 if new_map else None)
            with ref_shim.patch_generators(f), contextlib.redirect_stdout(io.StringIO()):   # the density rule prints
                if p == 0:
                    env = rd.DMFBenv(W, L, n, nb, fov=fov, b_degrade=deg, per_degrade=per)
                    mgr = env.routing_manager
                else:
                    mgr.refresh(new=(p == 2))
            assert f.idle() and f.map_calls == (2 if new_map else 0)
            assert len(mgr.blocks) == len(f.block_attempts)
            blocks = [(b.x_min, b.x_max, b.y_min, b.y_max) for b in mgr.blocks]
            rec.setdefault('p%d_starts' % p, []).append(_u8(mgr.starts, (n, 2)))
            rec.setdefault('p%d_ends' % p, []).append(_u8(mgr.ends, (n, 2)))
            rec.setdefault('p%d_blocks' % p, []).append(_u8(blocks, (len(blocks), 4)))
            rec.setdefault('p%d_task_attempts' % p, []).append(np.int32(f.task_attempts))
            rec.setdefault('p%d_block_attempts' % p, []).append(np.array(f.block_attempts, dtype=np.int32))
            if new_map and e < map_chips:
                m = np.array(mgr.m_degrade, dtype=np.float64)
                assert m.shape == (W, L)
                rec.setdefault('p%d_degrade' % p, []).append(m)
    out = {k: np.stack(v) for k, v in rec.items()}
    out['cfg'] = np.array([W, L, n, fov, nb, int(deg)], dtype=np.int64)
    out['per_degrade'] = np.float64(per)
    out['seed'] = np.uint64(seed)
    return out


def record_meda(rm, case, chips=N_CHIPS, map_chips=N_MAP_CHIPS):
    W, L, n, fov, version, deg, per, seed = case
    cls = rm.MEDAEnv_v0_2 if version == 2 else rm.MEDAEnv
    rec = {}
    for e in range(chips):
        f = MedaFeeder(seed, e, W, L)
        calls = []                                  # (is destination list, draws consumed) per _genLegalDroplet call
        legal = rm.RoutingTaskManager._genLegalDroplet

        def counted(self, dtype, _legal=legal, _f=f, _calls=calls):
            before = _f.draws
            _legal(self, dtype)
            _calls.append((dtype is self.destinations, _f.draws - before))

        for p in range(3):
            f.begin_task(p)
            del calls[:]
            f.begin_map(0 if (p == 0 and deg) else None)
            rm.RoutingTaskManager._genLegalDroplet = counted      # counts the calls; the reference's own code does the work
            try:
                with ref_shim.patch_generators(f):
                    if p == 0:
                        env = cls(W, L, n, fov=fov, b_degrade=deg, per_degrade=per)
                        mgr = env.routing_manager
                    else:
                        mgr.refresh()
            finally:
                rm.RoutingTaskManager._genLegalDroplet = legal
            assert f.idle() and f.map_calls == (2 if (deg and p == 0) else 0) and len(mgr.starts) == n
            dest = [d for is_dest, d in calls if is_dest]
            assert len(calls) - len(dest) == n and sum(d for _, d in calls) == f.draws
            rec.setdefault('p%d_starts' % p, []).append(_u8([(d.x_center, d.y_center) for d in mgr.starts], (n, 2)))
            rec.setdefault('p%d_ends' % p, []).append(_u8([(d.x_center, d.y_center) for d in mgr.destinations], (n, 2)))
            rec.setdefault('p%d_draws' % p, []).append(np.int32(f.draws))
            rec.setdefault('p%d_overlap_redraws' % p, []).append(np.int32(len(dest) - n))
            rec.setdefault('p%d_dest_redraws' % p, []).append(np.int32(sum(d - 1 for d in dest)))
            if p == 0 and deg and e < map_chips:
                m = np.array(env.m_degrade, dtype=np.float64)
                assert m.shape == (W, L)
                rec.setdefault('p0_degrade', []).append(m)
    out = {k: np.stack(v) for k, v in rec.items()}
    out['cfg'] = np.array([W, L, n, fov, version, int(deg)], dtype=np.int64)
    out['per_degrade'] = np.float64(per)
    out['seed'] = np.uint64(seed)
    return out


def save(name, arrays):
    """An .npz whose bytes depend on the arrays alone (np.savez stamps every member with the time of day)."""
    path = os.path.join(OUT, name + '.npz')
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    size = os.path.getsize(path)
    assert size < 400 * 1024, '%s: %d bytes' % (name, size)
    return size


def check_philox():
    """The pure-Python Philox above against the oracle's own (oracle/dmfb_oracle.c) on a few counters."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
    from oracle.dmfb_oracle import philox as c_philox
    for seed, ctr in [(0, (0, 0, 0, 0)), (5, (63, 2, 4095, (4 << 8) | 11)), (0xDEADBEEF12345678, (M32, M32, 7, 3 << 8))]:
        assert list(c_philox(seed & M32, seed >> 32, ctr)) == list(philox(seed, *ctr))


def main():
    check_philox()
    ref_shim.install()
    from env.DMFB import dmfb as rd
    from env.MEDA import meda as rm
    seen = dict(task64=0, block64=0, first=0, overlap=0, dest=0)
    for case in DMFB_CASES:
        g = record_dmfb(rd, case)
        ta = np.stack([g['p%d_task_attempts' % p] for p in range(3)])
        ba = np.stack([g['p%d_block_attempts' % p] for p in range(3)])
        worst = max(int(ta.max()), int(ba.max(initial=0)))
        assert worst < LOOP_MARGIN, 'a rejection loop of %d attempts is too close to the feeder limit' % worst
        counts = dict(task64=int((ta > 64).sum()), block64=int((ba > 64).any(axis=2).sum()), first=int((ta == 1).sum()))
        for k, v in counts.items():
            seen[k] += v
        size = save(dmfb_name(*case), g)
        print('%-40s %3d kB  largest attempt count %4d (blocks %3d)  generations accepted at task attempt >= 64: %3d, '
              'with a block at attempt >= 64: %3d, at task attempt 0: %3d  blocks per chip %d'
              % (dmfb_name(*case), size // 1000, int(ta.max()), int(ba.max(initial=0)), counts['task64'], counts['block64'],
                 counts['first'], g['p0_blocks'].shape[1]))
    for case in MEDA_CASES:
        g = record_meda(rm, case)
        dr = np.stack([g['p%d_draws' % p] for p in range(3)])
        ov = np.stack([g['p%d_overlap_redraws' % p] for p in range(3)])
        de = np.stack([g['p%d_dest_redraws' % p] for p in range(3)])
        assert int(dr.max()) < LOOP_MARGIN
        seen['overlap'] += int((ov > 0).sum())
        seen['dest'] += int((de > 0).sum())
        size = save(meda_name(*case), g)
        print('%-40s %3d kB  largest draw count %4d  generations with an isDropletOverlap redraw: %3d, '
              'with a destination redrawn in _genLegalDroplet: %3d'
              % (meda_name(*case), size // 1000, int(dr.max()), int((ov > 0).sum()), int((de > 0).sum())))
    print('required situations (chip generations):', seen)
    assert all(v > 0 for v in seen.values()), 'a required situation does not occur in the committed cases: %r' % seen


if __name__ == '__main__':
    main()
