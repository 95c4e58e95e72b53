"""The CPU oracles' task, block and degrade-map GENERATORS against the reference's own.

Every other env golden injects tasks, blocks and maps, so gen_start_end / gen_blocks / gen_degrade (oracle/dmfb_oracle.c)
and gen_task / the degrade loop (oracle/meda_oracle.c) were only ever compared with their HIP twins.  The recordings
tests/golden/gen_*.npz hold what the reference's _Generate_Start_End, GenRandomBlocks, _random_health_statue
(env/DMFB/dmfb.py:157-251), addTask, _genLegalDroplet, getRandomYX and MEDAEnv.__init__'s degrade map
(env/MEDA/meda.py:175-233, :497-502) accepted when fed the candidate stream of DESIGN.md section 4
(tools/oracle/gen_generator_golden.py).  The oracles, built on the recorded seed with 64 chips from env id 0, must hold
the same starts, ends, blocks (integers) and degrade maps (float64 bit patterns) after construction and after each of
two resets; for DMFB the second is reset(new=True), which draws the map of rng_map 1.

The live test re-runs the feeder against the reference where the reference is present, so a stale recording cannot
hide drift between the reference and the oracle."""
import os
import sys

import numpy as np
import pytest

import generator_golden as gg

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'oracle')


def test_committed_cases_are_all_there():
    assert gg.committed('dmfb') == sorted(gg.DMFB_FILES) and gg.committed('meda') == sorted(gg.MEDA_FILES)


def test_recordings_hold_the_required_situations():
    """What the issue asks of the inputs: the kernels test 64 attempts per wave round, so some accepted task attempt and
    some accepted block attempt has index >= 64 and some chip is accepted at attempt 0; both MEDA redraw loops are taken;
    the density rule's case has no blocks; the map of reset(new=True) is a new one; nothing near the feeder's 4096."""
    d = [gg.load(n) for n in gg.DMFB_FILES]
    ta = np.concatenate([g['p%d_task_attempts' % p] for g in d for p in range(3)])
    ba = np.concatenate([g['p%d_block_attempts' % p].ravel() for g in d for p in range(3)])
    assert (ta > 64).any() and (ba > 64).any() and (ta == 1).any() and max(ta.max(), ba.max()) < 2048
    assert gg.load('gen_dmfb_10x10_4d_fov9_6b_s6')['p0_blocks'].shape == (64, 0, 4)
    for g in d:
        if 'p0_degrade' in g:
            assert not np.array_equal(g['p0_degrade'], g['p2_degrade'])
            assert (g['p0_degrade'] == 1.0).any() and (g['p0_degrade'] < 1.0).any()
    m = [gg.load(n) for n in gg.MEDA_FILES]
    assert all((g['p%d_overlap_redraws' % p] > 0).any() and (g['p%d_dest_redraws' % p] > 0).any() for g in m for p in range(3))
    assert max(g['p%d_draws' % p].max() for g in m for p in range(3)) < 2048
    assert any('p0_degrade' in g for g in m)


@pytest.mark.parametrize('name', gg.DMFB_FILES)
def test_dmfb_oracle_generates_what_the_reference_accepts(name):
    from oracle.dmfb_oracle import DmfbOracle
    g = gg.load(name)
    gg.walk_dmfb(DmfbOracle(env_id0=0, **gg.dmfb_kwargs(g)), g)


@pytest.mark.parametrize('name', gg.MEDA_FILES)
def test_meda_oracle_generates_what_the_reference_accepts(name):
    from oracle.meda_oracle import MedaOracle
    g = gg.load(name)
    gg.walk_meda(MedaOracle(env_id0=0, **gg.meda_kwargs(g)), g)


def _stepper(O):
    def step(a):
        term = O.step(a)[1].all(axis=1).astype(np.uint8)
        O.reset(mask=term)
        return term
    return step


def test_oracle_masked_resets_draw_the_reference_tasks():
    """The walk tests/test_gpu_generator_golden.py takes through the step kernel's autoreset, on the oracles."""
    from oracle.dmfb_oracle import DmfbOracle
    from oracle.meda_oracle import MedaOracle
    g = gg.load(gg.DMFB_AUTORESET)
    O = DmfbOracle(env_id0=0, **gg.dmfb_kwargs(g))
    gg.autoreset_walk(O, g, _stepper(O), gg.dmfb_toward, True, gg.DMFB_AUTORESET_STEPS)
    g = gg.load(gg.MEDA_AUTORESET)
    O = MedaOracle(env_id0=0, **gg.meda_kwargs(g))
    gg.autoreset_walk(O, g, _stepper(O), gg.meda_toward, False, gg.MEDA_AUTORESET_STEPS)


@pytest.fixture
def reference():
    """The reference's env modules, imported from where they lie (tools/oracle/ref_shim.py); the import path, the
    module table and the patched random functions are as before once the test is over."""
    path, modules = list(sys.path), set(sys.modules)
    sys.path.insert(0, TOOLS)
    try:
        import ref_shim
        if not os.path.isdir(ref_shim.REFERENCE_ROOT):
            pytest.skip('the reference is not on this machine')
        import gen_generator_golden as gen
        ref_shim.install()
        from env.DMFB import dmfb as rd
        from env.MEDA import meda as rm
        yield gen, rd, rm
        ref_shim.install.done = False
    finally:
        sys.path[:] = path
        for k in set(sys.modules) - modules:
            del sys.modules[k]


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def test_live_reference_dmfb(reference):
    import random
    from oracle.dmfb_oracle import DmfbOracle
    gen, rd, rm = reference
    before = (np.random.randint, np.random.rand, random.randrange, random.randint)
    for case in [c for c in gen.DMFB_CASES if gen.dmfb_name(*c) in ('gen_dmfb_12x9_3d_fov7_2b_s3', 'gen_dmfb_10x10_4d_fov9_4b_s2')]:
        g = gen.record_dmfb(rd, case)
        _same({k: np.asarray(v) for k, v in g.items()}, gg.load(gen.dmfb_name(*case)))     # the committed file is current
        gg.walk_dmfb(DmfbOracle(env_id0=0, **gg.dmfb_kwargs(g)), g)
    # a degrade case on a seed that is in no file, small enough to keep every chip's map (W != L, rng_map 0 and 1)
    g = gen.record_dmfb(rd, (9, 12, 3, 5, 2, True, 0.5, 99), chips=gg.N_CHIPS, map_chips=gg.N_CHIPS)
    gg.walk_dmfb(DmfbOracle(env_id0=0, **gg.dmfb_kwargs(g)), g)
    assert before == (np.random.randint, np.random.rand, random.randrange, random.randint)


def test_live_reference_meda(reference):
    import random
    from oracle.meda_oracle import MedaOracle
    gen, rd, rm = reference
    before = (np.random.randint, np.random.rand, random.randrange, random.randint)
    for case in [c for c in gen.MEDA_CASES if gen.meda_name(*c) in ('gen_meda_v0_30x30_4d_fov19_s11', 'gen_meda_v0_45x30_6d_fov9_s13')]:
        g = gen.record_meda(rm, case)
        _same({k: np.asarray(v) for k, v in g.items()}, gg.load(gen.meda_name(*case)))
        gg.walk_meda(MedaOracle(env_id0=0, **gg.meda_kwargs(g)), g)
    g = gen.record_meda(rm, (30, 45, 5, 9, 0, True, 0.5, 98), chips=gg.N_CHIPS, map_chips=gg.N_CHIPS)
    gg.walk_meda(MedaOracle(env_id0=0, **gg.meda_kwargs(g)), g)
    assert before == (np.random.randint, np.random.rand, random.randrange, random.randint)
