"""The HIP envs' task, block and degrade-map generators (csrc/dmfb_kernels.h gen_task_wave / gen_blocks_wave /
degrade_of, csrc/meda_kernels.h) against what the REFERENCE's own generators accepted on the same candidate stream
(tests/golden/gen_*.npz, tools/oracle/gen_generator_golden.py; see tests/test_generator_golden.py for the CPU side).
The other GPU parity tests compare these kernels with the CPU oracle only; here nothing but the recordings is read.

VecDMFB / VecMEDA on the recorded seed with 64 chips must return the recorded starts, ends, blocks (integers) and degrade
maps (float64 bit patterns) after construction, after reset() and after a further reset -- reset(new=True) for DMFB, the
facade's refresh(new=True), which draws the map of rng_map 1 -- in both DMFB launch shapes.  The reset inside the step
kernel (autoreset) is pinned too: a chip that has terminated c times holds the recorded task of rng_ep = c."""
import numpy as np
import pytest
import torch

import generator_golden as gg

pytestmark = pytest.mark.gpu

SHAPES = ['fused', 'split']


def _shape(monkeypatch, shape):
    if shape == 'split':        # step-only launch + observation kernel, as test_lockstep_blocks_split_launch forces it
        monkeypatch.setenv('DMFB_VEC_SPLIT_MIN_ENVS', '1')
    else:
        monkeypatch.delenv('DMFB_VEC_SPLIT_MIN_ENVS', raising=False)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('name', gg.DMFB_FILES)
def test_dmfb_kernels_generate_what_the_reference_accepts(name, shape, monkeypatch):
    from vec_adapter import make_vec
    _shape(monkeypatch, shape)
    g = gg.load(name)
    gg.walk_dmfb(make_vec(**gg.dmfb_kwargs(g)), g)


@pytest.mark.parametrize('name', gg.MEDA_FILES)
def test_meda_kernels_generate_what_the_reference_accepts(name):
    from vec_adapter import MedaAdapter
    g = gg.load(name)
    gg.walk_meda(MedaAdapter(**gg.meda_kwargs(g)), g)


def _stepper(V, **kw):
    def step(a):
        V.step(torch.as_tensor(a).cuda(), autoreset=True, **kw)
        return V.last_info['terminated']
    return step


@pytest.mark.parametrize('shape', SHAPES)
def test_dmfb_step_kernel_autoreset_draws_the_reference_task(shape, monkeypatch):
    from vec_adapter import make_vec
    _shape(monkeypatch, shape)
    g = gg.load(gg.DMFB_AUTORESET)
    V = make_vec(**gg.dmfb_kwargs(g))
    gg.autoreset_walk(V, g, _stepper(V, record=True), gg.dmfb_toward, True, gg.DMFB_AUTORESET_STEPS)


def test_meda_step_kernel_autoreset_draws_the_reference_task():
    from vec_adapter import MedaAdapter
    g = gg.load(gg.MEDA_AUTORESET)
    V = MedaAdapter(**gg.meda_kwargs(g))
    gg.autoreset_walk(V, g, _stepper(V), gg.meda_toward, False, gg.MEDA_AUTORESET_STEPS)
