"""Host side of the poisoned-allocation tests (tests/poison_alloc.py): the helper itself, the guard that keeps the package to the
two allocation calls the helper intercepts, and the CPU tensor-op learns of the smallest VDN and QMIX goldens under clean memory
and both patterns, bit for bit."""
import glob
import os
import re

import pytest
import torch

import poison_alloc as PA
from qmix_helpers import load_learn_golden, qmix_agents, replay_batch
from vdn_helpers import det_init, learn_golden_setup, learn_golden_step

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), 'marl_dmfb_amd')
# every dtype the package passes to torch.empty / torch.empty_like (grep dtype= in marl_dmfb_amd/), and the two 16-bit floats
DTYPES = [torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int8, torch.uint8, torch.int32, torch.int64, torch.bool]


# ------------------------------------------------------------------------------------------------------------------ the helper
@pytest.mark.parametrize('pattern', ['A', 'B'])
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d)[6:])
def test_every_dtype_is_filled_as_specified(pattern, dtype):
    with PA.poisoned(pattern) as log:
        a = torch.empty((3, 5), dtype=dtype)
        b = torch.empty_like(torch.zeros(7, dtype=dtype))
        c = torch.empty(4, 2, dtype=dtype)                       # sizes as positional integers
    assert log.count == 3 and a.dtype == b.dtype == c.dtype == dtype and a.shape == (3, 5) and b.shape == (7,) and c.shape == (4, 2)
    for t in (a, b, c):
        if dtype == torch.bool:
            assert bool(t.all()) if pattern == 'A' else not bool(t.any())
        elif dtype.is_floating_point:
            assert bool(torch.isnan(t).all()) if pattern == 'A' else bool((t == -777.25).all())     # -777.25 is exact in bfloat16 too
        else:
            assert bool((t == (1 if pattern == 'A' else 2)).all())


def test_integer_poison_is_small_and_non_negative():
    """A poisoned integer that a bug lets through as an index must stay inside every buffer of the GPU scenarios (at least 4 chips,
    3 droplets, 5 actions)."""
    for pattern in PA.PATTERNS:
        for dtype in (torch.int8, torch.uint8, torch.int32, torch.int64):
            assert 0 <= PA.fill_value(pattern, dtype) <= 2
    assert PA.fill_value('A', torch.int32) != PA.fill_value('B', torch.int32)


def test_zero_element_tensors_are_left_alone():
    with PA.poisoned('A') as log:
        a = torch.empty((0, 4))
        b = torch.empty_like(torch.zeros(0, dtype=torch.int32))
    assert log.count == 0 and a.shape == (0, 4) and b.numel() == 0


def test_originals_are_restored_also_after_an_exception():
    empty, empty_like = torch.empty, torch.empty_like
    with PA.poisoned('B'):
        assert torch.empty is not empty and torch.empty_like is not empty_like
    assert torch.empty is empty and torch.empty_like is empty_like
    with pytest.raises(KeyError):
        with PA.poisoned('A'):
            raise KeyError('inside')
    assert torch.empty is empty and torch.empty_like is empty_like
    with pytest.raises(ValueError):
        with PA.poisoned('C'):
            pass
    assert torch.empty is empty and torch.empty_like is empty_like


def test_counter_and_call_sites():
    from marl_dmfb_amd.policy.td_lambda import lambda_targets_torch
    q = torch.zeros(2, 3, 1, dtype=torch.float64)
    with PA.poisoned('A') as log:
        torch.empty(3)                                           # a caller outside the package: counted, no site
        assert log.count == 1 and log.sites == {}
        lambda_targets_torch(q, q, q, q, 0.99, 0.8)
    assert log.count == 2 and log.package_count() == 1
    (site,) = log.sites
    assert re.fullmatch(r'policy/td_lambda\.py:\d+', site) and log.files() == {'policy/td_lambda.py'}
    assert log.functions_seen('policy/td_lambda.py', {'lambda_targets_torch', 'check_lambda'}) == {'lambda_targets_torch'}
    with PA.poisoned('A', only={'nowhere.py:1'}) as log:         # narrowing: seen, not filled
        t = torch.empty(3)
        lambda_targets_torch(q, q, q, q, 0.99, 0.8)
    assert log.count == 0 and log.package_count() == 1 and not torch.isnan(t).any()


def test_bits_equal_is_nan_safe_and_sees_the_sign_of_zero():
    nan = torch.tensor([float('nan'), 1.0])
    assert PA.bits_equal(nan, nan.clone()) and PA.first_difference(nan, nan.clone()) == ''
    assert not PA.bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not PA.bits_equal(torch.tensor([1.0]), torch.tensor([1.0], dtype=torch.float64))
    assert 'first at (1,)' in PA.first_difference(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 3.0]))


# ------------------------------------------------------------------------------------------------------------ the source guard
# ways of getting uninitialised memory that `poisoned` does not intercept, and ways of reaching the two it does past the patch
BYPASSES = [r'\bnew_empty\b', r'\bempty_strided\b', r'\bresize_\b', r'\bresize_as_\b', r'\bempty_permuted\b', r'\bempty_quantized\b',
            r'\btorch\.Tensor\(', r'\btorch\.(cuda\.)?(Float|Double|Half|BFloat16|Byte|Char|Short|Int|Long|Bool)Tensor\(',
            r'\bfrom\s+torch\s+import\b.*\bempty', r'=\s*torch\.empty(_like)?\s*($|#)', r'\bnp\.empty\w*\(.*\bdevice\b']


def test_package_allocates_uninitialised_memory_only_through_the_two_intercepted_calls():
    found, intercepted = [], 0
    files = sorted(glob.glob(os.path.join(PKG, '**', '*.py'), recursive=True))
    assert len(files) > 10
    for path in files:
        with open(path) as fh:
            for ln, line in enumerate(fh, 1):
                intercepted += len(re.findall(r'\btorch\.empty(_like)?\b', line))
                for pat in BYPASSES:        # comments and docstrings are scanned too: naming a bypass there is rare enough to reword
                    if re.search(pat, line):
                        found.append('%s:%d: %s' % (os.path.relpath(path, PKG), ln, line.strip()))
    assert not found, 'uninitialised memory that tests/poison_alloc.py does not intercept:\n' + '\n'.join(found)
    assert intercepted >= 90          # the scan reads the package: 94 sites when this test was written


# -------------------------------------------------------------------------------------------------- CPU tensor-op learns
OPTIONS = [(0.0, False), (0.8, False), (0.0, True), (0.8, True)]
MODES = ['clean', 'A', 'B']


def _snapshot(pol, nets):
    out = [('loss', pol.last_loss.detach().clone()), ('grad_norm', torch.as_tensor(pol.last_grad_norm).detach().clone())]
    for label, net in nets:
        for k, p in net.named_parameters():
            out += [('%sgrad/%s' % (label, k), p.grad.detach().clone()), ('%sw/%s' % (label, k), p.detach().clone())]
    return out


def _vdn_cpu(mode, lam, double_q, host_len_bound=False):
    golden = os.path.join(HERE, 'golden', 'vdn_learn_4d_od24_short.npz')
    with PA.run_mode(mode) as log:
        g, agents = learn_golden_setup(golden, 'cpu')
        agents.policy.args.td_lambda, agents.policy.args.double_q = lam, double_q
        out = []
        for step in range(2):
            learn_golden_step(g, agents, 'cpu', step, host_len_bound=host_len_bound)
            out += _snapshot(agents.policy, [('', agents.policy.eval_rnn)])
    return out, log


def _qmix_cpu(mode, lam, double_q, ring_layout=True):
    g = load_learn_golden(os.path.join(HERE, 'golden', 'qmix_learn_4d_od24.npz'))
    W, L, n, fov = [int(v) for v in g['cfg'][:4]]
    with PA.run_mode(mode) as log:
        agents = qmix_agents(W, L, n, fov, 'cpu')
        pol = agents.policy
        pol.args.qmix_lambda, pol.args.qmix_double_q = lam, double_q
        det_init(pol.eval_rnn)
        det_init(pol.target_rnn, salt=0.5)
        det_init(pol.eval_qmix_net, salt=0.3)
        pol.target_qmix_net.load_state_dict(pol.eval_qmix_net.state_dict())
        out = []
        for step in range(2):
            agents.train(replay_batch(g, 'cpu', ring_layout), step)
            out += _snapshot(pol, [('', pol.eval_rnn), ('mix.', pol.eval_qmix_net)])
    return out, log


# the paths of tests/test_vdn_learn_golden.py and tests/test_qmix_learn_golden.py on the CPU
LEARNERS = {'vdn': _vdn_cpu, 'vdn_host_len_bound': lambda *a: _vdn_cpu(*a, host_len_bound=True),
            'qmix_ring_views': _qmix_cpu, 'qmix_two_tensors': lambda *a: _qmix_cpu(*a, ring_layout=False)}


@pytest.mark.parametrize('lam,double_q', OPTIONS, ids=['lam%g-double_%s' % (l, 'on' if d else 'off') for l, d in OPTIONS])
@pytest.mark.parametrize('learner', list(LEARNERS))
def test_cpu_learn_is_bit_equal_under_clean_and_poisoned_memory(learner, lam, double_q):
    run = LEARNERS[learner]
    threads = torch.get_num_threads()
    torch.set_num_threads(min(threads, 8))       # one thread count for the three runs (the float32 GEMMs split their sums by it)
    try:
        runs = {mode: run(mode, lam, double_q) for mode in MODES}
    finally:
        torch.set_num_threads(threads)
    clean = runs['clean'][0]
    assert len(clean) >= 2 * (2 + 2 * 10)
    bad = []
    for mode in ('A', 'B'):
        out, log = runs[mode]
        assert log.count > 0
        if lam:
            assert 'policy/td_lambda.py' in log.files()          # the one torch.empty_like of the CPU learn path
        assert [k for k, _ in out] == [k for k, _ in clean]
        for (k, x), (_, y) in zip(clean, out):
            d = PA.first_difference(x, y)
            if d:
                bad.append('%s pattern %s %s: %s' % (learner, mode, k, d))
    assert not bad, '\n'.join(bad)
