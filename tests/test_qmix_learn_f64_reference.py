"""The float64 ground truth of the QMIX learns (tests/qmix_learn_f64.py) is tied to the reference, and the reference's own float32
noise on each batch is measured, all on the CPU.

  * on the two reference goldens the restatement in float32 AND in float64 reproduces loss, gradient norm, the sampled CRNN
    tensors and the mixer tensors (in full or at `midx/`) under exactly the rule of `qmix_helpers.qmix_learn_golden_check`
    (`qmix_check_sampled`: rtol 1e-5, atol 1e-5 x max|ref|, weights atol 2e-6 / 1e-5);
  * the envelope E_ref[batch][step][tensor] exists on all five batches, the three with synthetic states included: max|x64| > 0
    and E_ref > 0 for every gradient, weight tensor, norm and loss of both learns;
  * a permuted episode order in float64 gives the identity order's numbers to rounding;
  * the gap the full-tensor check closes is real: a defect of 1e-3 x max|g| in one element of hyper_w1.0.weight between the
    samples of the 10-droplet golden passes the sampled rule and fails the full one, at that tensor only.

tests/test_gpu_qmix_learn_f64.py holds every shipped QMIX learn path on the GPU to 2 x E_ref per whole tensor."""
import numpy as np
import pytest
import torch

import learn_f64
import qmix_learn_f64 as Q
from qmix_helpers import qmix_check_sampled


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('spec', Q.REFERENCE_GOLDENS)
def test_restatement_reproduces_the_golden(spec, dtype):
    env = Q.qmix_envelope(spec)
    result = env['runs32'][0] if dtype == torch.float32 else env['ref']     # runs32[0]: the episodes in the golden's order
    g = Q.load_spec(spec)['qmix']
    for step in range(2):
        crnn, mix = Q.split_tensors(result[step])
        assert len(crnn) == len(g['names']) and len(mix) == len(g['mixer_names']) == 14
        assert all(t.dtype == dtype for _, grad, w in crnn + mix for t in (grad, w))
        qmix_check_sampled(g, step, result[step]['loss'], result[step]['grad_norm'], crnn, mix, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('spec', list(Q.SPECS))
def test_reference_noise_envelope_is_defined(spec):
    env = Q.qmix_envelope(spec)
    assert len(env['runs32']) == learn_f64.N_ORDERS == 5
    kind, W, L, n, fov, hh, clip, A, S = Q.spec_config(spec)
    for step in range(2):
        ref, E = env['ref'][step], env['E'][step]
        assert ref['grad'][Q.MIX + 'hyper_w1.0.weight'].shape == (hh, S)
        assert ref['grad'][Q.MIX + 'hyper_w1.2.weight'].shape == (n * Q.QMIX_HIDDEN, hh)
        assert ref['grad']['fc1.weight'].shape == (A, learn_f64.HIDDEN)
        for kind_ in ('grad', 'w'):
            assert list(E[kind_]) == list(ref[kind_]) and sum(k.startswith(Q.MIX) for k in E[kind_]) == 14
            for tensor, x64 in ref[kind_].items():
                assert x64.dtype == torch.float64 and float(x64.abs().max()) > 0, (kind_, tensor)
                assert E[kind_][tensor] > 0, (step, kind_, tensor)
        for kind_ in ('grad_norm', 'loss'):
            assert abs(ref[kind_]) > 0 and E[kind_] > 0, (step, kind_)


@pytest.mark.parametrize('spec', ['meda_4d_od32', 'fov5_4d_od24', 'fov13_3d_od32'])
def test_synthetic_states_are_what_the_docstring_says(spec):
    g = Q.load_spec(spec)
    s, s_next = g['s'], g['s_next']
    assert s.dtype == np.int8 and np.array_equal(s[:, 1:], s_next[:, :-1])
    nz = s[s != 0]
    assert 0.025 < nz.size / s.size < 0.035 and nz.min() == -10 and nz.max() == 10
    assert 0.03 < (nz < 0).mean() < 0.07
    valid = g['padded'][:, :, 0] == 0
    assert (s[valid] < 0).any() and (s_next[valid] < 0).any()          # negative entries reach steps that count


def test_permuted_episode_order_is_the_same_mathematics():
    """In float64 a permuted batch gives the identity order's numbers to rounding: the permutations of the envelope change the
    float32 summation order and nothing else, the states included."""
    spec = 'fov13_3d_od32'
    ref = Q.qmix_envelope(spec)['ref']
    order = learn_f64.episode_orders(Q.load_spec(spec)['o'].shape[0])[1]
    perm = Q.qmix_reference_learn(spec, torch.float64, order)
    for step in range(2):
        assert learn_f64.scalar_error(perm[step]['loss'], ref[step]['loss']) < 1e-13
        for tensor, x64 in ref[step]['grad'].items():
            assert learn_f64.full_error(perm[step]['grad'][tensor], x64)[0] < 1e-11, (step, tensor)


def test_sampled_check_is_blind_where_the_full_check_is_not():
    spec = 'qmix_learn_10d_od32'
    env, g = Q.qmix_envelope(spec), Q.load_spec(spec)['qmix']
    ref = env['ref'][0]
    tensor = 'hyper_w1.0.weight'
    sampled = set(g['midx/' + tensor].tolist())
    assert g['mgrad0/' + tensor].shape == (len(sampled),) and len(sampled) < ref['grad'][Q.MIX + tensor].numel()
    flat = min(set(range(ref['grad'][Q.MIX + tensor].numel())) - sampled)           # the first element the golden does not hold
    grads = {k: v.clone() for k, v in ref['grad'].items()}
    grads[Q.MIX + tensor].view(-1)[flat] += 1e-3 * float(ref['grad'][Q.MIX + tensor].abs().max())
    # the norm such a defect would report: the clipped gradients scale the norm before clipping
    total = lambda d: float(sum((v ** 2).sum() for v in d.values())) ** 0.5
    norm = ref['grad_norm'] * total(grads) / total(ref['grad'])
    defect = {'grad': grads, 'w': ref['w']}
    qmix_check_sampled(g, 0, ref['loss'], norm, *Q.split_tensors(defect), rtol=1e-5, atol=1e-5)            # accepted
    tensors = lambda r: [(k, r['grad'][k], r['w'][k]) for k in r['grad']]
    bad = learn_f64.compare_step('meta', 0, env, norm, ref['loss'], tensors(defect))                 # every row at learn_f64.FACTOR
    assert len(bad) == 1 and 'grad/' + Q.MIX + tensor in bad[0], bad                                # rejected, and only there
    assert learn_f64.compare_step('meta', 0, env, ref['grad_norm'], ref['loss'], tensors(ref)) == []


def test_the_factor_table_names_real_rows_and_keeps_its_limit():
    """QMIX_FACTORS: every entry is a case of the GPU test and a tensor of that batch, every factor a power of two above
    learn_f64.FACTOR, and no tensor's is above 16."""
    from qmix_helpers import F64_CASES
    for spec, by_path in Q.QMIX_FACTORS.items():
        tensors = Q.qmix_envelope(spec)['ref'][0]['grad']
        for (path, step), rows in by_path.items():
            assert (spec, path) in F64_CASES and step in (0, 1), (spec, path, step)
            assert rows is Q.qmix_path_factors(spec, path, step)
            for what, factor in rows.items():
                assert factor > learn_f64.FACTOR and factor == 2 ** int(np.log2(factor)), (spec, path, step, what)
                if what not in ('loss', 'grad_norm'):
                    kind, tensor = what.split('/', 1)
                    assert kind in ('grad', 'w') and tensor in tensors and factor <= Q.MAX_TENSOR_FACTOR, (spec, path, step, what)
    assert Q.qmix_path_factors('fov13_3d_od32', 'no such path', 0) == {}
