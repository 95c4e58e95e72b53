"""No learn path reads memory that nothing wrote: every shipped GPU learn path, run from the same golden with clean allocations,
with every torch.empty / torch.empty_like of the process filled with pattern 'A' (NaN / 1 / True) and with pattern 'B'
(-777.25 / 2 / False) (tests/poison_alloc.py), must leave the same bits.

Per case: the learner is built and two consecutive learns are run (helpers and PATHS tables of tests/test_gpu_learn_f64.py,
test_gpu_td_lambda_learn.py, test_gpu_double_q_learn.py and their QMIX twins), the `with` block around set-up and learns alike.
After each learn: last_loss, last_grad_norm, the masked TD errors and the mask as the TD node's forward left them, the double-Q
picks, p.grad and p of every eval parameter (the mixer's too) and the moments of the fused clip + Adam step -- bit-equal (NaN-safe)
between the clean run and either poisoned run.  Every poisoned run must have poisoned allocations of the path's own call sites
(the GRU sequence node, the front-end node and the TD node the path is named for), so a case that fell back to another path and
poisoned nothing of interest fails.

Control: a second clean run must be bit-equal to the first.  Where it is not, that is a finding about determinism, and for that
case each poisoned run is held instead to the float64 restatement with the bound and factors of tests/test_gpu_learn_f64.py
(`learn_f64.compare_step`), which is measured against the reference, not against a path under test.  profiles/poisoned_alloc/NOTES.md
has the table of cases and what the tests found."""
import numpy as np
import pytest
import torch

import learn_f64
import poison_alloc as PA
import qmix_learn_f64 as Q
from qmix_helpers import F64_CASES, F64_PATHS, f64_case_agents, f64_case_learn, replay_batch
from test_gpu_double_q_learn import PATHS as DOUBLE_PATHS
from test_gpu_learn_f64 import PATHS as VDN_PATHS
from test_gpu_td_lambda_learn import PATHS as LAMBDA_PATHS
from vdn_helpers import learn_golden_setup, learn_golden_step

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHORT = 'vdn_learn_4d_od24_short.npz'
LAM = 0.8
assert set(LAMBDA_PATHS) == set(DOUBLE_PATHS) == {'fused_td', 'packed'} and all(LAMBDA_PATHS[p] == VDN_PATHS[p] for p in LAMBDA_PATHS)

# the autograd node of the HIP front end that serves a field of view (network/base_net.py: CRNN.features_obs_train)
FRONT = {5: '_FrontFovTrain', 7: '_FrontFovTrain', 9: '_Front9Train', 11: '_FrontWideTrain', 13: '_FrontWideTrain', 19: '_Front19Train'}
# path -> {package file: functions / classes that must have allocated under poison}
VDN_SITES = {'fused_td': {'network/base_net.py': {'_GRUSeqHip'}, 'policy/vdn.py': {'_td_forward', '_TDLoss'}},
             'host_len_bound': {'network/base_net.py': {'_GRUSeqHip'}, 'policy/vdn.py': {'_td_forward', '_TDLoss'}},
             'packed': {'network/base_net.py': {'_GRUSeqPairPacked'}, 'policy/vdn.py': {'_td_forward', '_TDLossPacked', '_packed_q_values'}},
             'packed_valu': {'network/base_net.py': {'_GRUSeqHipPacked'},
                             'policy/vdn.py': {'_td_forward', '_TDLossPacked', '_packed_q_values'}}}
QMIX_SITES = {'fused_ring': {'network/base_net.py': {'_GRUSeqHip'}, 'policy/qmix.py': {'_mix_forward', '_mix_backward', '_MixTD'}},
              'fused_two_tensors': {'network/base_net.py': {'_GRUSeqHip'}, 'policy/qmix.py': {'_mix_forward', '_mix_backward', '_MixTD'}},
              'torch_ops': {'network/base_net.py': {'_GRUSeqHip'}},
              'packed': {'network/base_net.py': {'_GRUSeqPairPacked'}, 'policy/vdn.py': {'_packed_q_values'},
                         'policy/qmix.py': {'_mix_forward', '_mix_backward', '_MixTDPacked', 'learn_packed'}},
              'packed_valu': {'network/base_net.py': {'_GRUSeqHipPacked'}, 'policy/vdn.py': {'_packed_q_values'},
                              'policy/qmix.py': {'_mix_forward', '_mix_backward', '_MixTDPacked', 'learn_packed'}}}


def _pair_env(monkeypatch, pair):
    if pair is not None:
        monkeypatch.setenv('MARL_DMFB_GRU_PAIR', pair)
    else:
        monkeypatch.delenv('MARL_DMFB_GRU_PAIR', raising=False)


def _spy_td(monkeypatch, seen):
    """The masked TD errors and the mask of every TD node's forward (policy/vdn.py: _td_forward, policy/qmix.py: _mix_forward),
    as tests/test_gpu_double_q_learn.py reads them."""
    from marl_dmfb_amd.policy import qmix, vdn
    for module, name in ((vdn, '_td_forward'), (qmix, '_mix_forward')):
        real = getattr(module, name)

        def forward(*a, _real=real, **k):
            out = _real(*a, **k)
            seen.append((out[0], out[1]))
            return out
        monkeypatch.setattr(module, name, forward)


def _snapshot(pol, seen, mixer):
    """Everything a caller can observe after one learn, on the host."""
    out = [('last_loss', pol.last_loss), ('last_grad_norm', torch.as_tensor(pol.last_grad_norm))]
    for k, (mtd, mask) in enumerate(seen):
        out += [('mtd[%d]' % k, mtd), ('mask[%d]' % k, mask)]
    del seen[:]
    if pol.double_picks:
        out.append(('double_picks', pol.double_picks[-1]))
    nets = [('', pol.eval_rnn)] + ([('mix.', pol.eval_qmix_net)] if mixer else [])
    for label, net in nets:
        for k, p in net.named_parameters():
            assert p.grad is not None, 'no gradient for %s%s' % (label, k)
            out += [('grad/%s%s' % (label, k), p.grad), ('w/%s%s' % (label, k), p)]
            if pol._adam is not None:
                out += [('adam_m/%s%s' % (label, k), pol._adam['m'][id(p)]), ('adam_v/%s%s' % (label, k), pol._adam['v'][id(p)])]
    return [(k, t.detach().cpu().clone()) for k, t in out]


def _tensors(snap, mixer):
    """(name, gradient, weights) of a snapshot as `learn_f64.compare_step` takes them."""
    d = dict(snap)
    names = [k[2:] for k, _ in snap if k.startswith('w/')]
    return [((Q.MIX + k[4:]) if mixer and k.startswith('mix.') else k, d['grad/' + k], d['w/' + k]) for k in names]


def _check(label, run, sites, envelope=None):
    """run(mode) -> (snapshots of the two learns, poison log or None).  envelope() -> (float64 envelope, factors(step), mixer) for
    the fall-back of a case whose control is not bit-equal, or None where the case has none."""
    clean, _ = run('clean')
    again, _ = run('clean')
    control = ['%s learn %d %s: %s' % (label, step, k, PA.first_difference(x, y))
               for step in range(2) for (k, x), (_, y) in zip(clean[step], again[step]) if not PA.bits_equal(x, y)]
    assert len(clean) == 2 and len(clean[0]) >= 2 + 2 * 10 and [k for k, _ in clean[0]] == [k for k, _ in again[0]]
    assert all(torch.isfinite(t).all() for snap in clean for k, t in snap if t.is_floating_point()), 'the clean run is not finite'
    bad = []
    for mode in ('A', 'B'):
        got, log = run(mode)
        seen = {f: log.functions_seen(f, names) for f, names in sites.items()}
        print('poisoned %-60s pattern %s: %4d allocations (%4d in the package), sites %s' % (
            label, mode, log.count, log.package_count(), ' '.join(sorted(log.sites))))
        assert log.package_count() > 0 and seen == sites, 'the path under test did not allocate where it should: %r, wanted %r' % (seen, sites)
        if control:
            assert envelope is not None, 'control not bit-equal and no float64 fall-back for this case:\n' + '\n'.join(control)
            env, factors, mixer = envelope()
            for step in range(2):
                d = dict(got[step])
                bad += learn_f64.compare_step('%s pattern %s' % (label, mode), step, env, float(d['last_grad_norm']),
                                              float(d['last_loss']), _tensors(got[step], mixer), factors(step))
            continue
        for step in range(2):
            assert [k for k, _ in got[step]] == [k for k, _ in clean[step]]
            for (k, x), (_, y) in zip(clean[step], got[step]):
                d = PA.first_difference(x, y)
                if d:
                    bad.append('%s pattern %s learn %d %s: %s' % (label, mode, step, k, d))
    if control:
        print('CONTROL NOT BIT-EQUAL (held to the float64 bound instead):\n' + '\n'.join(control))
    assert not bad, '\n'.join(bad)


# ------------------------------------------------------------------------------------------------------------------------ VDN
def _vdn_run(name, path, lam, double_q, monkeypatch):
    flags, pair = VDN_PATHS[path]
    golden = learn_f64.golden_path(name)

    def run(mode):
        _pair_env(monkeypatch, pair)
        seen = []
        _spy_td(monkeypatch, seen)
        try:
            with PA.run_mode(mode) as log:
                g, agents = learn_golden_setup(golden, DEV)
                pol = agents.policy
                pol.args.td_lambda, pol.args.double_q = lam, double_q      # after the set-up: the learner reads both at learn time
                if double_q:
                    pol.double_picks = []
                snaps = []
                for step in range(2):
                    learn_golden_step(g, agents, DEV, step, **flags)
                    snaps.append(_snapshot(pol, seen, False))
                pol.check_td_inputs()
        finally:
            monkeypatch.undo()
        return snaps, log
    return run


def _vdn_sites(name, path):
    fov = learn_f64.golden_config(np.load(learn_f64.golden_path(name)))[4]
    sites = {f: set(v) for f, v in VDN_SITES[path].items()}
    sites['network/base_net.py'].add(FRONT[fov])
    return sites


OPTIONS = [(0.0, False), (LAM, False), (0.0, True), (LAM, True)]
SHORT_CASES = [(path, lam, dq) for path in VDN_PATHS for lam, dq in OPTIONS if not dq or path in DOUBLE_PATHS]
assert len(SHORT_CASES) == 12


@pytest.mark.parametrize('path,lam,double_q', SHORT_CASES, ids=['%s-lam%g-double_%s' % (p, l, 'on' if d else 'off') for p, l, d in SHORT_CASES])
def test_vdn_learn_options_read_no_unwritten_memory(path, lam, double_q, monkeypatch):
    import td_lambda_f64
    envelope = None
    if not double_q:
        envelope = (lambda: (td_lambda_f64.envelope(learn_f64.golden_path(SHORT), lam), lambda s: td_lambda_f64.path_factors(SHORT, path, s),
                             False)) if lam else \
                   (lambda: (learn_f64.envelope(learn_f64.golden_path(SHORT)), lambda s: learn_f64.path_factors(SHORT, path, s), False))
    print()
    _check('vdn %s %s lam=%g double_q=%s' % (SHORT[:-4], path, lam, double_q), _vdn_run(SHORT, path, lam, double_q, monkeypatch),
           _vdn_sites(SHORT, path), envelope)


SHAPE_GOLDENS = ['vdn_learn_10d_od32.npz', 'vdn_learn_meda_4d_od32.npz'] + learn_f64.FOV_GOLDENS
SHAPE_CASES = [(name, path) for name in SHAPE_GOLDENS for path in ('packed', 'fused_td')]
assert len(learn_f64.FOV_GOLDENS) == 4


@pytest.mark.parametrize('name,path', SHAPE_CASES, ids=['%s-%s' % (n[:-4], p) for n, p in SHAPE_CASES])
def test_vdn_learn_shapes_read_no_unwritten_memory(name, path, monkeypatch):
    """The per-fov front ends (the zero tail of their x, their `part` / `tot` scratch), 10 droplets and MEDA's 9 actions."""
    print()
    _check('vdn %s %s' % (name[:-4], path), _vdn_run(name, path, 0.0, False, monkeypatch), _vdn_sites(name, path),
           lambda: (learn_f64.envelope(learn_f64.golden_path(name)), lambda s: learn_f64.path_factors(name, path, s), False))


# ----------------------------------------------------------------------------------------------------------------------- QMIX
def _qmix_run(spec, path, lam, double_q, monkeypatch):
    def run(mode):
        _pair_env(monkeypatch, F64_PATHS[path][2])
        seen = []
        _spy_td(monkeypatch, seen)
        try:
            with PA.run_mode(mode) as log:
                g = Q.load_spec(spec)
                agents = f64_case_agents(g, Q.spec_config(spec), path, DEV)
                pol = agents.policy
                pol.args.qmix_lambda, pol.args.qmix_double_q = lam, double_q
                if double_q:
                    pol.double_picks = []
                snaps = []
                for step in range(2):
                    f64_case_learn(g, agents, path, DEV, step)
                    snaps.append(_snapshot(pol, seen, True))
                pol.check_td_inputs()
        finally:
            monkeypatch.undo()
        return snaps, log
    return run


def _qmix_sites(spec, path):
    sites = {f: set(v) for f, v in QMIX_SITES[path].items()}
    sites['network/base_net.py'].add(FRONT[Q.spec_config(spec)[4]])
    return sites


@pytest.mark.parametrize('spec,path', F64_CASES, ids=['%s-%s' % c for c in F64_CASES])
def test_qmix_learn_reads_no_unwritten_memory(spec, path, monkeypatch):
    print()
    _check('qmix %s %s' % (spec, path), _qmix_run(spec, path, 0.0, False, monkeypatch), _qmix_sites(spec, path),
           lambda: (Q.qmix_envelope(spec), lambda s: Q.qmix_path_factors(spec, path, s), True))


QMIX_OPTIONS = [(path, lam, dq) for path in ('fused_ring', 'packed') for lam, dq in OPTIONS[1:]]


@pytest.mark.parametrize('path,lam,double_q', QMIX_OPTIONS, ids=['%s-lam%g-double_%s' % (p, l, 'on' if d else 'off') for p, l, d in QMIX_OPTIONS])
def test_qmix_learn_options_read_no_unwritten_memory(path, lam, double_q, monkeypatch):
    """args.qmix_lambda / args.qmix_double_q on qmix_learn_4d_od24.  (The learners never read args.stream_state, which only decides
    how the Trainer fills the ring that `qmix_helpers.replay_batch` stands in for, and `f64_case_agents` takes no such argument:
    there is no separate stream_state learn case to build.)"""
    print()
    _check('qmix qmix_learn_4d_od24 %s lam=%g double_q=%s' % (path, lam, double_q),
           _qmix_run('qmix_learn_4d_od24', path, lam, double_q, monkeypatch), _qmix_sites('qmix_learn_4d_od24', path))


# ------------------------------------------------------------------------------------------- a drawn batch with padded rows
def _draw(lens, n, pad=64):
    """The longest-first draw of the most episodes of a batch whose packed row count V = n x (valid steps) is no multiple of the
    row padding -> (slots, their lengths, V, Vp)."""
    order = np.argsort(-lens, kind='stable')
    for k in range(len(order), 1, -1):
        V = int(lens[order[:k]].sum()) * n
        if V % pad:
            return order[:k], lens[order[:k]], V, -(-V // pad) * pad
    raise AssertionError('no draw of this batch has a padded tail')


def _spy_rows(monkeypatch, rows):
    """(valid rows V, rows of the packed Q tensor) of every `VDN._packed_q_values`."""
    from marl_dmfb_amd.policy.vdn import VDN
    real = VDN._packed_q_values

    def packed_q_values(self, *a, **k):
        out = real(self, *a, **k)
        rows.append((int(out[3]) * self.n_agents, int(out[0].shape[0])))
        return out
    monkeypatch.setattr(VDN, '_packed_q_values', packed_q_values)


@pytest.mark.parametrize('learner', ['vdn', 'qmix'])
def test_packed_learn_of_a_draw_with_padded_rows_reads_no_unwritten_memory(learner, monkeypatch):
    """A draw whose V valid rows are no multiple of 64: rows [V:Vp) of every packed tensor exist, and only the tail fills and the
    kernels' own zero rows stand between them and the GEMMs."""
    from marl_dmfb_amd.policy import vdn
    name, spec = SHORT, 'qmix_learn_4d_od24'
    rows = []

    def run(mode):
        _pair_env(monkeypatch, '1')
        seen = []
        _spy_td(monkeypatch, seen)
        _spy_rows(monkeypatch, rows)
        try:
            with PA.run_mode(mode) as log:
                if learner == 'vdn':
                    g, agents = learn_golden_setup(learn_f64.golden_path(name), DEV)
                    batch = {k: torch.as_tensor(g[k]).to(DEV) for k in learn_f64.BATCH_KEYS}
                    batch['padded'], batch['terminated'], batch['r'] = batch['padded'].bool(), batch['terminated'].bool(), batch['r'].float()
                    for k in ('u', 'avail_u', 'avail_u_next', 'u_onehot', 'o', 'o_next'):
                        batch[k] = batch[k].to(torch.int8)
                else:
                    g = Q.load_spec(spec)
                    agents = f64_case_agents(g, Q.spec_config(spec), 'packed', DEV)
                    batch = replay_batch(g, DEV, True)
                pol = agents.policy
                assert pol.packed_ok(batch) is True
                lens = (~batch['padded'][:, :, 0]).sum(1).cpu().numpy()
                idx, ln, V, Vp = _draw(lens, pol.n_agents)
                assert Vp > V and V < vdn.PACK_ROWS * 16
                snaps = []
                for step in range(2):
                    pol.learn_packed(batch, idx, ln, step)
                    snaps.append(_snapshot(pol, seen, learner == 'qmix'))
                    assert rows[-1] == (V, Vp), (rows[-1], V, Vp)
                pol.check_td_inputs()
        finally:
            monkeypatch.undo()
        return snaps, log
    print()
    sites = _vdn_sites(name, 'packed') if learner == 'vdn' else _qmix_sites(spec, 'packed')
    _check('%s packed draw with padded rows' % learner, run, sites)
    assert rows and all(vp > v for v, vp in rows)
