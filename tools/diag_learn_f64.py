"""The experiments behind profiles/learn_f64/NOTES.md, so that a factor of tests/learn_f64.py: FACTORS can be derived again when a
kernel changes.  Diagnostics, not tests: they print figures and assert nothing.

  python tools/diag_learn_f64.py cpu [golden.npz ...]   no GPU.  Per golden: (a) leave-one-out ratios of the envelope's five
        float32 runs (how independent the five episode orders are); (b) the float32 restatement on 1, 3 and 16 intra-op threads
        against E_ref (what another summation order of the reference's own arithmetic does); (c) the float32 restatement with the
        GRU kernels' sigmoid 1 / (1 + exp2(-x log2 e)) in place of torch.sigmoid.
  python tools/diag_learn_f64.py gpu [golden.npz ...]   MI355X.  Stage swaps on the first learn: the float32 GEMMs of the eval
        network's linear layers (`_LinearSplitK` forward x W^T, backward g W and `_wgrad_splitk` g^T x) replaced by float64
        products of the same float32 operands, only the weight-gradient products replaced, and the HIP GRU kernels replaced by
        the per-step aten cell (padded path).  Prints err / E_ref and relL2 / E_ref(relL2) of every gradient tensor for the
        padded path, the packed path on the matrix cores and the packed path on the VALU kernels.
  python tools/diag_learn_f64.py qmix [batch ...] [path ...]   MI355X.  The same swaps on the first learn of the QMIX cases
        (tests/qmix_learn_f64.py: SPECS, tests/qmix_helpers.py: F64_PATHS), and with them or alone the mixer's own GEMMs: F.linear
        of `QMIX._first_layers` (forward, g W, g^T x) and the three z^T x products of the mixing / TD autograd nodes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import learn_f64 as L


def _short(t):
    return t.replace('weight', 'w').replace('bias', 'b')


def cpu(names):
    log2e = torch.tensor(1.4426950408889634, dtype=torch.float32)
    sigmoid = torch.sigmoid

    def fast_sigmoid(x):
        return sigmoid(x) if x.dtype != torch.float32 else 1.0 / (1.0 + torch.exp2((-x) * log2e))

    for name in names:
        path = L.golden_path(name)
        env = L.envelope(path)
        ref, runs = env['ref'], env['runs32']
        loo = []
        for step in range(2):
            for kind in ('grad', 'w'):
                for t, x64 in ref[step][kind].items():
                    errs = [L.full_error(r[step][kind][t], x64)[0] for r in runs]
                    loo += [errs[k] / max(e for i, e in enumerate(errs) if i != k) for k in range(len(errs))]
        loo = np.sort(np.array(loo))
        print('%s leave-one-out err / max(other four): median %.2f  99%% %.2f  max %.2f' % (name, np.median(loo), loo[int(.99 * len(loo))], loo[-1]))
        for step in range(2):
            print('   losses of the five runs, learn %d: %s' % (step, ' '.join('%.9g' % r[step]['loss'] for r in runs)))
        for threads in (1, 3, 16):
            L.THREADS = threads
            try:
                run = L.reference_learn(path, torch.float32)
            finally:
                L.THREADS = 8
            ratios = {(s, k, t): L.full_error(run[s][k][t], x64)[0] / env['E'][s][k][t]
                      for s in range(2) for k in ('grad', 'w') for t, x64 in ref[s][k].items()}
            over = ['learn %d %s/%s %.2f' % (s, k, _short(t), r) for (s, k, t), r in ratios.items() if r > L.FACTOR]
            print('   %2d threads: largest err / E_ref %.2f; above %g: %s' % (threads, max(ratios.values()), L.FACTOR, ', '.join(over) or 'none'))
        torch.sigmoid = fast_sigmoid
        try:
            run = L.reference_learn(path, torch.float32)
        finally:
            torch.sigmoid = sigmoid
        print('   exp2 sigmoid, first learn, relL2 / E_ref(relL2): ' + '  '.join(
            '%s %.2f' % (_short(t), L.full_error(run[0]['grad'][t], x64)[1] / env['E_l2'][0]['grad'][t]) for t, x64 in ref[0]['grad'].items()))


def _crnn_swaps():
    """swap(variant): 'wgrad64' / 'linear64' put float64 products of the same float32 operands in the place of the weight-gradient
    GEMM / of all three GEMMs of `_LinearSplitK`; anything else restores the shipped ones."""
    from marl_dmfb_amd.network import base_net
    shipped = (base_net._wgrad_splitk, base_net._LinearSplitK.forward, base_net._LinearSplitK.backward)

    def wgrad64(g2d, x2d):
        return torch.matmul(g2d.double().t(), x2d.double()).float()

    def forward64(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        y = torch.matmul(x.double(), weight.double().t())
        return (y if bias is None else y + bias.double()).float()

    def backward64(ctx, g):
        x, w = ctx.saved_tensors
        gx = torch.matmul(g.double(), w.double()).float() if ctx.needs_input_grad[0] else None
        return gx, wgrad64(g, x), (g.double().sum(0).float() if ctx.has_bias else None)

    def swap(variant):
        base_net._wgrad_splitk = wgrad64 if variant in ('wgrad64', 'linear64') else shipped[0]
        base_net._LinearSplitK.forward = staticmethod(forward64 if variant == 'linear64' else shipped[1])
        base_net._LinearSplitK.backward = staticmethod(backward64 if variant == 'linear64' else shipped[2])
    return swap


def gpu(names):
    from vdn_helpers import learn_golden_setup, learn_golden_step
    swap = _crnn_swaps()

    def run(name, label, variant, packed, pair):
        swap(variant)
        os.environ['MARL_DMFB_GRU_PAIR'] = pair
        path = L.golden_path(name)
        env = L.envelope(path)
        g, agents = learn_golden_setup(path, 'cuda:0')
        if variant == 'aten_gru':
            agents.policy.eval_rnn.gru_impl = agents.policy.target_rnn.gru_impl = 'aten'
        learn_golden_step(g, agents, 'cuda:0', 0, replay_dtypes=True, packed=packed)
        cells = []
        for t, p in agents.policy.eval_rnn.named_parameters():
            err, l2, _ = L.full_error(p.grad, env['ref'][0]['grad'][t])
            cells.append('%s %.2f/%.2f' % (_short(t), err / env['E'][0]['grad'][t], l2 / env['E_l2'][0]['grad'][t]))
        print('%-28s %-11s %-9s %s' % (name, label, variant, '  '.join(cells)), flush=True)

    for name in names:
        for label, packed, pair in (('padded', False, '1'), ('packed', True, '1'), ('packed_valu', True, '0')):
            for variant in ('shipped', 'wgrad64', 'linear64') + (('aten_gru',) if not packed else ()):
                run(name, label, variant, packed, pair)


def qmix(cases):
    """First learn of the QMIX cases of tests/test_gpu_qmix_learn_f64.py with float64 products of the same float32 operands in
    the place of: the GEMMs of `_LinearSplitK` (crnn64); the mixer's GEMMs (mixer64: the first-layer GEMM of `QMIX._first_layers`
    with its backward and the three z^T x products of `_MixTD` / `_MixTDPacked`, on the torch-op path the Linear layers and the
    two bmm's of QMixNet); both (all64).  For the shipped learn a second line holds the weights after the Adam step against the
    float64 Adam step of the path's OWN float32 gradient, in units of E_ref: what is left of a weight row's excess once the
    gradient's float32 noise is taken out of it."""
    import torch.nn.functional as F
    import qmix_learn_f64 as Q
    from qmix_helpers import F64_PATHS, f64_case_agents, f64_case_learn
    from marl_dmfb_amd.policy.qmix import QMIX
    swap = _crnn_swaps()
    shipped_first, shipped_mm, shipped_bmm = QMIX.__dict__['_first_layers'], torch.Tensor.mm, torch.bmm

    def linear64(x, weight, bias):
        return F.linear(x.double(), weight.double(), bias.double()).float()

    def first64(net, rows):
        layers = net.first_layers()
        return linear64(rows, torch.cat([m.weight for m in layers]), torch.cat([m.bias for m in layers]))

    def mm64(a, b):          # Tensor.mm is called by the two autograd nodes of policy/qmix.py only, torch.bmm by QMixNet only
        return shipped_mm(a.double(), b.double()).float() if a.dtype == torch.float32 else shipped_mm(a, b)

    def bmm64(a, b):
        return shipped_bmm(a.double(), b.double()).float() if a.dtype == torch.float32 else shipped_bmm(a, b)

    def cells_of(tensors, kind, ref, env, tally=None):
        cells, ratios = [], []
        for t, x in tensors:
            err, l2, _ = L.full_error(x, ref[t])
            ratios.append(err / env['E'][0][kind][t])
            cells.append('%s %.2f/%.2f' % (_short(t), ratios[-1], l2 / env['E_l2'][0][kind][t]))
        if tally is not None:
            rows, over, worst = above.get(tally, (0, 0, 0.0))
            above[tally] = (rows + len(ratios), over + sum(r > L.FACTOR for r in ratios), max([worst] + ratios))
        return max(ratios), '  '.join(cells)

    above = {}
    for spec, path in cases:
        env, g = Q.qmix_envelope(spec), Q.load_spec(spec)
        for variant in ('shipped', 'crnn64', 'mixer64', 'all64'):
            swap('linear64' if variant in ('crnn64', 'all64') else 'shipped')
            mixer64 = variant in ('mixer64', 'all64')
            pair = F64_PATHS[path][2]
            os.environ.pop('MARL_DMFB_GRU_PAIR', None)
            if pair is not None:
                os.environ['MARL_DMFB_GRU_PAIR'] = pair
            try:
                agents = f64_case_agents(g, Q.spec_config(spec), path, 'cuda:0')
                pol = agents.policy
                named = list(pol.eval_rnn.named_parameters()) + [(Q.MIX + k, p) for k, p in pol.eval_qmix_net.named_parameters()]
                w0 = {t: p.detach().double().clone() for t, p in named}
                if mixer64:
                    QMIX._first_layers, torch.Tensor.mm, torch.bmm = staticmethod(first64), mm64, bmm64
                    for net in (pol.eval_qmix_net, pol.target_qmix_net):
                        for m in net.modules():
                            if isinstance(m, torch.nn.Linear):
                                m.forward = lambda x, m=m: linear64(x, m.weight, m.bias)
                f64_case_learn(g, agents, path, 'cuda:0', 0)
            finally:
                swap('shipped')
                QMIX._first_layers, torch.Tensor.mm, torch.bmm = shipped_first, shipped_mm, shipped_bmm
            worst, cells = cells_of([(t, p.grad) for t, p in named], 'grad', env['ref'][0]['grad'], env, 'grad, ' + variant)
            print('%-20s %-17s %-8s grad worst %5.2f | %s' % (spec, path, variant, worst, cells), flush=True)
            if variant == 'shipped':
                worst, cells = cells_of([(t, p) for t, p in named], 'w', env['ref'][0]['w'], env, 'w, shipped')
                print('%-20s %-17s %-8s w    worst %5.2f | %s' % (spec, path, variant, worst, cells), flush=True)
                # Adam's first step on the path's own clipped gradient, in float64: w0 - lr g / (|g| + eps)
                group = pol.optimizer.param_groups[0]
                own = {t: (w0[t] - group['lr'] * p.grad.double() / (p.grad.double().abs() + group['eps'])).cpu() for t, p in named}
                worst, cells = cells_of([(t, p) for t, p in named], 'w', own, env, 'w against the float64 Adam step of the own gradient')
                print('%-20s %-17s %-8s w|own worst %5.2f | %s' % (spec, path, 'own grad', worst, cells), flush=True)
    for what, (rows, over, worst) in above.items():
        print('first learn, %d cases, %s: %d of %d rows above %g x E_ref, largest %.2f' % (len(cases), what, over, rows, L.FACTOR, worst))


if __name__ == '__main__':
    mode, names = sys.argv[1], sys.argv[2:]
    if mode == 'qmix':       # qmix [batch ...] [path ...]: those of the cases of tests/test_gpu_qmix_learn_f64.py, default all
        from qmix_helpers import F64_CASES, F64_PATHS
        specs, paths = [x for x in names if x not in F64_PATHS], [x for x in names if x in F64_PATHS]
        qmix([c for c in F64_CASES if (not specs or c[0] in specs) and (not paths or c[1] in paths)])
    else:
        {'cpu': cpu, 'gpu': gpu}[mode](names or L.ALL_GOLDENS)
