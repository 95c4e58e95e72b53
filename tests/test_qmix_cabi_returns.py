"""The return code of every exported mixing / TD entry point of libqmix_ops.so (include/qmix_ops.h, qmix_packed.h, qmix_lambda.h,
qmix_double.h) for one valid argument list with one argument broken at a time, and for pairs of broken arguments that pin the ORDER of
the checks (n_units < 0 before the shape check, the shape check before the NULL checks, n_units == 0 accepted only after every check).

tests/golden/qmix_cabi_returns.json holds the codes that the library gave BEFORE its entry points were folded into one argument check
and one launch path (tools/record_mix_block_fixture.py).  Every call here returns before any launch: its recorded code is an error, or
its n_units is 0.  So the device pointers are dummy non-NULL numbers, `counts` and the two qmix_mixer structs are host memory, and the
test needs no GPU.  An argument that may be NULL (d_bad_actions, d_targets, d_picks, d_p_target_row, d_sel_units, the stream) is only
broken where n_units == 0 keeps the call from launching, that is in the packed forms."""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'qmix_cabi_returns.json')
B, T, TL, N, A, H, M, U = 3, 5, 7, 4, 5, 32, 32, 9
COUNTS = [3, 2, 2, 1, 1]                                   # sums to U
BIG = 513                                                  # QMIX_LAMBDA_MAX_T + 1
_PTRS = {}


def ptr(name):
    """A dummy device pointer: non-NULL, 256-byte aligned, one per name."""
    return _PTRS.setdefault(name, 0x7f0000000000 + 0x1000 * (len(_PTRS) + 1))


def counts(values):
    return (C.c_int32 * max(1, len(values)))(*values)


def mixer(name, misaligned=False):
    from marl_dmfb_amd import _lib
    return _lib.QmixMixer(*[ptr(name + f) + (4 if misaligned and f == 'w1' else 0) for f in ('w1', 'b1', 'w2', 'b2', 'wb', 'bb')])


def _d(*names):
    return [(k, ptr(k)) for k in names]


def _padded_forward():
    return (_d('qe', 'qt', 'u', 'r', 'avail', 'term', 'padded') + [('B', B), ('T', T), ('Tl', TL), ('n', N), ('A', A), ('pe', ptr('pe')),
            ('pe_rows', T + 1), ('pe_off', 0), ('pt', ptr('pt')), ('pt_rows', T + 1), ('pt_off', 1), ('H', H), ('M', M), ('ev', 'ev'),
            ('tg', 'tg'), ('gamma', 0.99)] + _d('mtd', 'mask', 'cnt'))


def _packed_forward():
    return (_d('qe', 'qt', 'units') + [('U', U)] + _d('u', 'r', 'avail', 'term', 'padded') + [('n', N), ('A', A)] + _d('pe', 'pt', 'trow') +
            [('H', H), ('M', M), ('ev', 'ev'), ('tg', 'tg'), ('gamma', 0.99)] + _d('mtd', 'mask', 'cnt'))


_LAMBDA = [('lam', 0.8)] + _d('tot_e', 'tot_t', 'tgt')
_STEPS = [('n_steps', len(COUNTS)), ('counts', COUNTS)]
# entry point -> its valid argument list, in order
ARGS = {
    'qmix_mix_td_forward': _padded_forward() + [('stream', None)],
    'qmix_mix_td_lambda_forward': _padded_forward() + _LAMBDA + [('stream', None)],
    'qmix_mix_td_double_forward': _padded_forward() + _LAMBDA + _d('sel', 'picks') + [('stream', None)],
    'qmix_mix_td_forward_packed': _packed_forward() + [('stream', None)],
    'qmix_mix_td_lambda_forward_packed': _packed_forward() + _LAMBDA + _STEPS + [('stream', None)],
    'qmix_mix_td_double_forward_packed': (_packed_forward() + _LAMBDA + _STEPS + [('sel', ptr('sel')), ('n_sel', U + 3)] + _d('sel_units', 'picks') +
                                          [('stream', None)]),
    'qmix_mix_td_backward': (_d('mtd', 'mask', 'qe', 'u') + [('B', B), ('T', T), ('Tl', TL), ('n', N), ('A', A), ('pe', ptr('pe')),
                             ('pe_rows', T + 1), ('pe_off', 0), ('H', H), ('M', M), ('ev', 'ev')] + _d('gnum', 'gq', 'gp', 'z', 'x') +
                             [('stream', None)]),
    'qmix_mix_td_backward_packed': (_d('mtd', 'mask', 'qe', 'units') + [('U', U), ('u', ptr('u')), ('n', N), ('A', A), ('rows_pad', 64),
                                    ('pe', ptr('pe')), ('H', H), ('M', M), ('ev', 'ev')] + _d('gnum', 'gq', 'gp', 'z', 'x') + [('stream', None)]),
}
TABLE = {'qmix_mix_td_forward': 'qmix_ops', 'qmix_mix_td_backward': 'qmix_ops', 'qmix_mix_td_forward_packed': 'qmix_packed',
         'qmix_mix_td_backward_packed': 'qmix_packed', 'qmix_mix_td_lambda_forward': 'qmix_lambda',
         'qmix_mix_td_lambda_forward_packed': 'qmix_lambda', 'qmix_mix_td_double_forward': 'qmix_double',
         'qmix_mix_td_double_forward_packed': 'qmix_double'}
MAY_BE_NULL = ('cnt', 'tgt', 'picks', 'trow', 'sel_units', 'stream')
NO_UNITS = dict(U=0, n_steps=0, counts=[], rows_pad=0)


def rows(entry):
    """[(label, {argument: broken value})] of one entry point."""
    names = [k for k, _ in ARGS[entry]]
    has = lambda *ks: all(k in names for k in ks)   # noqa: E731
    out = []

    def add(label, **over):
        assert all(k in names for k in over), (entry, label)
        out.append((label, over))
    for k, v in ARGS[entry]:                                    # each pointer NULL
        if (isinstance(v, int) and v > 0xffff and k not in MAY_BE_NULL) or k in ('ev', 'tg'):
            add(k + '=NULL', **{k: None})
    zero = {k: v for k, v in NO_UNITS.items() if k in names}
    if has('U'):
        add('n_units=-1', U=-1)
        add('n_units=-1,hyper_hidden=25', U=-1, H=25)
        add('n_units=0', **zero)
        add('n_units=0,hyper_hidden=25', **dict(zero, H=25))
        add('n_units=0,qe=NULL', **dict(zero, qe=None))
        for k in MAY_BE_NULL:
            if has(k) and k != 'sel_units':
                add('n_units=0,%s=NULL' % k, **dict(zero, **{k: None}))
    else:
        add('B=0', B=0)
        add('B=0,hyper_hidden=25', B=0, H=25)
        add('T=513', T=BIG)                                    # beyond t_limit
        add('p_eval_rows<T+p_eval_off', pe_rows=T - 1)
        add('p_eval_off=2', pe_off=2)
        add('n_agents=17,p_eval_rows<T+p_eval_off', n=17, pe_rows=T - 1)
    add('n_agents=17', n=17)
    add('n_actions=17', A=17)
    add('hyper_hidden=25', H=25)
    add('qmix_hidden=31', M=31)
    add('hyper_hidden=25,qe=NULL', H=25, qe=None)
    add('w1 misaligned', ev='misaligned')
    if has('tg'):
        add('target w1 misaligned', tg='misaligned')
    if has('rows_pad'):
        add('rows_pad<n_units*n_agents', rows_pad=U * N - 1)
    if has('lam'):
        for lam in (-0.1, 1.5, float('nan')):
            add('lam=%g' % lam, lam=lam)
        add('lam=nan,hyper_hidden=25', lam=float('nan'), H=25)
        add('lam=nan,qe=NULL', lam=float('nan'), qe=None)
        big = dict(T=BIG, Tl=BIG + 2, pe_rows=BIG + 1, pt_rows=BIG + 1) if has('T') else dict(n_steps=BIG, counts=[1] * BIG, U=BIG)
        add('T=513 in range of its buffers', **big)
        if has('sel'):                                          # at lam == 0 the steps are not limited: another check must answer
            add('lam=0,T=513 in range of its buffers,sel=NULL', **dict(big, lam=0.0, sel=None))
    if has('counts'):
        add('counts growing', counts=[3, 1, 2, 2, 1])
        add('counts sum != n_units', counts=[3, 2, 2, 1, 0])
        add('counts beyond n_units', counts=[4, 3, 2, 1, 1])
        add('counts negative', counts=[3, 3, 3, 1, -1])
        add('counts=NULL', counts=None)
        add('n_steps=-1', n_steps=-1)
        add('n_units=0,counts sum 9', U=0)
        if has('sel'):                                          # not read at lam == 0: accepted, and no unit to launch for
            add('lam=0,n_units=0,counts growing', lam=0.0, U=0, counts=[3, 1, 2, 2, 1])
            add('lam=0,n_units=0,counts=NULL', lam=0.0, U=0, counts=None)
            add('lam=0,n_units=0,tot_e=NULL', lam=0.0, U=0, tot_e=None)
    if has('n_sel'):
        add('n_sel_units=0', n_sel=0)
        add('sel_units=NULL,n_sel_units<n_units', sel_units=None, n_sel=U - 1)
        add('n_units=0,sel_units=NULL', **dict(zero, sel_units=None))
        add('n_units=0,n_sel_units=0', **dict(zero, n_sel=0))
    assert len({label for label, _ in out}) == len(out), entry
    return out


def call(entry, over):
    """-> (return code, whether the call had units to launch for)"""
    from marl_dmfb_amd import _lib
    a = dict(ARGS[entry])
    a.update(over)
    keep = []                                                   # host memory that must outlive the call
    for k in ('ev', 'tg'):
        if a.get(k) is not None:
            keep.append(mixer(k, a[k] == 'misaligned'))
            a[k] = C.byref(keep[-1])
    if a.get('counts') is not None:
        a['counts'] = counts(a['counts'])
    fn = getattr(getattr(_lib, TABLE[entry])(), entry)
    return fn(*[a[k] for k, _ in ARGS[entry]]), a.get('U', 1) != 0


def record():
    """entry point -> {label: code} from the library in use.  No row may get as far as a launch."""
    rec = {}
    for entry in ARGS:
        rec[entry] = {}
        for label, over in rows(entry):
            rc, units = call(entry, over)
            assert rc != 0 or not units, (entry, label, 'the arguments are accepted: the call went on to a launch')
            rec[entry][label] = rc
    return rec


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_record_holds_every_row():
    g = _golden()
    assert sorted(g) == sorted(ARGS)
    for entry in ARGS:
        assert list(g[entry]) == [label for label, _ in rows(entry)], entry
        assert set(g[entry].values()) <= {0, -1, -6}, entry
        assert {-1, -6} <= set(g[entry].values()), entry
        assert g[entry]['hyper_hidden=25'] == -6 and g[entry]['hyper_hidden=25,qe=NULL'] == -6 and g[entry]['w1 misaligned'] == -1
        if 'n_units=-1,hyper_hidden=25' in g[entry]:
            assert g[entry]['n_units=-1,hyper_hidden=25'] == -1 and g[entry]['n_units=0'] == 0 and g[entry]['n_units=0,qe=NULL'] == -1
    assert g['qmix_mix_td_lambda_forward_packed']['n_units=0,counts sum 9'] == -1
    assert g['qmix_mix_td_double_forward_packed']['lam=0,n_units=0,counts growing'] == 0
    assert sum(len(v) for v in g.values()) > 250


@pytest.mark.parametrize('entry', sorted(ARGS))
def test_return_codes_of_the_build_before(entry):
    g = _golden()[entry]
    for label, over in rows(entry):
        want = g[label]
        assert want != 0 or over.get('U') == 0, (entry, label, 'a row that would launch')
        rc, _ = call(entry, over)
        print('%s [%s]: %d (recorded %d)' % (entry, label, rc, want))
        assert rc == want, (entry, label, rc, want)
