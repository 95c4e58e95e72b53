"""CPU-side checks of the packed QMIX ABI (include/qmix_packed.h, built into libqmix_ops.so): the cross-compiled library exports
every declared prototype, the binding table 'qmix_packed' has the declared parameter counts, the host guards of the three entry
points return the documented code for one refused argument at a time, and a count of zero returns 0.

EVERY call below is one the host refuses or answers without a launch: the pointers are fake, aligned, non-null addresses that are
never dereferenced (only the qmix_mixer structs, which live in host memory, are read)."""
import ctypes as C
import os
import re

import pytest

from marl_dmfb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED = 0, -1, -6
FAKE = 0x10000            # 16-byte aligned, never dereferenced


def _prototypes():
    txt = open(os.path.join(ROOT, 'include', 'qmix_packed.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    txt = re.sub(r'^\s*#.*$', '', txt, flags=re.M)
    out = {}
    for name, params in re.findall(r'\b([a-z][a-z_0-9]*)\s*\(([^()]*)\)\s*;', txt):
        params = params.strip()
        out[name] = 0 if params in ('', 'void') else params.count(',') + 1
    return out


def test_library_exports_every_declared_symbol():
    declared = _prototypes()
    assert declared == {'qmix_mix_td_forward_packed': 23, 'qmix_mix_td_backward_packed': 19, 'qmix_gather_states': 7}
    table = _lib.SIGNATURES['qmix_packed']
    assert sorted(table) == sorted(declared)
    assert _lib._FILE['qmix_packed'] == 'qmix_ops'
    lib = _lib.qmix_packed()
    assert lib._name == _lib.qmix_ops()._name             # one library file
    for name, n in declared.items():
        assert len(table[name]) == n, name
        assert len(getattr(lib, name).argtypes) == n, name


def test_the_prefix_resolves_to_the_error_getter():
    for fn in _lib.SIGNATURES['qmix_packed']:
        assert [p for p in _lib._LAST_ERROR if fn.startswith(p)] == ['qmix_'], fn
    with pytest.raises(RuntimeError, match=r'qmix_gather_states failed: -1 \(hip 0\)'):
        _lib.checked('qmix_packed').qmix_gather_states(FAKE, 10, 0, FAKE, 4, FAKE, None)


def _mixer(**kw):
    f = dict(w1=FAKE, b1=FAKE + 4, w2=FAKE + 32, b2=FAKE + 4, wb=FAKE + 8, bb=FAKE + 12)
    f.update(kw)
    return _lib.QmixMixer(**f)


GOOD = dict(q_e=FAKE, q_t=FAKE, units=FAKE, U=6, u=FAKE, r=FAKE, avail=FAKE, term=FAKE, padded=FAKE, n=4, A=5, p_e=FAKE, p_t=FAKE,
            trow=FAKE, H=24, M=32, ev='ok', tg='ok', mtd=FAKE, mask=FAKE, bad=FAKE, rows_pad=64, g_num=FAKE, gq=FAKE, gp=FAKE, z=FAKE,
            x=FAKE)
FWD_ONLY = {'q_t', 'r', 'avail', 'term', 'padded', 'p_t', 'trow', 'tg', 'bad'}
BWD_ONLY = {'rows_pad', 'g_num', 'gq', 'gp', 'z', 'x'}


def _call(which, **kw):
    """One call with exactly the arguments of `kw` replaced.  A call that neither is refused nor has a zero count would launch:
    never make one."""
    assert kw, 'a call that the host accepts with a count above zero must not be made here'
    a = dict(GOOD)
    a.update(kw)
    keep = []                                     # the structs must outlive the call
    for k in ('ev', 'tg'):
        if a[k] == 'ok':
            a[k] = _mixer()
        if a[k] is not None:
            keep.append(a[k])
            a[k] = C.byref(a[k])
    lib = _lib.qmix_packed()
    if which == 'forward':
        return lib.qmix_mix_td_forward_packed(a['q_e'], a['q_t'], a['units'], a['U'], a['u'], a['r'], a['avail'], a['term'], a['padded'],
                                              a['n'], a['A'], a['p_e'], a['p_t'], a['trow'], a['H'], a['M'], a['ev'], a['tg'], 0.99,
                                              a['mtd'], a['mask'], a['bad'], None)
    return lib.qmix_mix_td_backward_packed(a['mtd'], a['mask'], a['q_e'], a['units'], a['U'], a['u'], a['n'], a['A'], a['rows_pad'],
                                           a['p_e'], a['H'], a['M'], a['ev'], a['g_num'], a['gq'], a['gp'], a['z'], a['x'], None)


NULL_MIXER = _lib.QmixMixer()      # every field NULL
REFUSED = [
    (dict(U=-1), BAD_ARG), (dict(U=-(2 ** 31)), BAD_ARG), (dict(n=0), BAD_ARG), (dict(n=-1), BAD_ARG), (dict(A=0), BAD_ARG),
    (dict(A=-1), BAD_ARG), (dict(ev=None), BAD_ARG),
    # the build limits; this code comes back even if the mixer's fields are NULL
    (dict(M=16), UNSUPPORTED), (dict(M=64), UNSUPPORTED), (dict(H=16), UNSUPPORTED), (dict(H=28), UNSUPPORTED), (dict(H=64), UNSUPPORTED),
    (dict(n=17), UNSUPPORTED), (dict(A=17), UNSUPPORTED),
    (dict(M=16, ev=NULL_MIXER, tg=NULL_MIXER), UNSUPPORTED), (dict(n=17, ev=NULL_MIXER, tg=NULL_MIXER), UNSUPPORTED),
    # the mixer's fields
    (dict(ev=NULL_MIXER), BAD_ARG),
] + [(dict(ev=_mixer(**{f: None})), BAD_ARG) for f in ('w1', 'b1', 'w2', 'b2', 'wb', 'bb')] + [
    (dict(ev=_mixer(w1=FAKE + 4)), BAD_ARG), (dict(ev=_mixer(w2=FAKE + 8)), BAD_ARG),
    # every required device pointer
] + [(dict([(p, None)]), BAD_ARG) for p in ('q_e', 'q_t', 'units', 'u', 'r', 'avail', 'term', 'padded', 'p_e', 'p_t', 'mtd', 'mask',
                                            'g_num', 'gq', 'gp', 'z', 'x')] + [
    # fewer rows of grad_q than the units have (6 units x 4 droplets)
    (dict(rows_pad=23), BAD_ARG), (dict(rows_pad=0), BAD_ARG), (dict(rows_pad=-64), BAD_ARG),
    # the target mixer, the eval mixer being fine
    (dict(tg=None), BAD_ARG), (dict(tg=NULL_MIXER), BAD_ARG), (dict(tg=_mixer(wb=None)), BAD_ARG), (dict(tg=_mixer(w2=FAKE + 4)), BAD_ARG),
]


def _id(kw):
    return ','.join('%s=%s' % (k, v if isinstance(v, int) or v is None else ''.join(
        f for f, _ in v._fields_ if not getattr(v, f)) or 'misaligned') for k, v in kw.items())


@pytest.mark.parametrize('kw,code', REFUSED, ids=[_id(kw) for kw, _ in REFUSED])
def test_one_refused_argument_at_a_time(kw, code):
    names = set(kw)
    ran = 0
    if not names <= BWD_ONLY:
        assert _call('forward', **{k: v for k, v in kw.items() if k not in BWD_ONLY}) == code
        ran += 1
    if not names <= FWD_ONLY:
        assert _call('backward', **{k: v for k, v in kw.items() if k not in FWD_ONLY}) == code
        ran += 1
    assert ran


def test_the_optional_pointers_alone_are_not_refused():
    """d_bad_actions and d_p_target_row may be NULL (include/qmix_packed.h): a call refused for another reason returns that
    reason's code with and without them, and with a zero count the call is accepted."""
    for opt in ('bad', 'trow'):
        assert _call('forward', U=-1, **{opt: None}) == BAD_ARG and _call('forward', H=28, **{opt: None}) == UNSUPPORTED
        assert _call('forward', U=0, **{opt: None}) == OK


def test_zero_counts_return_ok_without_a_launch():
    assert _call('forward', U=0) == OK
    assert _call('backward', U=0) == OK and _call('backward', U=0, rows_pad=0) == OK
    assert _lib.qmix_packed().qmix_gather_states(FAKE, 10, 300, FAKE, 0, FAKE, None) == OK
    assert _lib.qmix_packed().qmix_last_hip_error() == 0


GATHER_GOOD = dict(states=FAKE + 1, n_state_rows=10, S=300, rows=FAKE, n_rows=4, out=FAKE)


@pytest.mark.parametrize('kw', [dict(states=None), dict(rows=None), dict(out=None), dict(n_rows=-1), dict(S=0), dict(S=-5),
                                dict(n_state_rows=0), dict(n_state_rows=-1)], ids=lambda kw: _id(kw))
def test_gather_refuses_one_argument_at_a_time(kw):
    a = dict(GATHER_GOOD)
    a.update(kw)
    assert _lib.qmix_packed().qmix_gather_states(a['states'], a['n_state_rows'], a['S'], a['rows'], a['n_rows'], a['out'], None) == BAD_ARG
