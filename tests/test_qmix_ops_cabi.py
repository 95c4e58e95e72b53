"""CPU-side checks of the mixing + TD ABI (include/qmix_ops.h): the cross-compiled library exports every declared prototype, the
binding table has the declared parameter counts, and the host guards of both entry points return the documented code for one
refused argument at a time.

EVERY call below is one the host refuses, so nothing is ever launched: the other pointers are fake, aligned, non-null addresses
that are never dereferenced (only the qmix_mixer structs, which live in host memory, are read)."""
import ctypes as C
import os
import re

import pytest

from marl_dmfb_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -6
FAKE = 0x10000            # 16-byte aligned, never dereferenced


def _prototypes():
    txt = open(os.path.join(ROOT, 'include', 'qmix_ops.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    txt = re.sub(r'^\s*#.*$', '', txt, flags=re.M)
    out = {}
    for name, params in re.findall(r'\b([a-z][a-z_0-9]*)\s*\(([^()]*)\)\s*;', txt):
        params = params.strip()
        out[name] = 0 if params in ('', 'void') else params.count(',') + 1
    return out


def test_qmix_ops_library_exports_every_declared_symbol():
    declared = _prototypes()
    assert declared == {'qmix_mix_td_forward': 27, 'qmix_mix_td_backward': 21, 'qmix_last_hip_error': 0}
    table = _lib.SIGNATURES['qmix_ops']
    assert sorted(table) == sorted(declared)
    lib = _lib.qmix_ops()
    for name, n in declared.items():
        sig = table[name]
        assert len(sig[0] if isinstance(sig, tuple) else sig) == n, name
        assert len(getattr(lib, name).argtypes) == n, name


def test_error_codes_are_the_headers():
    txt = open(os.path.join(ROOT, 'include', 'qmix_ops.h')).read()
    codes = dict(re.findall(r'#define (QMIX_[A-Z_]+) \(?(-?\d+)\)?', txt))
    assert codes == {'QMIX_OK': '0', 'QMIX_ERR_BAD_ARG': '-1', 'QMIX_ERR_UNSUPPORTED': '-6', 'QMIX_ERR_HIP': '-100'}


def test_the_prefix_resolves_to_the_error_getter():
    assert _lib._LAST_ERROR['qmix_'] == 'qmix_last_hip_error'
    owners = [p for p in _lib._LAST_ERROR if 'qmix_mix_td_forward'.startswith(p)]
    assert owners == ['qmix_']
    assert _lib.qmix_ops().qmix_last_hip_error() == 0
    # the checked library turns a refused call into an exception that names the function, the code and the last HIP error
    ev = _mixer()
    with pytest.raises(RuntimeError, match=r'qmix_mix_td_backward failed: -1 \(hip 0\)'):
        _lib.checked('qmix_ops').qmix_mix_td_backward(FAKE, FAKE, FAKE, FAKE, 0, 3, 6, 4, 5, FAKE, 4, 0, 24, 32, C.byref(ev), FAKE, FAKE, FAKE,
                                                      FAKE, FAKE, None)


def _mixer(**kw):
    f = dict(w1=FAKE, b1=FAKE + 4, w2=FAKE + 32, b2=FAKE + 4, wb=FAKE + 8, bb=FAKE + 12)
    f.update(kw)
    return _lib.QmixMixer(**f)


GOOD = dict(q_e=FAKE, q_t=FAKE, u=FAKE, r=FAKE, avail=FAKE, term=FAKE, padded=FAKE, B=4, T=3, t_limit=6, n=4, A=5, p_e=FAKE, pe_rows=4,
            pe_off=0, p_t=FAKE, pt_rows=4, pt_off=1, H=24, M=32, ev='ok', tg='ok', mtd=FAKE, mask=FAKE, bad=FAKE, g_num=FAKE, gq=FAKE,
            gp=FAKE, z=FAKE, x=FAKE)
FWD_ONLY = {'q_t', 'r', 'avail', 'term', 'padded', 'p_t', 'pt_rows', 'pt_off', 'tg', 'bad'}
BWD_ONLY = {'g_num', 'gq', 'gp', 'z', 'x'}


def _call(which, **kw):
    """One call with exactly the arguments of `kw` replaced.  A call without a refused argument would launch: never make one."""
    assert kw, 'a call that the host accepts must not be made here'
    a = dict(GOOD)
    a.update(kw)
    keep = []                                     # the structs must outlive the call
    for k in ('ev', 'tg'):
        if a[k] == 'ok':
            a[k] = _mixer()
        if a[k] is not None:
            keep.append(a[k])
            a[k] = C.byref(a[k])
    lib = _lib.qmix_ops()
    if which == 'forward':
        return lib.qmix_mix_td_forward(a['q_e'], a['q_t'], a['u'], a['r'], a['avail'], a['term'], a['padded'], a['B'], a['T'], a['t_limit'],
                                       a['n'], a['A'], a['p_e'], a['pe_rows'], a['pe_off'], a['p_t'], a['pt_rows'], a['pt_off'], a['H'],
                                       a['M'], a['ev'], a['tg'], 0.99, a['mtd'], a['mask'], a['bad'], None)
    return lib.qmix_mix_td_backward(a['mtd'], a['mask'], a['q_e'], a['u'], a['B'], a['T'], a['t_limit'], a['n'], a['A'], a['p_e'],
                                    a['pe_rows'], a['pe_off'], a['H'], a['M'], a['ev'], a['g_num'], a['gq'], a['gp'], a['z'], a['x'], None)


NULL_MIXER = _lib.QmixMixer()      # every field NULL
REFUSED = [
    # the shape and the mixer pointer itself
    (dict(B=0), BAD_ARG), (dict(B=-1), BAD_ARG), (dict(T=0), BAD_ARG), (dict(T=-3), BAD_ARG), (dict(t_limit=2), BAD_ARG),
    (dict(n=0), BAD_ARG), (dict(n=-1), BAD_ARG), (dict(A=0), BAD_ARG), (dict(A=-1), BAD_ARG), (dict(ev=None), BAD_ARG),
    # the build limits; this code comes back even if the mixer's fields are NULL
    (dict(M=16), UNSUPPORTED), (dict(M=64), UNSUPPORTED), (dict(H=16), UNSUPPORTED), (dict(H=28), UNSUPPORTED), (dict(H=64), UNSUPPORTED),
    (dict(n=17), UNSUPPORTED), (dict(A=17), UNSUPPORTED),
    (dict(M=16, ev=NULL_MIXER, tg=NULL_MIXER), UNSUPPORTED), (dict(H=28, ev=NULL_MIXER, tg=NULL_MIXER), UNSUPPORTED),
    (dict(n=17, ev=NULL_MIXER, tg=NULL_MIXER), UNSUPPORTED), (dict(A=17, ev=NULL_MIXER, tg=NULL_MIXER), UNSUPPORTED),
    # the mixer's fields
    (dict(ev=NULL_MIXER), BAD_ARG),
] + [(dict(ev=_mixer(**{f: None})), BAD_ARG) for f in ('w1', 'b1', 'w2', 'b2', 'wb', 'bb')] + [
    (dict(ev=_mixer(w1=FAKE + 4)), BAD_ARG), (dict(ev=_mixer(w1=FAKE + 8)), BAD_ARG), (dict(ev=_mixer(w2=FAKE + 4)), BAD_ARG),
    (dict(ev=_mixer(w2=FAKE + 8)), BAD_ARG),
    # the device pointers and the P layout
] + [(dict([(p, None)]), BAD_ARG) for p in ('q_e', 'q_t', 'u', 'r', 'avail', 'term', 'padded', 'p_e', 'p_t', 'mtd', 'mask', 'g_num', 'gq',
                                            'gp', 'z', 'x')] + [
    (dict(pe_off=-1), BAD_ARG), (dict(pe_rows=2), BAD_ARG), (dict(pe_rows=3, pe_off=1), BAD_ARG), (dict(pt_off=-1), BAD_ARG),
    (dict(pt_rows=3), BAD_ARG), (dict(pt_rows=2, pt_off=0), BAD_ARG),
    # the target mixer, the eval mixer being fine: its own code
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
        assert _call('forward', **kw) == code
        ran += 1
    if not names <= FWD_ONLY:
        assert _call('backward', **{k: v for k, v in kw.items() if k not in FWD_ONLY}) == code
        ran += 1
    assert ran


def test_the_counter_may_be_null_but_that_alone_is_not_refused():
    """d_bad_actions is the one pointer that may be NULL (include/qmix_ops.h): a call that is refused for another reason returns
    that reason's code with and without it."""
    assert _call('forward', bad=None, B=0) == BAD_ARG and _call('forward', bad=None, H=28) == UNSUPPORTED
