"""Poisoned allocations: `poisoned(pattern)` replaces torch.empty and torch.empty_like, for the length of a `with` block, with
wrappers that allocate through the real function and then fill the result.  A value that comes out of a learn, a rollout or a
planner the same with clean memory, under pattern 'A' and under pattern 'B' was computed from written elements only; one that
differs was read from memory nobody wrote (tests/test_poison_alloc.py, test_gpu_poisoned_learn.py, test_gpu_poisoned_rollout.py).

Patterns: floating dtypes NaN ('A') / -777.25 ('B': finite, and no computation here produces it); integer dtypes 1 / 2; bool
True / False.  The integer values are small and non-negative on purpose: a poisoned word that a bug lets through as a chip id, row
index, action or slot is still a valid index into every buffer of the scenarios of those tests (at least 4 chips, 3 droplets and
5 actions), so a wrong VALUE is all these tests can cause, never an out-of-range address.

The fill is `fill_` alone (no host synchronisation), so the wrappers also work while a HIP graph is being captured.  What the
wrappers do not see -- new_empty, empty_strided, resize_, the legacy constructors, `from torch import empty` -- the package must
not use: the source guard of tests/test_poison_alloc.py holds it to that."""
import contextlib
import os
import sys

import torch

FLOAT_B = -777.25
PATTERNS = {'A': (float('nan'), 1, True), 'B': (FLOAT_B, 2, False)}
PACKAGE = 'marl_dmfb_amd'
_PKG_DIR = os.sep + PACKAGE + os.sep


def fill_value(pattern, dtype):
    """What `poisoned(pattern)` fills a tensor of `dtype` with."""
    f, i, b = PATTERNS[pattern]
    if dtype == torch.bool:
        return b
    if dtype.is_floating_point or dtype.is_complex:
        return f
    return i


class Log:
    """count: poisoned allocations (all callers); sites: {'<file inside the package>:<line>': poisoned allocations made there},
    the innermost frame inside marl_dmfb_amd/ of each allocation that has one."""

    def __init__(self):
        self.count = 0
        self.sites = {}

    def package_count(self):
        return sum(self.sites.values())

    def files(self):
        return {s.rsplit(':', 1)[0] for s in self.sites}

    def functions_seen(self, module_file, names):
        """The names of `names` (functions or classes of the package file `module_file`, e.g. 'network/base_net.py') inside whose
        source lines a recorded site falls."""
        import ast
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), PACKAGE, module_file)
        with open(path) as fh:
            tree = ast.parse(fh.read())
        lines = {int(s.rsplit(':', 1)[1]) for s in self.sites if s.rsplit(':', 1)[0] == module_file}
        seen = set()
        for node in ast.walk(tree):
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
                if any(node.lineno <= ln <= node.end_lineno for ln in lines):
                    seen.add(node.name)
        return seen


def _site():
    f = sys._getframe(2)
    while f is not None:
        name = f.f_code.co_filename
        k = name.rfind(_PKG_DIR)
        if k >= 0:
            return '%s:%d' % (name[k + len(_PKG_DIR):].replace(os.sep, '/'), f.f_lineno)
        f = f.f_back
    return None


@contextlib.contextmanager
def poisoned(pattern, only=None):
    """pattern: 'A' or 'B'.  only: a set of sites ('policy/vdn.py:53') -- then only allocations made there are filled (for narrowing
    a finding to one allocation); every allocation is counted and recorded either way.  Yields the `Log`."""
    if pattern not in PATTERNS:
        raise ValueError('pattern must be one of %s' % sorted(PATTERNS))
    log = Log()
    real = {'empty': torch.empty, 'empty_like': torch.empty_like}

    def wrap(fn):
        def alloc(*args, **kwargs):
            t = fn(*args, **kwargs)
            if isinstance(t, torch.Tensor) and t.numel() > 0:
                site = _site()
                if site is not None:
                    log.sites[site] = log.sites.get(site, 0) + 1
                if only is None or site in only:
                    t.fill_(fill_value(pattern, t.dtype))
                    log.count += 1
            return t
        alloc.__name__ = fn.__name__
        alloc.__wrapped__ = fn
        return alloc

    try:
        for name, fn in real.items():
            setattr(torch, name, wrap(fn))
        yield log
    finally:
        for name, fn in real.items():
            setattr(torch, name, fn)


@contextlib.contextmanager
def clean():
    """The same `with` shape for the unpoisoned run: yields None."""
    yield None


def run_mode(mode):
    """'clean' -> clean(), 'A' / 'B' -> poisoned(mode)."""
    return clean() if mode == 'clean' else poisoned(mode)


def bits_equal(a, b):
    """Bit equality of two tensors (or numpy arrays, or Python scalars) of one dtype and shape, NaN-safe."""
    import numpy as np
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        a, b = torch.as_tensor(a).detach().cpu(), torch.as_tensor(b).detach().cpu()
        if a.dtype != b.dtype or a.shape != b.shape:
            return False
        a, b = a.contiguous().numpy(), b.contiguous().numpy()
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return a.tobytes() == b.tobytes()


def first_difference(a, b):
    """'' when bit-equal, else a short description of where two same-shaped tensors first differ and of how many elements do."""
    import numpy as np
    if bits_equal(a, b):
        return ''
    a, b = np.asarray(torch.as_tensor(a).detach().cpu()), np.asarray(torch.as_tensor(b).detach().cpu())
    if a.dtype != b.dtype or a.shape != b.shape:
        return 'dtype/shape %s %s against %s %s' % (a.dtype, a.shape, b.dtype, b.shape)
    ne = ~((a == b) | ((a != a) & (b != b)))
    if a.ndim == 0:
        return '%r against %r' % (a.item(), b.item())
    at = tuple(int(i[0]) for i in np.nonzero(ne)) if ne.any() else ()
    if not at:
        return 'bit patterns differ (sign of zero / NaN payload)'
    return '%d of %d elements differ, first at %s: %r against %r' % (ne.sum(), ne.size, at, a[at].item(), b[at].item())
