"""What the GPU tests share: scoped options on a Renderer, the bit-pattern comparison, the error a call must raise, and the one order in which a
test's own Renderer is made.  The defaults and setters of every option come from tests/schedule_knobs.py, which tests/test_schedule_cpu.py holds
against hr_api.hip.

No GPU in this module."""
from contextlib import contextmanager

import numpy as np
import pytest

from schedule_knobs import ALL_DEFAULTS, SETTERS


class _Scope:
    def __init__(self, renderer):
        self.renderer = renderer
        self.touched = []              # keys in the order they were first set

    def set(self, key, value):
        """set the option now; it goes back to its default once, when the scope ends"""
        getattr(self.renderer, SETTERS[key])(key, value)   # (a refused value leaves what was in force: nothing to restore)
        if key not in self.touched:
            self.touched.append(key)

    def restore(self):
        for key in reversed(self.touched):
            getattr(self.renderer, SETTERS[key])(key, ALL_DEFAULTS[key])


@contextmanager
def options(renderer, opts=None, dbg=None):
    """Apply `opts` through set_option and `dbg` through set_debug_option, in the order given; on the way out — normal or not — set every key
    touched back to ALL_DEFAULTS[key], in reverse order (russian_roulette and precise_shading 1 refuse each other).  A key that is not in the
    table, or is given to the wrong setter, raises KeyError before anything is set.  The yielded scope's .set(key, value) changes a value
    inside the scope."""
    opts, dbg = opts or {}, dbg or {}
    for setter, given in (("set_option", opts), ("set_debug_option", dbg)):
        for key in given:
            if SETTERS[key] != setter:
                raise KeyError("%s goes through %s" % (key, SETTERS[key]))
    scope = _Scope(renderer)
    try:
        for key, value in list(opts.items()) + list(dbg.items()):
            scope.set(key, value)
        yield scope
    finally:
        scope.restore()


def bits(a):
    """the array's bit patterns (1-, 4- and 8-byte element types)"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def error_of(ha, fn, *a, **kw):
    """(code, text) of the HipError fn(*a, **kw) must raise"""
    with pytest.raises(ha.HipError) as e:
        fn(*a, **kw)
    return e.value.code, str(e.value)


def renderer(ha, sc, opts=None, dbg=None, frame=None, region=None, moments=False, counts=False, buckets=0):
    """A Renderer of the test's own (the caller closes it): options, debug options, the scene (None: none yet), then with a frame the target
    and the plane options (retarget)."""
    r = ha.Renderer(0)
    for k, v in (opts or {}).items():
        r.set_option(k, v)
    for k, v in (dbg or {}).items():
        r.set_debug_option(k, v)
    if sc is not None:
        r.upload_scene(sc)
    if frame is not None:
        retarget(r, frame, region, moments, counts, buckets)
    return r


def retarget(r, frame, region=None, moments=False, counts=False, buckets=0):
    r.set_resolution(*frame)
    if region is not None:
        r.set_region(*region)
    r.set_option("moments", 1 if moments else 0)
    r.set_option("sample_counts", 1 if counts else 0)
    r.set_option("robust_buckets", buckets)
