"""tests/gpu_helpers.py without a GPU: options() against a fake that records its set_option / set_debug_option calls, and the bit comparison."""
import numpy as np
import pytest

from gpu_helpers import bits, options, same
from schedule_knobs import ALL_DEFAULTS as DEF


class Fake:
    """records (setter, key, value); raises RuntimeError on its `fail_at`-th call (1-based)"""

    def __init__(self, fail_at=0):
        self.calls, self.fail_at, self.n = [], fail_at, 0

    def _set(self, setter, key, value):
        self.n += 1
        if self.n == self.fail_at:
            raise RuntimeError("refused")
        self.calls.append((setter, key, value))

    def set_option(self, key, value):
        self._set("set_option", key, value)

    def set_debug_option(self, key, value):
        self._set("set_debug_option", key, value)


OPTS, DBG = {"russian_roulette": 3, "batch": 1, "counters": 1}, {"kchunk": 1, "trace_mode": 1}
ENTRY = [("set_option", "russian_roulette", 3), ("set_option", "batch", 1), ("set_option", "counters", 1),
         ("set_debug_option", "kchunk", 1), ("set_debug_option", "trace_mode", 1)]
EXIT = [("set_debug_option", "trace_mode", DEF["trace_mode"]), ("set_debug_option", "kchunk", DEF["kchunk"]), ("set_option", "counters", DEF["counters"]),
        ("set_option", "batch", DEF["batch"]), ("set_option", "russian_roulette", DEF["russian_roulette"])]


def test_options_apply_in_order_and_restore_in_reverse():
    f = Fake()
    with options(f, OPTS, DBG):
        assert f.calls == ENTRY
    assert f.calls == ENTRY + EXIT
    f = Fake()
    with options(f):
        pass
    assert f.calls == []


def test_options_restore_after_an_exception_in_the_body():
    f = Fake()
    with pytest.raises(ZeroDivisionError):
        with options(f, OPTS, DBG):
            1 / 0
    assert f.calls == ENTRY + EXIT


def test_options_restore_what_was_applied_when_a_setter_raises_on_entry():
    f = Fake(fail_at=4)          # kchunk is refused: the three before it go back, trace_mode is never set
    with pytest.raises(RuntimeError):
        with options(f, OPTS, DBG):
            raise AssertionError("the body must not run")
    assert f.calls == ENTRY[:3] + EXIT[2:]


def test_options_refuse_an_unknown_key_before_anything_is_set():
    for opts, dbg in (({"batch": 1, "no_such_option": 1}, None), ({"batch": 1}, {"no_such_option": 1}), ({"batch": 1, "kchunk": 1}, None)):
        f = Fake()
        with pytest.raises(KeyError):
            with options(f, opts, dbg):
                raise AssertionError("the body must not run")
        assert f.calls == []
    f = Fake()
    with pytest.raises(KeyError):
        with options(f, {"batch": 1}) as o:
            o.set("no_such_option", 1)
    assert f.calls == [("set_option", "batch", 1), ("set_option", "batch", DEF["batch"])]


def test_set_several_times_restores_once():
    f = Fake()
    with options(f, {"counters": 1}) as o:
        for v in (8, 1, 8):
            o.set("batch", v)
        o.set("seed_mode", 1)
        o.set("counters", 0)
    assert f.calls == [("set_option", "counters", 1), ("set_option", "batch", 8), ("set_option", "batch", 1), ("set_option", "batch", 8),
                       ("set_debug_option", "seed_mode", 1), ("set_option", "counters", 0),
                       ("set_debug_option", "seed_mode", DEF["seed_mode"]), ("set_option", "batch", DEF["batch"]), ("set_option", "counters", DEF["counters"])]


def test_same_and_bits():
    a = np.arange(6, dtype=np.float32)
    assert same(a, a.copy()) and not same(a, a.reshape(2, 3)) and not same(a.reshape(3, 2), a.reshape(2, 3))
    assert not same(np.array([0.0], np.float32), np.array([-0.0], np.float32)) and not same(np.array([0.0]), np.array([-0.0]))
    nan = np.array([np.nan], np.float32)
    assert same(nan, nan.copy())
    assert bits(np.array([1.0, -0.0], np.float32)).tolist() == [0x3F800000, 0x80000000] and bits(np.float32([1.0])).dtype == np.uint32
    assert bits(np.array([1.0, -0.0], np.float64)).tolist() == [0x3FF0000000000000, 0x8000000000000000] and bits(np.float64([1.0])).dtype == np.uint64
    assert bits(a.reshape(2, 3)[:, ::2]).shape == (2, 2)          # a strided view is made contiguous first
