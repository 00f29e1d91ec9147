"""options() of tests/gpu_helpers.py on the device: a scope that changes the bits leaves nothing behind, although its body raises."""
import pytest

from gpu_helpers import options, same

pytestmark = pytest.mark.gpu

FRAME = (33, 17)              # ragged 4x4 tiles on both edges
S_BEGIN, S_END = 1, 4         # samplings 1 .. 3: batch 1 cuts three launches where the automatic batch cuts one


def _render(r):
    r.clear()
    r.render(S_BEGIN, S_END)
    return r.read_accumulator(), r.stats()["shading_in_force"]


def test_a_scope_that_raises_leaves_the_defaults(ha, scenes):
    with ha.Renderer(0) as r:
        r.upload_scene(scenes("rtcamp6_v3_1")[0])
        r.set_resolution(*FRAME)
        a, shading = _render(r)
        assert a.any()
        with pytest.raises(ZeroDivisionError):
            with options(r, {"batch": 1, "precise_shading": 1, "counters": 1}, {"kchunk": 1, "trace_mode": 1}):
                inside, _ = _render(r)
                assert not same(inside, a), "the scope changed nothing"
                1 / 0
        after, shading_after = _render(r)
        assert same(after, a) and shading_after == shading
