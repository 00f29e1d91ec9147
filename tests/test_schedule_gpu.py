"""Schedule knobs change no bit (tests/schedule_knobs.py) on the MI355X, at frames so small that the unit and queue arithmetic
of both pipelines meets its edges: the last partial chunk, bulk_units == 0, tail_tiles == 0, fewer work units than waves, fewer items than the
split pipeline's 64 sub-queues, a budget of one workgroup.  Every comparison is bit for bit; the reference of a (scene, frame, pipeline, shading)
is the same context with every knob at its default — the render the parity tests pin to the f64 oracle.

Samplings 1 .. 7 with option batch 3: launches of 3, 3 and 1 samplings (a partial last chunk under kchunk 2; num_k 1)."""
import numpy as np
import pytest

import light_material_scenes as lm
import schedule_knobs as K
from gpu_helpers import bits, error_of, options, renderer

pytestmark = pytest.mark.gpu

HR_ERR_INVALID, HR_ERR_UNSUPPORTED = -1, -6
S_BEGIN, S_END, BATCH, LAUNCHES = 1, 8, 3, 3
SAMPLINGS = S_END - S_BEGIN
RAGGED = (130, 71)        # 33 x 18 = 594 tiles, both sides ragged: several work units per wave
TINY = (9, 5)             # 3 x 2 = 6 tiles: fewer units than one workgroup's waves, fewer items than sub-queues, fewer tiles than tail_div
STRIPS = ((64, 1), (1, 64))   # 16 tiles, every one hanging over an edge
MESH_SCENE = "rtcamp6_v3_1"   # the full table runs here (a mesh BVH: leaf and box phases both busy)
MANY_LIGHTS = "many-ggx"      # nine emitters: a step of the split pipeline holds several shadow rays per path
MODES = [K.MEGA, K.SPLIT]
# (scene, [(frame, full table?)])
PLAN = [(MESH_SCENE, [(RAGGED, True), (TINY, True), (STRIPS[0], False), (STRIPS[1], False)]),
        ("cornell_mini", [(RAGGED, False), (TINY, False)]),
        (MANY_LIGHTS, [(RAGGED, False), (TINY, False)])]


def _scene(ha, scenes, name):
    if name == MANY_LIGHTS:
        assert len(lm.LIGHTS[lm.light_case(name)]) > 1
        return lm.CASES[name][1](ha)
    return scenes(name)[0]


def _make(ha, mode, precise, counters=0):
    return renderer(ha, None, {"batch": BATCH, "precise_shading": precise, "counters": counters}, {"trace_mode": mode})


def _render(r):
    r.clear()
    r.render(S_BEGIN, S_END)
    return r.read_accumulator()


def _reference(r, what):
    ref = _render(r)
    assert np.isfinite(ref).all() and ref.any(), what
    assert np.array_equal(bits(ref), bits(_render(r))), ("the default render does not repeat", what)
    return ref


def _walk(ha, scenes, r, plan=PLAN):
    """(what, frame, settings) over the plan, the scene uploaded and the frame set"""
    for name, frames in plan:
        r.upload_scene(_scene(ha, scenes, name))
        for (w, h), full in frames:
            r.set_resolution(w, h)
            yield (name, w, h), (w, h), full


@pytest.mark.parametrize("precise", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_single_knob_sweep(ha, scenes, mode, precise):
    """Every value of every row that acts on the pipeline in force, and the two combined settings: the accumulator of the defaults."""
    with _make(ha, mode, precise) as r:
        for what, _, full in _walk(ha, scenes, r):
            ref = _reference(r, what)
            assert r.stats()["shading_in_force"] == {K.MEGA: (0, 1), K.SPLIT: (3, 2)}[mode][precise], what
            for label, setting in K.settings(mode, full):
                with options(r, *K.split(setting)):
                    got = _render(r)
                differ = int((bits(got) != bits(ref)).any(axis=-1).sum())
                assert differ == 0, (what, mode, precise, label, "%d pixels differ" % differ)


@pytest.mark.parametrize("precise", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_accounting_sweep(ha, scenes, mode, precise):
    """The same settings under option counters: every path of the frame is rendered exactly once (a path rendered twice writes the same record
    twice and stays invisible in the accumulator), the rays traced and the shadow rays culled are the default setting's, three launches."""
    with _make(ha, mode, precise, counters=1) as r:
        for what, (w, h), full in _walk(ha, scenes, r):
            ref = _reference(r, what)
            st0 = r.stats()
            assert st0["paths"] == w * h * 4 * SAMPLINGS and st0["trace_launches"] == LAUNCHES and st0["rays"] >= st0["paths"], (what, st0["paths"], st0["rays"])
            for label, setting in K.settings(mode, full):
                with options(r, *K.split(setting)):
                    got = _render(r)
                    st = r.stats()
                tag = (what, mode, precise, label)
                assert st["paths"] == w * h * 4 * SAMPLINGS, tag + (st["paths"], w * h * 4 * SAMPLINGS)
                assert st["rays"] == st0["rays"] and st["shadow_culled"] == st0["shadow_culled"], tag + (st["rays"], st0["rays"], st["shadow_culled"], st0["shadow_culled"])
                assert st["trace_launches"] == LAUNCHES, tag
                assert np.array_equal(bits(got), bits(ref)), tag


def _mask():
    """seven of the 594 tiles of 130 x 71, the first and the last among them (the last one's lanes overhang the frame on both sides)"""
    ty, tx = (RAGGED[1] + 3) // 4, (RAGGED[0] + 3) // 4
    m = np.zeros((ty, tx), np.uint8)
    for y, x in [(0, 0), (0, tx - 1), (5, 7), (9, 20), (12, 3), (ty - 1, 0), (ty - 1, tx - 1)]:
        m[y, x] = 1
    return m


@pytest.mark.parametrize("precise", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_tile_mask_sweep(ha, scenes, mode, precise):
    """The LIST forms of the trace kernel and of wf_start_kernel (dense tile index against region tile): under a mask of seven tiles the unit and
    budget knobs give the masked default render, which is the unmasked render on the active tiles and nothing anywhere else."""
    w, h = RAGGED
    mask = _mask()
    pix = np.kron(mask != 0, np.ones((4, 4), bool))[:h, :w]
    with _make(ha, mode, precise) as r:
        r.upload_scene(scenes(MESH_SCENE)[0])
        r.set_resolution(w, h)
        r.set_option("sample_counts", 1)
        full = _reference(r, "unmasked")
        r.set_tile_mask(mask)
        assert r.tile_mask()[1] == int(mask.sum())
        ref = _render(r)
        assert np.array_equal(bits(ref), bits(np.where(pix[..., None], full, np.float32(0)))), "the masked default render"
        for label, setting in K.settings(mode, True, keys=K.UNIT_KNOBS):
            with options(r, *K.split(setting)):
                got = _render(r)
                counts = r.read_sample_counts()
            assert not bits(got)[~pix].any(), (mode, precise, label, "a pixel outside the active tiles was touched")
            assert np.array_equal(bits(got), bits(ref)), (mode, precise, label)
            assert np.array_equal(counts, np.where(pix, SAMPLINGS, 0).astype(np.uint32)), (mode, precise, label)


@pytest.mark.parametrize("precise", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_path_log_sweep(ha, scenes, mode, precise):
    """hr_debug_path_log plans its own launch (no tail, no budget): the knobs that still reach it leave the log of sampling 1 — radiance, ray
    counts, events and hashes of every path — word for word the default's."""
    with _make(ha, mode, precise) as r:
        r.upload_scene(scenes(MESH_SCENE)[0])
        for w, h in (TINY, RAGGED):
            r.set_resolution(w, h)
            ref = r.debug_path_log(1)
            assert np.isfinite(ref[0]).all() and ref[0].any() and (ref[1] > 0).all(), (w, h)
            for label, setting in K.settings(mode, True, keys=K.PATH_LOG_KNOBS, combined=False):
                with options(r, *K.split(setting)):
                    got = r.debug_path_log(1)
                for a, b in zip(got, ref):
                    assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), (w, h, mode, precise, label)


@pytest.mark.parametrize("mode", MODES)
def test_order_and_stickiness(ha, scenes, mode):
    """One context through both combined extremes and back to the defaults: nothing of a setting stays behind — the result is the reference
    again, and the result of a fresh context."""
    sc = scenes(MESH_SCENE)[0]
    r, fresh = _make(ha, mode, 0), None
    try:
        r.upload_scene(sc)
        for frame in (RAGGED, TINY):
            r.set_resolution(*frame)
            ref = _reference(r, frame)
            with options(r) as opt:
                for name in ("smallest", "largest", "smallest"):
                    for key, value in K.COMBINED[name].items():
                        opt.set(key, value)
                    assert np.array_equal(bits(_render(r)), bits(ref)), (frame, mode, name)
            assert np.array_equal(bits(_render(r)), bits(ref)), (frame, mode, "back at the defaults")
            if fresh is None:
                fresh = _make(ha, mode, 0)
                fresh.upload_scene(sc)
            fresh.set_resolution(*frame)
            assert np.array_equal(bits(_render(fresh)), bits(ref)), (frame, mode, "a fresh context")
    finally:
        r.close()
        if fresh is not None:
            fresh.close()


def test_roulette_and_precise_shading_refuse_each_other(ha, scenes):
    """The roulette estimator has no f64 instantiation: whichever of russian_roulette and precise_shading 1 is asked for second is refused with
    HR_ERR_UNSUPPORTED where it is asked for, what was in force stays, and the next render gives the bits it gave before the refused call."""
    with ha.Renderer(0) as r:
        r.set_option("batch", BATCH)
        r.upload_scene(scenes(MESH_SCENE)[0])
        r.set_resolution(*RAGGED)
        # precise shading first
        r.set_option("precise_shading", 1)
        before, shading = _render(r), r.stats()["shading_in_force"]
        assert shading == 2 and np.isfinite(before).all() and before.any()
        code, text = error_of(ha, r.set_option, "russian_roulette", 3)
        assert code == HR_ERR_UNSUPPORTED and "precise_shading" in text
        assert r.stats()["shading_in_force"] == shading
        assert np.array_equal(bits(_render(r)), bits(before))
        r.set_option("russian_roulette", 0)                  # off is no conflict
        assert error_of(ha, r.set_option, "russian_roulette", 1)[0] == HR_ERR_INVALID     # (a bad value is a bad value first)
        # the roulette first
        r.set_option("precise_shading", -1)
        plain = _render(r)
        r.set_option("russian_roulette", 3)
        before = _render(r)
        assert np.isfinite(before).all() and not np.array_equal(bits(before), bits(plain))
        code, text = error_of(ha, r.set_option, "precise_shading", 1)
        assert code == HR_ERR_UNSUPPORTED and "russian_roulette" in text
        assert r.stats()["shading_in_force"] == 0
        assert np.array_equal(bits(_render(r)), bits(before))
        r.set_option("precise_shading", 0)                   # the other values are no conflict
        r.set_option("precise_shading", -1)
        # the roulette off again: the image of before, and precise shading is accepted again
        r.set_option("russian_roulette", 0)
        assert np.array_equal(bits(_render(r)), bits(plain))
        r.set_option("precise_shading", 1)
        assert r.stats()["shading_in_force"] == 2


def test_roulette_starts_the_governor_over(ha, scenes):
    """russian_roulette changes what runs (the estimator lives in the megakernel; automatic precise shading stands back): setting it synchronises
    and starts the governor over, as precise_shading and trace_mode do — what it had decided and the budget it had settled on are gone.  (The
    headline frame: only there do the kernels run beside each other long enough to be judged, test_wave_budget_governor.)"""
    with ha.Renderer(0) as r:
        r.set_option("batch", 4)
        r.upload_scene(scenes(MESH_SCENE)[0])
        r.set_resolution(1920, 1080)
        r.render(1, 1 + 4 * 16)                              # sixteen launches in one call, governed
        r.synchronize()
        st = r.stats()
        assert st["governor_decisions"] >= 1 and st["governor_budget"] > 0, (st["governor_decisions"], st["governor_budget"])   # (24 launches: >= 12 there)
        r.set_option("russian_roulette", 3)
        st = r.stats()
        assert st["governor_decisions"] == 0 and st["governor_level"] == 0 and st["governor_budget"] == 0 and st["governor_budget_moves"] == 0
        r.render(65, 69)
        r.synchronize()
        r.set_option("russian_roulette", 0)
        assert r.stats()["governor_decisions"] == 0 and np.isfinite(r.read_accumulator()).all()
