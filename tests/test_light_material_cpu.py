"""Light and material scenes (tests/light_material_scenes.py), CPU tier: what makes every case a case (asserted on the oracle's log alone), how
discontinuous the reference is on every case (the source of the caps), the host emulation of the kernels' per-lane code against the oracle,
path by path, and nee_setup's shortcuts on against off — the twin of tests/test_light_material_gpu.py.  The emulation computes with libm
where the device uses its rcp / rsq / sin / exp / log instructions: this tier speaks for the written form of the code, the GPU tier for the
device."""
import numpy as np
import pytest

import light_material_scenes as lm

ALL = sorted(lm.CASES)
LIGHT_CASES = sorted(lm.LIGHT_CASES)
MATERIAL_CASES = sorted(lm.MATERIAL_CASES)

# share of the paths with an NEE-visible bit in some iteration, at least
MIN_VISIBLE = {"tiny": 0.30, "marginal": 0.30, "many": 0.30, "touching": 0.15, "close": 0.15, "overlap": 0.15, "shell_emits": 0.15, "inside": 0.15,
               "large": 0.04}


@pytest.mark.parametrize("name", LIGHT_CASES)
def test_light_case_is_lit_by_next_event_estimation(ha, orc, name):
    _, ref = lm.get(ha, orc, name)
    share = lm.nee_visible_share(ref)
    print("%s: %.3f of the paths have an NEE-visible bit" % (name, share))
    assert share >= MIN_VISIBLE[lm.light_case(name)], (name, share)


@pytest.mark.parametrize("floor", lm.FLOORS)
def test_shell_emits_adds_the_shells_emission(ha, orc, floor):
    """the shadow ray's closest hit is the shell: what the oracle renders changes with the shell's tint (emitter 1 of the case), the branches do not"""
    name = "shell_emits-" + floor
    _, ref = lm.get(ha, orc, name)
    other = lm.oracle_log(orc, lm.CASES[name][1](ha, vary=("tint", 1, (5.0, 2.0, 5.0))))
    assert np.array_equal(ref[2], other[2]) and np.array_equal(ref[3], other[3])
    lit = ((ref[2][..., :9] & 0xf0) != 0).any(axis=-1)
    changed = np.abs(ref[0] - other[0]).max(axis=-1) > 1e-3
    assert lit.mean() >= 0.15 and (changed & lit).sum() >= 0.5 * lit.sum(), (lit.mean(), changed.mean())
    # ... and the emitter's own tint adds nothing through NEE: its samples are seen through the shell, whose emission is what is added
    dark = lm.oracle_log(orc, lm.CASES[name][1](ha, vary=("tint", 0, (9.0, 9.0, 9.0))))
    first = (ref[2][..., 0] & 7) == (5 if floor == "ggx" else 2)
    one_bounce = first & (ref[2][..., 1] & 7 == 1)                       # the floor, then the sky: NEE is the only light
    assert one_bounce.sum() > 1000 and np.array_equal(ref[0][one_bounce], dark[0][one_bounce])


@pytest.mark.parametrize("floor", lm.FLOORS)
def test_many_every_emitter_is_seen(ha, orc, floor):
    """the log folds emitter k into bit k mod 4: nine variants in which only emitter k emits (the geometry stays) tell them apart"""
    name = "many-" + floor
    assert len(lm.LIGHTS["many"]) == 9
    for k in range(9):
        s = lm.CASES[name][1](ha, vary=("only", k))
        assert len(lm.emitters_of(s)) == 1
        log = lm.oracle_log(orc, s)
        seen = int(((log[2][..., :9] & 0x10) != 0).any(axis=-1).sum())
        assert ((log[2][..., :9] & 0xe0) == 0).all() and seen >= 50, (name, k, seen)


def test_corridor_ends_at_the_bounce_limit(ha, orc):
    _, ref = lm.get(ha, orc, "corridor")
    share = float((ref[2][..., 8] != 0).mean())
    print("corridor: %.3f of the paths reach iteration 9" % share)
    assert share >= 0.9


@pytest.mark.parametrize("name", MATERIAL_CASES)
def test_material_case_shows_every_object(ha, orc, name):
    """every one of the eight objects is the first hit of at least 50 paths: the oracle's closest hit along the pinhole's rays (ray_with_dof,
    camera.rs:83-96, with a lens radius of 0; the sub-sample's coordinate of renderer.rs:52-53)"""
    s, ref = lm.get(ha, orc, name)
    cam = s.desc.camera
    v = lambda a: np.array([a.x, a.y, a.z])
    y, x, sub = np.meshgrid(np.arange(s.h), np.arange(s.w), np.arange(4), indexing="ij")
    m = float(min(s.w, s.h))
    ncx = ((x + (sub & 1) * 0.5 - 0.5) * 2.0 - s.w) / m
    ncy = (((s.h - y) + (sub >> 1) * 0.5 - 0.5) * 2.0 - s.h) / m
    d = ncx[..., None] * v(cam.plane_half_right) + ncy[..., None] * v(cam.plane_half_up) + cam.focus_distance * v(cam.forward)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    rays = np.concatenate([np.broadcast_to(v(cam.eye), d.shape), d], axis=-1).reshape(-1, 6)
    _, el = orc.OracleScene(s.desc_ptr).intersect(rays)
    counts = np.bincount(el[el >= 0], minlength=len(s.elements))
    print("%s: first hits per element %s" % (name, counts.tolist()))
    assert (counts[lm.FIRST_OBJECT:lm.FIRST_OBJECT + 8] >= 50).all(), (name, counts)
    assert (el >= 0).sum() == ((ref[2][..., 0] & 7) != 1).sum()                      # the pinhole's rays are the log's first rays
    if name in ("mat_ior", "mat_ggx_ior"):
        share = float(((ref[2][..., :9] & 8) != 0).any(axis=-1).mean())
        print("%s: %.3f of the paths carry a transmitted bit" % (name, share))
        assert share >= 0.03


@pytest.mark.parametrize("name", LIGHT_CASES + MATERIAL_CASES)
def test_check_notices_a_change_of_one_percent(ha, orc, name):
    """check() on two ORACLE logs fails when one emitter's radius (light cases) or one object's roughness or index (material cases) is 1 % off:
    a case that survived would be too dull to notice a wrong constant"""
    _, ref = lm.get(ha, orc, name)
    if lm.CASES[name][0] == lm.LIGHT:
        vary = ("radius", lm.SENSITIVE_EMITTER.get(lm.light_case(name), 0), 1.01)
    else:
        vary = lm.SENSITIVE_OBJECT[name] + (1.01,)
    got = lm.oracle_log(orc, lm.CASES[name][1](ha, vary=vary))
    with pytest.raises(AssertionError):
        lm.check(name, got, ref, "oracle, %s %d x 1.01" % vary[:2])


@pytest.mark.parametrize("name", ALL)
def test_reference_discontinuity_is_what_the_caps_were_derived_from(ha, orc, name):
    """The oracle on the case as built against the oracle on the nudged case (the eye by 2^-22 of its distance to the target, every emitter's
    centre and radius by 2^-22 relative): the count of paths that change IS NUDGE_MEASURED's, and it is at most 0.1 % of the paths."""
    count, worst, n = lm.nudge_count(ha, orc, name)
    print("%s: %d of %d paths change under the nudge, worst same-branch change %.3g" % (name, count, n, worst))
    assert count <= lm.MAX_NUDGE_SHARE * n, (name, count, n)
    rec_count, rec_worst = lm.NUDGE_MEASURED[name]
    assert count == rec_count and worst <= rec_worst, (name, count, worst, lm.NUDGE_MEASURED[name])


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_emulation_path_by_path(ha, orc, emu, name, precise):
    """path_advance<.., LOG> (and <.., PREC>) of pt_core.h / prec_core.h on the host against the oracle's path log: light_material_scenes.check."""
    s, ref = lm.get(ha, orc, name)
    e = emu.EmuScene(s.desc_ptr)
    try:
        emu.set_precise(precise)
        got = e.path_log(s.w, s.h, 1)
    finally:
        emu.set_precise(False)
    a = lm.check(name, got, ref, "emulation, precise" if precise else "emulation, fp32")
    assert a["paths"] == s.w * s.h * 4


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("name", LIGHT_CASES)
def test_nee_culls_do_not_change_a_bit_here_either(ha, orc, emu, name, precise):
    """tests/test_emu_parity.py test_nee_culls_do_not_change_a_bit on the light cases: with nee_setup's shortcuts off the per-lane code renders
    the same accumulator and writes the same path log, bit for bit, from more rays — and no shortcut fires on an emitter whose diameter lies
    inside the proximity window (tiny), where a far-side sample IS seen."""
    s, _ = lm.get(ha, orc, name)
    e = emu.EmuScene(s.desc_ptr)
    try:
        emu.set_precise(precise)
        emu.set_nee_cull(True)
        a, ca = e.render(s.w, s.h, 1, 5)
        la = e.path_log(s.w, s.h, 1)
        emu.set_nee_cull(False)
        b, cb = e.render(s.w, s.h, 1, 5)
        lb = e.path_log(s.w, s.h, 1)
    finally:
        emu.set_nee_cull(True)
        emu.set_precise(False)
    assert a.sum() > 0 and np.array_equal(a, b)
    for x, y in zip(la, lb):
        assert np.array_equal(x, y)
    print("%s, precise %d: %d of %d shadow and main rays not traced" % (name, precise, ca["shadow_culled"], cb["rays"]))
    assert cb["shadow_culled"] == 0 and ca["rays"] + ca["shadow_culled"] == cb["rays"]
    if lm.light_case(name) == "tiny":
        assert ca["shadow_culled"] == 0
    else:
        assert ca["shadow_culled"] > 0


@pytest.mark.parametrize("name", ALL)
def test_split_pipeline_is_the_same_arithmetic_here_either(ha, orc, emu, name):
    """csrc/wf_core.h holds nee_setup's constants and the shadow branch a second time (the split pipeline's per-lane code): driven path by path
    on the host it renders the megakernel's accumulator, bit for bit, with the shortcuts on and off.  (On the GPU:
    tests/test_light_material_gpu.py test_split_pipeline_renders_the_same_bits.)"""
    s, _ = lm.get(ha, orc, name)
    e = emu.EmuScene(s.desc_ptr)
    a, _ = e.render(s.w, s.h, 1, 3)
    b = e.render_wf(s.w, s.h, 1, 3)
    try:
        emu.set_nee_cull(False)
        c = e.render_wf(s.w, s.h, 1, 3)
    finally:
        emu.set_nee_cull(True)
    assert a.sum() > 0 and np.array_equal(a, b) and np.array_equal(a, c)
