"""Hit surfaces, textures and the sky, point by point (tests/lookup_sweeps.py), CPU tier: the conditions every point set must meet on the oracle
alone, every set through the host emulation of hr_debug_surface / hr_debug_sky / hr_debug_texture (csrc/query_core.h, the per-point code the
device runs) in both modes and on both sky variants, and the proof that the check rejects subtly wrong lookups.  The twin of
tests/test_lookups_gpu.py.  Figures: profiles/lookup_sweeps.txt."""
import numpy as np
import pytest

import lookup_sweeps as ls

SKIES = sorted(ls.SKIES)


@pytest.fixture(scope="module")
def emulated(ha, orc, emu):
    """{sky variant: the emulated scene}"""
    return {sky: emu.EmuScene(ls.scene(ha, orc, sky)[0].desc_ptr) for sky in SKIES}


def _no_failures(fig, fails):
    assert not fails, "%d points fail:\n%s" % (fig["failures"], "\n".join(fails))


# ------------------------------------------------------------------------------------------ the sets, on the oracle alone
@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("name", ls.SURFACE_SETS)
def test_surface_set_meets_its_conditions(ha, orc, name, precise):
    """FRAGILE share within the cap (0.01; 0.5 for the edge sets; B's points recorded only), every face centre of A, B and C and every grazing ray
    with b / r <= 0.9999 a solid hit, >= 200 comparable points, and on `general` the share that needs the sensitivity clause <= MAX_CLAUSE."""
    fig = ls.surface_conditions(ls.get_surface(ha, orc, name, precise))
    print("lookups %s [oracle, %s]: %s" % (name, "precise" if precise else "fp32", fig))


def test_face_centres_of_the_far_cuboid_are_in_the_set(ha, orc):
    """hit_surface's nearest-face fallback needs |pos| >~ 1700: B's face centres are there, and they are hits of B that no fp32 move of the ray turns"""
    p = ls.get_surface(ha, orc, "cuboid_faces")
    far = p["must_be_solid"] & (p["box"] == "B")
    assert far.sum() == 24 and (p["decision"][far, 1] == ls.ELEMENT["B"]).all() and not p["fragile"][far].any()
    assert (np.sqrt((p["ref"][far][:, ls.POS_COLS] ** 2).sum(-1)) > 1700).all()
    assert sorted(set(p["decision"][far, 2].tolist())) == list(range(6))


@pytest.mark.parametrize("sky", SKIES)
@pytest.mark.parametrize("name", ls.SKY_SETS)
def test_sky_set_meets_its_conditions(ha, orc, sky, name):
    """all six faces, the oracle finite on every point — and NOT finite on the x == y, z == 0 ties the seams leave out"""
    print("lookups %s/%s [oracle]: %s" % (name, sky, ls.sky_conditions(ls.get_sky(ha, orc, sky, name))))


@pytest.mark.parametrize("sky", SKIES)
def test_texture_set_meets_its_conditions(ha, orc, sky):
    p = ls.get_texture(ha, orc, sky)
    fig = ls.texture_conditions(p)
    assert fig["images"] == 10 and {tuple(a.shape[1::-1]) for a in ls.scene(ha, orc, sky)[0].arrays} >= set(ls.cs.SURFACE_IMAGES)
    print("lookups texture/%s [oracle]: %s" % (sky, fig))


# ------------------------------------------------------------------------------------------ the emulation
@pytest.mark.parametrize("sky", SKIES)
def test_each_sky_variant_is_on_the_form_intended(emulated, sky):
    """six faces of one size: the footprint table; six sizes: the per-face lookup"""
    assert emulated[sky].sky_form() == ls.EXPECTED_FORM[sky]


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("name", ls.SURFACE_SETS)
def test_emulation_surface_set(ha, orc, emulated, name, precise):
    fig, fails, _ = ls.run_surface(ha, orc, emulated["nonsquare"], name, precise, "emulation")
    _no_failures(fig, fails)


@pytest.mark.parametrize("sky", SKIES)
@pytest.mark.parametrize("name", ls.SKY_SETS)
def test_emulation_sky_set(ha, orc, emulated, sky, name):
    p = ls.get_sky(ha, orc, sky, name)
    fig, fails = ls.check_sky(p, *emulated[sky].debug_sky(p["dirs"]), "emulation")
    print(ls.report_line(fig))
    _no_failures(fig, fails)
    if len(p["undefined"]):          # where the reference is undefined the answer is recorded, not judged
        rgb, _ = emulated[sky].debug_sky(p["undefined"])
        print("lookups %s/%s [emulation]: %d of %d answers on the x == y, z == 0 ties are finite" % (name, sky, int(np.isfinite(rgb).all(axis=1).sum()), len(rgb)))


@pytest.mark.parametrize("sky", SKIES)
def test_emulation_texture_set(ha, orc, emulated, sky):
    p = ls.get_texture(ha, orc, sky)
    fig, fails = ls.check_texture(p, *emulated[sky].debug_texture(p["image"], p["uv"]), "emulation")
    print(ls.report_line(fig))
    _no_failures(fig, fails)


# ------------------------------------------------------------------------------------------ the check has teeth
def _mutant_images(ha, emu, sky, change):
    """the emulation of the scene with every image put through `change` — the lookups of a kernel that reads its images that way"""
    def mutate(s):
        for k in range(len(s.arrays)):
            ls.set_image(s, k, change(s.arrays[k]))
    s = ls.build_scene(ha, sky, mutate)
    return emu.EmuScene(s.desc_ptr), s


def _clamp_x_against_height(a):
    h, w = a.shape[:2]
    if w <= h:
        return a
    b = a.copy()
    b[:, h:] = a[:, h - 1:h]
    return b


def test_check_rejects_u_and_v_swapped(ha, orc, emulated):
    p = ls.get_texture(ha, orc, "nonsquare")
    fig, fails = ls.check_texture(p, *emulated["nonsquare"].debug_texture(p["image"], p["uv"][:, ::-1]), "u and v swapped")
    assert fails and fig["failures"] > 100, fig


def test_check_rejects_a_face_with_w_and_h_swapped(ha, orc, emu):
    e, keep = _mutant_images(ha, emu, "nonsquare", lambda a: a.reshape(a.shape[1], a.shape[0], 4) if a.shape[:2] == (5, 12) else a)
    p = ls.get_sky(ha, orc, "nonsquare", "sky_texels")
    fig, fails = ls.check_sky(p, *e.debug_sky(p["dirs"]), "w and h swapped")
    assert fails and fig["failures"] > 100, fig


def test_check_rejects_the_row_not_flipped(ha, orc, emu):
    e, keep = _mutant_images(ha, emu, "nonsquare", lambda a: a[::-1])
    p = ls.get_texture(ha, orc, "nonsquare")
    fig, fails = ls.check_texture(p, *e.debug_texture(p["image"], p["uv"]), "row not flipped")
    assert fails and fig["failures"] > 100, fig
    q = ls.get_sky(ha, orc, "nonsquare", "sky_texels")
    assert ls.check_sky(q, *e.debug_sky(q["dirs"]), "row not flipped")[1]


def test_check_rejects_x_clamped_against_the_height(ha, orc, emu):
    e, keep = _mutant_images(ha, emu, "nonsquare", _clamp_x_against_height)
    p = ls.get_texture(ha, orc, "nonsquare")
    fig, fails = ls.check_texture(p, *e.debug_texture(p["image"], p["uv"]), "x clamped against the height")
    assert fails and fig["failures"] > 100, fig


def test_check_rejects_the_cascade_with_x_and_z_exchanged(ha, orc, emulated):
    p = dict(ls.get_surface(ha, orc, "cuboid_faces"))
    out, out64, elem = emulated["nonsquare"].debug_surface(p["rays"], p["fix"], p["draws"], False)
    out = out.copy()
    out[:, [5, 7]] = out[:, [7, 5]]                                     # the normal's x and z
    out[:, 10] = np.array([0, 1, 4, 5, 2, 3, 6])[out[:, 10].astype(int)]  # and the face that goes with it
    fig, fails = ls.check_surface(p, out, out64, elem, "X and Z exchanged", False)
    assert fails and fig["failures"] > 100, fig


def test_check_rejects_sphere_lo_dropped(ha, orc, emu):
    """S1 with its centre and radius rounded to fp32 — a kernel that forgets Scene::sphere_lo: the normal of an r = 0.1 sphere moves by up to
    6e-8 x |c| / r = 1e-6, which precise shading's bound (one fp32 ulp) sees"""
    c, r = ls.S1
    s = ls.build_scene(ha, "nonsquare", s1_centre=c.astype(np.float32).astype(np.float64), s1_radius=float(np.float32(r)))
    fig, fails, _ = ls.run_surface(ha, orc, emu.EmuScene(s.desc_ptr), "sphere_uv", True, "sphere_lo dropped")
    assert fails and fig["failures"] > 20, fig


def test_check_rejects_the_fix_dropped(ha, orc, emulated):
    class NoFix:
        def debug_surface(self, rays, fix, draws, precise):
            return emulated["nonsquare"].debug_surface(rays, None, draws, precise)
    fig, fails, _ = ls.run_surface(ha, orc, NoFix(), "sphere_uv", True, "fix dropped")
    assert fails and fig["failures"] > 100, fig
    fig, fails, _ = ls.run_surface(ha, orc, NoFix(), "general", True, "fix dropped")
    assert fails, fig


def test_check_rejects_the_quad_tables_last_column_off_by_one(ha, orc, emu):
    e = emu.EmuScene(ls.scene(ha, orc, "nonsquare")[0].desc_ptr)
    e.break_sky_quads()
    p = ls.get_sky(ha, orc, "nonsquare", "sky_seams")
    rgb, where = e.debug_sky(p["dirs"])
    assert (where[:, 1] == 12).any(), "no point of the set reads the table's last corner column"
    fig, fails = ls.check_sky(p, rgb, where, "last column off by one")
    assert fails and fig["failures"] >= int((where[:, 1] == 12).sum()) // 2, fig
