"""Hit surfaces, textures and the sky ON THE DEVICE, point by point against the f64 oracle: the sets, the sensitivity and the check of
tests/lookup_sweeps.py through hr_debug_surface / hr_debug_sky / hr_debug_texture — v_rcp_f32 in the cuboid's and the sky's quotients, v_rsq_f32
and the device's atan2f in a sphere's coordinates, v_exp / v_log in the gamma curve, where the host emulation has libm — in both modes and on both
sky variants.  One launch of a few thousand threads per test, nothing renders.  tests/test_lookups_cpu.py asserts the sets' conditions and that
the check rejects wrong lookups.  Figures: profiles/lookup_sweeps.txt."""
import numpy as np
import pytest

import lookup_sweeps as ls
from gpu_helpers import error_of, options, same

pytestmark = pytest.mark.gpu

SKIES = sorted(ls.SKIES)
_uploaded = {}


def _with_scene(gpu, ha, orc, sky):
    """the shared renderer holding the variant's scene (uploaded again only when the last upload was another's)"""
    s, _ = ls.scene(ha, orc, sky)
    if _uploaded.get("scene") is not s or _uploaded.get("renderer") is not gpu or getattr(gpu, "_scene", None) is not s:
        gpu.upload_scene(s)
        _uploaded.update(scene=s, renderer=gpu)
    return s


def _emulated(ha, orc, emu, sky):
    if ("emu", sky) not in _uploaded:
        _uploaded[("emu", sky)] = emu.EmuScene(ls.scene(ha, orc, sky)[0].desc_ptr)
    return _uploaded[("emu", sky)]


def _no_failures(fig, fails):
    assert not fails, "%d points fail:\n%s" % (fig["failures"], "\n".join(fails))


@pytest.mark.parametrize("name", ls.SKY_SETS)
@pytest.mark.parametrize("sky", SKIES)
def test_sky_set_on_the_device(gpu, ha, orc, emu, sky, name):
    """the face the oracle's at EVERY point, the colour within max(T, K sens), the lookup in the form the variant was built for, and the
    face / quad corner the emulation's wherever the oracle's own is not fragile"""
    _with_scene(gpu, ha, orc, sky)
    p = ls.get_sky(ha, orc, sky, name)
    rgb, where = gpu.debug_sky(p["dirs"])
    fig, fails = ls.check_sky(p, rgb, where, "MI355X")
    print(ls.report_line(fig))
    _no_failures(fig, fails)
    assert ((where[:, 0] >> 3) == ls.EXPECTED_FORM[sky]).all()
    ls.same_where(p, where, _emulated(ha, orc, emu, sky).debug_sky(p["dirs"])[1], "%s/%s" % (name, sky))
    if len(p["undefined"]):
        u_rgb, _ = gpu.debug_sky(p["undefined"])
        print("lookups %s/%s [MI355X]: %d of %d answers on the x == y, z == 0 ties are finite" % (name, sky, int(np.isfinite(u_rgb).all(axis=1).sum()), len(u_rgb)))


@pytest.mark.parametrize("sky", SKIES)
def test_texture_set_on_the_device(gpu, ha, orc, emu, sky):
    _with_scene(gpu, ha, orc, sky)
    p = ls.get_texture(ha, orc, sky)
    rgb, rough64, quad = gpu.debug_texture(p["image"], p["uv"])
    fig, fails = ls.check_texture(p, rgb, rough64, quad, "MI355X")
    print(ls.report_line(fig))
    _no_failures(fig, fails)
    ls.same_where(p, quad, _emulated(ha, orc, emu, sky).debug_texture(p["image"], p["uv"])[2], "texture/%s" % sky)


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("name", ls.SURFACE_SETS)
@pytest.mark.parametrize("sky", SKIES)
def test_surface_set_on_the_device(gpu, ha, orc, sky, name, precise):
    """hit_surface + material_at (fp32 mode) and shade_hit_f64 (precise mode) on every surface set; the scene's surfaces are the same under both skies"""
    _with_scene(gpu, ha, orc, sky)
    fig, fails, _ = ls.run_surface(ha, orc, gpu, name, precise, "MI355X, %s sky" % sky)
    _no_failures(fig, fails)


@pytest.mark.parametrize("quant", [0, 1])
def test_axis_rays_through_the_render_kernels_traversal(gpu, ha, orc, quant):
    """Rays with direction components of exactly +0.0 and -0.0 (ray_set's sign-bit octants, clamp_inv, cuboid_test's 1 / 0) through hr_debug_trace on
    the 32-byte and on the quantised nodes: hit, element and distance bit-identical to the scalar walk's, and the oracle's hit and element."""
    s, o = ls.scene(ha, orc, "nonsquare")
    p = ls.get_surface(ha, orc, "axis_rays")
    with options(gpu, {"quant_nodes": quant}):
        gpu.upload_scene(s)
        _uploaded.clear()
        got, gel = gpu.debug_trace(p["rays"])
        ref, rel = gpu.debug_intersect(p["rays"])
    _uploaded.clear()
    assert same(got[:, :2], ref[:, :2]) and np.array_equal(gel, rel)
    assert np.array_equal(got[:, 0] != 0, p["decision"][:, 0] != 0) and np.array_equal(gel, p["decision"][:, 1])
    t = p["ref"][:, 1]
    assert (np.abs(got[:, 1] - t) <= np.maximum(ls.T, ls.K * p["sens"]) * np.maximum(1.0, np.abs(t))).all()


def test_queries_answer_bad_arguments_with_an_error(gpu, ha, orc):
    _with_scene(gpu, ha, orc, "nonsquare")
    code, text = error_of(ha, gpu.debug_texture, [0, 10], [[0.5, 0.5], [0.5, 0.5]])
    assert code == -1 and "image 10" in text, (code, text)
    code, text = error_of(ha, gpu.debug_texture, [-1], [[0.5, 0.5]])
    assert code == -1, (code, text)
    rgb, rough, quad = gpu.debug_texture([9], [[0.5, 0.5]])          # and goes on answering
    assert np.isfinite(rgb).all()
