"""Lens-sampled guide planes (hr_render_guides_lens) on the CPU tier: the table of lens points, guide_lens_ray against
camera.rs:83-96 in f64 numpy, the host form of the per-lane function (tests/guide_lens_harness.cpp, built here with g++) per ray against the same
chain in f64 over the oracle, the stated sum bit for bit, and the entry points, variant rows and CLI refusals without a device."""
import re

import numpy as np
import pytest

import guide_lens as gl
import interface_checks as ic
from cli import run_cli
from gpu_helpers import same
from schedule_knobs import SETTERS

HR_ERR_INVALID = -1
W, H = 48, 27
SHAPES = [gl.SQUARE, gl.CIRCLE]
COUNTS = [4, 16]
# guide_lens_ray (fp32) against camera.rs:83-96 in f64, over all pixels of 48x27, 4 sub-samples and the 16 lens points, on tbf3's camera and the
# hand-built scene's: 3 x the worst absolute difference observed (DESIGN §6.5's rule for a measured gate).  Observed: origin 3.88e-7 (tbf3; the
# hand-built camera 4.8e-8), direction 1.45e-7 (tbf3; the hand-built camera 1.36e-7).
TOL_RAY_ORIGIN, TOL_RAY_DIRECTION = 1.2e-6, 4.4e-7
# The host form per ray against the f64 chain, K = 2, L = 16, 48x27: test_guide_chain_cpu.py's measured gates, which are gates on the same
# functions (hit_surface, material_at, guide_chain_link).  No lens ray exceeds one of them, so they stand as they are — observed over the 82,944
# rays of each scene: albedo 4.16e-4 (rtcamp6_v3_1: the fp32 texture fetch and its gamma; the hand-built scene, untextured, 2.4e-8), normal
# 1.27e-5 (rtcamp6_v3_1; hand-built 8.2e-6), path length 5.6e-6 relative (rtcamp6_v3_1; hand-built 2.3e-6); divergent rays: none on either.
TOL_ALBEDO, TOL_NORMAL, TOL_LENGTH = 4.2e-4, 2.6e-5, 1.0e-5


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return gl.build_harness(tmp_path_factory.mktemp("guide_lens"))


@pytest.fixture(scope="module")
def wide(ha):
    return gl.wide_scene(ha)


@pytest.fixture(scope="module")
def host_lens(ha, harness, scenes, wide):
    """name -> (scene holder, HostLens); "wide" is the hand-built wide-aperture scene"""
    cache = {}

    def get(name):
        if name not in cache:
            sc = wide if name == "wide" else scenes(name)[0]
            cache[name] = (sc, gl.HostLens(harness, sc.desc_ptr))
        return cache[name]
    return get


# ---------------------------------------------------------------------------------------------------------------- the table

@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_table_properties(ha, harness, shape, count):
    uv = ha.guide_lens_points(shape, count)
    assert uv.shape == (count, 2) and uv.dtype == np.float32
    u, v = uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64)
    if shape == gl.CIRCLE:
        assert (u * u + v * v < 1.0).all()
    else:
        assert (np.abs(uv) < 1.0).all()
    assert (uv * 64 == np.round(uv * 64)).all()                                # multiples of 1/64
    points = {(float(a), float(b)) for a, b in uv}
    assert len(points) == count                                                # no point twice
    assert {(-a, -b) for a, b in points} == points                             # symmetric under (u, v) -> (-u, -v)
    assert same(uv[count // 2:], -uv[:count // 2])                             # (as the header states the order: the second half mirrors the first)
    assert u.sum() == 0.0 and v.sum() == 0.0 and np.float32(uv[:, 0]).sum() == 0.0  # the centroid, exactly
    assert same(uv, gl.harness_points(harness, shape, count))                  # the library's table is the per-lane function's


def test_table_is_the_stated_layout(ha):
    q = lambda pts: {(a / 64.0, b / 64.0) for a, b in pts}   # noqa: E731
    signs = [(1, 1), (-1, 1), (-1, -1), (1, -1)]
    half = q((32 * a, 32 * b) for a, b in signs)
    ring = q([(51, 0), (-51, 0), (0, 51), (0, -51)] + [(44 * a, 25 * b) for a, b in signs] + [(25 * a, 44 * b) for a, b in signs])
    got = lambda shape, count: {(float(a), float(b)) for a, b in ha.guide_lens_points(shape, count)}   # noqa: E731
    assert got(gl.CIRCLE, 4) == half and got(gl.SQUARE, 4) == half
    assert got(gl.CIRCLE, 16) == q((16 * a, 16 * b) for a, b in signs) | ring
    assert got(gl.SQUARE, 16) == q((a, b) for a in (-48, -16, 16, 48) for b in (-48, -16, 16, 48))


@pytest.mark.parametrize("count", [0, 1, 8, 17])
def test_other_counts_are_invalid(ha, count):
    uv = np.full((32, 2), 7.0, np.float32)
    for shape in SHAPES:
        assert ha.hip_lib().hr_guide_lens_points(shape, count, uv.ctypes.data) == HR_ERR_INVALID
    assert (uv == 7.0).all()
    with pytest.raises(ha.HipError) as e:
        ha.guide_lens_points(gl.CIRCLE, count)
    assert e.value.code == HR_ERR_INVALID
    assert ha.hip_lib().hr_guide_lens_points(2, 16, uv.ctypes.data) == HR_ERR_INVALID and ha.hip_lib().hr_guide_lens_points(1, 16, None) == HR_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- the ray

@pytest.mark.parametrize("scene", ["tbf3", "wide"])
def test_lens_ray_against_the_reference_in_f64(ha, host_lens, scene):
    sc, hl = host_lens(scene)
    assert sc.desc.camera.lens_radius > 0.05
    uv = ha.guide_lens_points(sc.desc.camera.lens_shape, 16)
    org, d = hl.rays(W, H, uv)
    org64, d64 = gl.lens_rays(sc.desc, W, H, uv)
    e_org = np.abs(org.astype(np.float64) - org64).max()
    e_dir = np.abs(d.astype(np.float64) - d64).max()
    print("%s: guide_lens_ray against f64: origin %.3g (gate %.3g), direction %.3g (gate %.3g)" % (scene, e_org, TOL_RAY_ORIGIN, e_dir, TOL_RAY_DIRECTION))
    assert e_org <= TOL_RAY_ORIGIN and e_dir <= TOL_RAY_DIRECTION
    assert np.abs(org64 - gl.gc._v(sc.desc.camera.eye)).max() > 0.5 * sc.desc.camera.lens_radius      # and the origins do leave the eye


def test_without_a_lens_offset_it_is_the_pinhole_ray(ha, harness, host_lens):
    """u = v = 0 on cameras with an aperture, and every table point on a camera with lens_radius == 0: debug_camera_ray's origin and direction,
    bit for bit (the sign of a zero included)."""
    for scene in ("tbf3", "wide"):
        sc, hl = host_lens(scene)
        org, d = hl.rays(W, H, np.zeros((1, 2), np.float32))
        org0, d0 = hl.pinhole_rays(W, H)
        assert same(org[..., 0, :], org0) and same(d[..., 0, :], d0), scene
    for target in ((0.0, 1.0, 0.0), (0.3, 0.2, -1.0)):                           # (the first camera has zero components in its basis)
        sc = gl.tiny_scene(ha, gl.WIDE_ELEMENTS, aperture=0.0, target=target)
        assert sc.desc.camera.lens_radius == 0.0
        hl = gl.HostLens(harness, sc.desc_ptr)
        for shape in SHAPES:
            uv = ha.guide_lens_points(shape, 16)
            org, d = hl.rays(W, H, uv)
            org0, d0 = hl.pinhole_rays(W, H)
            assert same(org, np.ascontiguousarray(np.broadcast_to(org0[..., None, :], org.shape))) and same(d, np.ascontiguousarray(np.broadcast_to(d0[..., None, :], d.shape)))
        hl.close()                                                              # (the PLANES of 16 equal rays are not the pinhole planes' bits: x + x + x
                                                                                #  rounds.  That is why hr_render_guides_lens runs the pinhole kernels there.)


# ---------------------------------------------------------------------------------------------------------------- the host form against f64

@pytest.fixture(scope="module")
def host_rays(ha, host_lens):
    """scene -> the host form's (per ray, info, planes) at 48x27, K = 2, L = 16, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = host_lens(name)[1].lens(W, H, 2, 16)
        return cache[name]
    return get


@pytest.mark.parametrize("scene", ["wide", "rtcamp6_v3_1"])
def test_host_form_against_the_f64_chain(ha, host_lens, host_rays, scenes, orc, scene):
    """K = 2, L = 16, per ray.  A ray is divergent when its chain has another number of hits than the f64 chain's or ends on another element; at
    most 1 % may be (a condition).  For the others: albedo within 4.2e-4 and normal within 2.6e-5 absolute, path length within 1.0e-5 relative
    (test_guide_chain_cpu.py's measured gates: the same functions), coverage equal."""
    sc, _ = host_lens(scene)
    osc = orc.OracleScene(sc.desc_ptr) if scene == "wide" else scenes(scene)[1]
    ray, info, _ = host_rays(scene)
    uv = ha.guide_lens_points(sc.desc.camera.lens_shape, 16)
    val, oinfo = gl.oracle_lens(orc, osc, sc.desc, W, H, 2, uv)
    divergent = (info != oinfo).any(-1)
    print("%s: %d of %d rays divergent; chain hits %s" % (scene, divergent.sum(), divergent.size, np.bincount(oinfo[..., 0].ravel()).tolist()))
    assert divergent.mean() <= 0.01
    ok = ~divergent
    d = np.abs(ray.astype(np.float64) - val)[ok]
    hit = val[ok][:, 7] == 1.0
    assert hit.sum() > 10000
    e_alb, e_nrm = d[:, 0:3].max(), d[:, 3:6].max()
    e_len = (d[hit][:, 6] / val[ok][hit][:, 6]).max()
    print("%s: worst albedo %.3g (gate %.3g), normal %.3g (gate %.3g), path length %.3g relative (gate %.3g)" % (scene, e_alb, TOL_ALBEDO, e_nrm, TOL_NORMAL, e_len, TOL_LENGTH))
    assert e_alb <= TOL_ALBEDO and e_nrm <= TOL_NORMAL and e_len <= TOL_LENGTH
    assert (d[:, 7] == 0.0).all() and (ray[ok][~hit] == 0.0).all()
    if scene == "rtcamp6_v3_1":
        assert (oinfo[..., 0] >= 2).sum() > 500                                  # chains that bounced are there to be compared


@pytest.mark.parametrize("scene", ["wide", "rtcamp6_v3_1"])
def test_planes_are_the_stated_sum_of_the_rays(host_lens, host_rays, scene):
    ray, _, pix = host_rays(scene)
    assert same(pix, gl.planes_of(ray))
    cover = pix[..., 7]
    assert (cover * 64 == np.round(cover * 64)).all()                            # coverage: the fraction of the 64 rays that hit
    if scene == "rtcamp6_v3_1":                                                  # (the hand-built scene is closed: every ray hits)
        assert ((cover > 0.0) & (cover < 1.0)).sum() > 10
    hl = host_lens(scene)[1]
    assert same(hl.lens(W, H, 2, 16, per_ray=False)[2], pix)
    x0, y0, w, h = 13, 9, 20, 11
    assert same(hl.lens(W, H, 2, 16, window=(x0, y0, w, h), per_ray=False)[2], np.ascontiguousarray(pix[y0:y0 + h, x0:x0 + w]))
    assert not same(hl.lens(W, H, 2, 1, per_ray=False)[2], pix)                  # and the lens does change the planes (L = 1: the pinhole ray)


def test_the_wide_scene_has_planes_that_differ(ha, harness, host_lens):
    """The hand-built scene at 96x54: the lens planes (L = 16) and the pinhole planes differ by more than 0.02 on several hundred pixels — what the
    quality test on the device needs (the issue's host measurement has 883)."""
    hl = host_lens("wide")[1]
    lens, pin = hl.lens(96, 54, 0, 16, per_ray=False)[2], hl.lens(96, 54, 0, 1, per_ray=False)[2]
    mask = gl.differ_mask(lens, pin)
    print("wide scene, 96x54: %d pixels where lens and pinhole planes differ by more than 0.02" % mask.sum())
    assert mask.sum() >= 300


# ---------------------------------------------------------------------------------------------------------------- the interface

def test_entry_points_declared_documented_exported_and_bound(ha):
    text = ic.header_text()
    assert ic.declared(text, r"int\s+hr_render_guides_lens\s*\(\s*%s\s*,\s*uint32_t\s+\w+\s*\)\s*;")
    assert re.search(r"int\s+hr_guide_lens_points\s*\(\s*int\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*float\s*\*\s*\w+\s*\)\s*;", text)
    assert ic.abi_version(text) == 7 and ha.hip_lib().hr_abi_version() == 7    # functions were added, nothing changed
    raw = ic.header_text(raw=True)
    for word in ("hr_render_guides_lens(ctx, L)", "hr_guide_lens_points(lens_shape", "lens_radius == 0", "multiples of 1/64"):
        assert word in raw, word
    assert "guide_lens" not in ic.read("include", "hanamaru_hip_debug.h") and "guides_lens" not in ic.read("include", "hanamaru_hip_debug.h")
    assert not ic.exported_and_bound(ha, ("hr_render_guides_lens", "hr_guide_lens_points"))
    L = ha.hip_lib()
    assert len(L.hr_render_guides_lens.argtypes) == 2 and len(L.hr_guide_lens_points.argtypes) == 3
    assert callable(getattr(ha.Renderer, "render_guides_lens", None)) and callable(ha.guide_lens_points)
    ffi = ic.rust_ffi()
    assert "pub fn hr_render_guides_lens(ctx: *mut HrCtx, lens_points: u32" in ffi and "pub fn hr_guide_lens_points(lens_shape: c_int, lens_points: u32, uv: *mut f32" in ffi


def test_no_option_key_was_added():
    api = ic.read("hanamaru-renderer_amd", "csrc", "hr_api.hip")
    keys = set(re.findall(r'\bk == "([a-z0-9_]+)"', api))
    assert len(keys) >= 10 and "guide_bounces" in keys and not [k for k in keys if "lens" in k]
    assert keys <= set(SETTERS), sorted(keys - set(SETTERS))


def test_variant_table_has_the_lens_rows_and_keeps_the_old_ones():
    kv = ic.kernel_variants()
    for row in ("HR_VARIANT(guide_lens_kernel, true)", "HR_VARIANT(guide_lens_kernel, false)", "select_guide_lens_kernel(bool qn)",
                "HR_VARIANT(guide_chain_kernel, true)", "HR_VARIANT(guide_chain_kernel, false)", "HR_VARIANT(guide_render_kernel, true)",
                "HR_VARIANT(guide_render_kernel, false)", "select_guide_chain_kernel(bool qn)", "select_guide_render_kernel(bool qn)"):
        assert row in kv, row
    assert "select_guide_lens_kernel(" in ic.read("hanamaru-renderer_amd", "csrc", "hr_api.hip")


def test_cli_help_lists_guide_lens(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0 and "--guide-lens L" in r.stdout


@pytest.mark.parametrize("args,word", [(["--denoise", "--guide-lens", "8"], "--guide-lens must be"), (["--guide-image", "g", "--guide-lens", "0"], "--guide-lens must be"),
                                       (["--denoise", "--guide-lens", "17"], "--guide-lens must be"), (["--denoise", "--guide-lens", "four"], "--guide-lens must be"),
                                       (["--guide-lens", "16"], "--guide-lens needs"), (["--guide-lens", "4", "--guide-bounces", "2"], "--guide-lens needs")])
def test_cli_refuses_guide_lens_before_any_device(tmp_path, args, word):
    r, left_result = ic.cli_refused(tmp_path, args)
    assert r.returncode == 1, r.stdout
    assert word in r.stdout
    assert not left_result


@pytest.mark.parametrize("flags", [["--denoise"], ["--robust", "5", "--robust-denoise"], ["--robust", "5", "--robust-restore"], ["--denoise-auto", "5"], ["--guide-image", "g"]])
def test_cli_accepts_guide_lens_with_every_flag_that_uses_guide_planes(tmp_path, flags):
    """Valid with the flags --guide-bounces is valid with: the run gets past the flag checks (and ends where it looks for its assets)."""
    r = run_cli(["--assets", tmp_path / "no_assets", "-w", "16", "-h", "12", "-s", "2", "--guide-lens", "16"] + flags, tmp_path, timeout=120)
    assert "--guide-lens needs" not in r.stdout and "--guide-lens must be" not in r.stdout
