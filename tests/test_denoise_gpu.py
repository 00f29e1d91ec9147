"""Guide planes and the à-trous denoiser on the MI355X.  The guide pass against the debug renderer it is a sibling of, its region
and node-format contracts bit for bit; hr_denoise against csrc/denoise_core.h compiled for the host, bit for bit (the filter has no tolerance: f64,
+ - x / max, no contraction); its resolve against hr_resolve / hr_resolve_counted byte for byte; the state rules; and that the default
parameters lower the error of a 16-sampling render."""
import ctypes as C

import numpy as np
import pytest

import ckpt
from cli import ASSETS, run_cli
from gpu_helpers import error_of, renderer, same
from post_cores import core, core_denoise  # noqa: F401  (core: the g++-built harness, a fixture)
from post_numpy import synthetic_inputs

pytestmark = pytest.mark.gpu

HR_ERR_INVALID = -1
W, H, S = 96, 54, 16
SCENES = ["spheres", "rtcamp6_v3_1"]
REGIONS = {"frame": None, "window": (29, 17, 40, 24), "45x27": (13, 9, 45, 27)}


def _make(ha, sc, region=None, moments=True, counts=False, opts=None):
    return renderer(ha, sc, opts, None, (W, H), region, moments=moments, counts=counts)


def _err(ha, fn, *a, **kw):
    return error_of(ha, fn, *a, **kw)[0]


def _window(full, region):
    if region is None:
        return full
    x0, y0, w, h = region
    return np.ascontiguousarray(full[y0:y0 + h, x0:x0 + w])


# ---------------------------------------------------------------------------------------------------------------- guide planes

@pytest.fixture(scope="module")
def full_guides(ha, scenes):
    """(scene, quant_nodes) -> the full-frame guide planes, rendered once."""
    cache = {}

    def get(name, qn):
        if (name, qn) not in cache:
            r = _make(ha, scenes(name)[0], moments=False, opts={"quant_nodes": qn})
            r.render_guides()
            cache[(name, qn)] = r.read_guides()
            r.close()
        return cache[(name, qn)]
    return get


@pytest.mark.parametrize("qn", [1, 0])
@pytest.mark.parametrize("scene", SCENES)
def test_guides_against_the_debug_renderer(ha, scenes, full_guides, scene, qn):
    """Normal and depth are what hr_render_debug modes 1 and 2 show.  A sub-sample that misses is sky colour in the debug renderer and eight zeros
    in the guides, so the comparison is over the pixels whose four sub-samples all hit (coverage 1): hundreds of them in either scene.  Normal: the
    guide is the sum x 0.25f (exact), so x 4 gives the debug accumulator's bits.  Depth: the guide is sum(t) x 0.25, the debug value
    sum(0.5 t rcp(focus)) — three fp32 roundings and a 1-ulp reciprocal on one side, two roundings on the other, under 5e-7: bound 1e-6.
    Partly covered pixels have no independent source for normal and depth (the debug renderer mixes sky into them); for them the albedo test and
    the region / node-format identities are what there is."""
    g = full_guides(scene, qn)
    cov = g[..., 7]
    assert set(np.unique(cov)) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    hit = cov == 1.0
    assert hit.sum() > 500
    r = _make(ha, scenes(scene)[0], moments=False, opts={"quant_nodes": qn})
    r.render_debug(1)
    normal = r.read_accumulator()
    r.clear()
    r.render_debug(2)
    depth = r.read_accumulator()
    r.close()
    assert same((g[..., 3:6] * np.float32(4.0))[hit], normal[hit])
    focus = np.float32(scenes(scene)[0].desc.camera.focus_distance)
    want = depth[..., 0].astype(np.float64) * 2.0 * float(focus) / 4.0
    rel = np.abs(g[..., 6].astype(np.float64) - want)[hit] / want[hit]
    print("depth against mode 2: worst relative difference %.3g" % rel.max())
    assert rel.max() <= 1e-6
    assert (g[cov == 0.0] == 0.0).all()
    assert (g[..., 0:3] >= 0.0).all() and np.isfinite(g).all()


def _constant_albedo_scene(ha, colour):
    import random_scenes
    sc = random_scenes.build(ha, 3, spheres=10, cuboids=3, meshes=2)
    el = sc.keep[1]
    for i in range(sc.num_elements):
        el[i].material.albedo.color = ha.Vec3(*colour)
        el[i].material.albedo.image = -1
    return sc


@pytest.mark.parametrize("qn", [1, 0])
def test_albedo_plane_on_a_scene_of_one_colour(ha, qn):
    colour = (0.75, 0.5, 0.25)                                   # fp32 values: four of them sum exactly, x 0.25 gives them back
    sc = _constant_albedo_scene(ha, colour)
    r = _make(ha, sc, moments=False, opts={"quant_nodes": qn})
    r.render_guides()
    g = r.read_guides()
    r.close()
    cov = g[..., 7]
    assert (cov == 1.0).sum() > 100
    assert (g[cov == 1.0][:, 0:3] == np.float32(colour)).all()
    assert (g[cov == 0.0] == 0.0).all()
    part = (cov > 0.0) & (cov < 1.0)
    assert (g[part][:, 0:3] == cov[part][:, None] * np.float32(colour)).all()   # misses add zeros


@pytest.mark.parametrize("qn", [1, 0])
@pytest.mark.parametrize("region", ["window", "45x27"])
@pytest.mark.parametrize("scene", SCENES)
def test_region_guides_are_the_frames_window(ha, scenes, full_guides, scene, region, qn):
    r = _make(ha, scenes(scene)[0], region=REGIONS[region], moments=False, opts={"quant_nodes": qn})
    r.render_guides()
    g = r.read_guides()
    r.close()
    assert same(g, _window(full_guides(scene, qn), REGIONS[region]))


def test_guide_pass_touches_nothing_else_and_ignores_the_mask(ha, scenes, full_guides):
    r = _make(ha, scenes("rtcamp6_v3_1")[0], counts=True)
    r.render(1, 5)
    mask = np.zeros(((H + 3) // 4, (W + 3) // 4), np.uint8)
    mask[2:5, 3:9] = 1
    r.set_tile_mask(mask)
    r.render(5, 7)
    before = (r.read_accumulator(), r.read_moments(), r.read_sample_counts(), r.stats())
    assert _err(ha, r.read_guides) == HR_ERR_INVALID            # none yet
    r.render_guides()
    g = r.read_guides()
    after = (r.read_accumulator(), r.read_moments(), r.read_sample_counts(), r.stats())
    assert same(before[0], after[0]) and same(before[1][0], after[1][0]) and before[1][1] == after[1][1] and np.array_equal(before[2], after[2])
    assert before[3]["paths"] == after[3]["paths"] and after[3]["debug_launches"] == before[3]["debug_launches"] + 1
    assert after[3]["trace_launches"] == before[3]["trace_launches"] and after[3]["debug_kernel_ms"] > before[3]["debug_kernel_ms"]
    assert same(g, full_guides("rtcamp6_v3_1", 1))              # the whole region, whatever the mask
    r.clear()
    assert same(r.read_guides(), g)                             # hr_clear keeps them
    r.set_region(1, 1, 20, 10)
    assert _err(ha, r.read_guides) == HR_ERR_INVALID            # the target went, they went
    r.close()


def test_write_guides_round_trips(ha):
    r = _make(ha, None, moments=False)
    g = np.random.default_rng(1).normal(size=(H, W, 8)).astype(np.float32)
    r.write_guides(g)
    assert same(r.read_guides(), g)
    r.close()


# ---------------------------------------------------------------------------------------------------------------- the filter, to the bit

CASES = [dict(levels=1, demodulate=1), dict(levels=4, demodulate=1), dict(levels=5, demodulate=1),
         dict(levels=1, demodulate=0), dict(levels=4, demodulate=0), dict(levels=5, demodulate=0)]


@pytest.mark.parametrize("region", ["frame", "45x27"])
@pytest.mark.parametrize("scene", SCENES)
def test_denoise_equals_the_host_core(ha, scenes, core, scene, region):
    r = _make(ha, scenes(scene)[0], region=REGIONS[region])
    r.render(1, S + 1)
    r.denoise()                                                  # renders the guides itself
    acc, (mom, n), g = r.read_accumulator(), r.read_moments(), r.read_guides()
    assert n == S
    for case in CASES:
        r.denoise(**case)
        got = r.read_denoised()
        want = core_denoise(core, acc, mom, n, g, **case)
        assert np.isfinite(got).all()
        assert same(got, want), case
        r.denoise(**case)
        assert same(r.read_denoised(), got)                     # two calls, identical bits
    raw = core_denoise(core, acc, mom, n, g, levels=0)
    assert not same(got, raw)
    r.close()


@pytest.mark.parametrize("scene", SCENES)
def test_denoise_with_unequal_counts_equals_the_host_core(ha, scenes, core, scene):
    r = _make(ha, scenes(scene)[0], counts=True)
    r.render(1, S // 2 + 1)
    e = r.noise_image()
    pad = np.full((((H + 3) // 4) * 4, ((W + 3) // 4) * 4), -np.inf)
    pad[:H, :W] = e
    tile_max = pad.reshape((H + 3) // 4, 4, (W + 3) // 4, 4).max(axis=(1, 3))
    active = r.select_tiles(threshold=float(np.median(tile_max)))           # about half of the tiles go on
    assert 0 < active < ((H + 3) // 4) * ((W + 3) // 4)
    r.render(S // 2 + 1, S + 1)
    acc, (mom, n), cnt = r.read_accumulator(), r.read_moments(), r.read_sample_counts()
    assert n == S and set(np.unique(cnt)) == {S // 2, S}
    r.denoise()
    g = r.read_guides()
    for case in (dict(levels=4, demodulate=1), dict(levels=5, demodulate=0)):
        r.denoise(**case)
        assert same(r.read_denoised(), core_denoise(core, acc, mom, cnt, g, **case)), case
    r.denoise(levels=0)
    assert np.array_equal(r.resolve_denoised(), r.resolve_counted())
    r.close()


@pytest.mark.parametrize("w,h", [(1, 1), (37, 23), (5, 1), (1, 5)])
@pytest.mark.parametrize("unequal", [False, True])
def test_denoise_of_written_inputs_equals_the_host_core(ha, core, w, h, unequal):
    counts = np.random.default_rng(3).integers(2, 20, size=(h, w)) if unequal else None
    acc, mom, n, g = synthetic_inputs(7, w, h, counts)
    r = ha.Renderer(0)                                           # no scene: everything is written
    r.set_resolution(w, h)
    r.set_option("moments", 1)
    if unequal:
        r.set_option("sample_counts", 1)
        r.write_sample_counts(n)
    r.write_accumulator(acc)
    r.write_moments(mom, int(np.max(n)))
    r.write_guides(g)
    for case in (dict(levels=5, demodulate=1), dict(levels=5, demodulate=0), dict(levels=2, demodulate=1), dict(levels=0, demodulate=1)):
        r.denoise(**case)
        assert same(r.read_denoised(), core_denoise(core, acc, mom, n, g, **case)), case
    r.close()


# ---------------------------------------------------------------------------------------------------------------- resolve and state

@pytest.mark.parametrize("scene", SCENES)
def test_resolve_of_level_zero_is_the_resolve(ha, scenes, scene):
    r = _make(ha, scenes(scene)[0])
    r.render(1, S + 1)
    for dem in (0, 1):
        r.denoise(levels=0, demodulate=dem)
        assert np.array_equal(r.resolve_denoised(), r.resolve(S))
    r.denoise()
    img = r.resolve_denoised()
    assert img.shape == (H, W, 3) and not np.array_equal(img, r.resolve(S))
    r.close()


def test_state_rules(ha, scenes):
    sc = scenes("spheres")[0]
    r = _make(ha, sc, moments=False)
    r.render(1, 5)
    assert _err(ha, r.denoise) == HR_ERR_INVALID                # option moments is off
    assert _err(ha, r.read_denoised) == HR_ERR_INVALID and _err(ha, r.resolve_denoised) == HR_ERR_INVALID
    r.set_option("moments", 1)
    assert _err(ha, r.denoise) == HR_ERR_INVALID                # no sampling behind the moments
    r.render(1, 2)
    assert _err(ha, r.denoise) == HR_ERR_INVALID                # one: a variance needs two
    r.render(2, 5)
    r.denoise()
    d = r.read_denoised()
    acc, mom = r.read_accumulator(), r.read_moments()
    # refused parameters leave D as it was
    for bad in (dict(levels=6), dict(demodulate=2), dict(sigma_color=0.0), dict(sigma_normal=-1.0), dict(sigma_albedo=float("nan")), dict(sigma_depth=float("inf"))):
        assert _err(ha, r.denoise, **bad) == HR_ERR_INVALID, bad
        assert same(r.read_denoised(), d)
    assert ha.hip_lib().hr_denoise(r._h, None) == 0              # NULL: the defaults
    assert same(r.read_denoised(), d)
    assert same(r.read_accumulator(), acc) and same(r.read_moments()[0], mom[0])     # the denoiser writes none of its inputs
    # whatever changes an input invalidates D
    g = r.read_guides()
    cnt = np.full((H, W), 4, np.uint32)
    steps = [lambda: r.render(5, 6), lambda: r.write_accumulator(acc), lambda: r.write_moments(*mom), lambda: r.write_guides(g), r.render_guides, r.clear]
    for step in steps:
        r.denoise()
        r.read_denoised()
        step()
        assert _err(ha, r.read_denoised) == HR_ERR_INVALID and _err(ha, r.resolve_denoised) == HR_ERR_INVALID
    r.render(1, 5)
    r.denoise()
    r.upload_scene(sc)
    assert _err(ha, r.read_denoised) == HR_ERR_INVALID and _err(ha, r.read_guides) == HR_ERR_INVALID
    r.denoise()
    r.set_region(3, 3, 40, 20)
    assert _err(ha, r.read_denoised) == HR_ERR_INVALID
    r.set_resolution(W, H)                                       # the options stay on, the planes start over
    assert _err(ha, r.read_denoised) == HR_ERR_INVALID
    # per-pixel counts: the pixel's own count is its n; a pixel below 2, or a count above the moments', is refused
    r.set_option("sample_counts", 1)
    r.render(1, 5)
    r.denoise()
    d = r.read_denoised()
    low = cnt.copy()
    low[7, 9] = 1
    r.write_sample_counts(low)
    assert _err(ha, r.denoise) == HR_ERR_INVALID
    high = cnt.copy()
    high[7, 9] = 5
    r.write_sample_counts(high)
    assert _err(ha, r.denoise) == HR_ERR_INVALID
    r.write_sample_counts(cnt)
    r.denoise()
    assert same(r.read_denoised(), d)
    r.write_sample_counts(cnt)
    assert _err(ha, r.read_denoised) == HR_ERR_INVALID
    r.close()
    # switching moments off invalidates too.  (hr_render_debug invalidates as well, but that cannot be observed: it refuses while moments is on, and
    # switching moments off has already invalidated D.)
    r = _make(ha, sc)
    r.render(1, 5)
    r.denoise()
    r.set_option("moments", 0)
    assert _err(ha, r.read_denoised) == HR_ERR_INVALID
    r.close()


# ---------------------------------------------------------------------------------------------------------------- quality

def _rel_sq_error(x, t):
    x, t = x.astype(np.float64), t.astype(np.float64)
    return float(np.mean((x - t) ** 2 / (t ** 2 + 0.01 ** 2)))


@pytest.mark.parametrize("scene", SCENES)
def test_default_parameters_lower_the_error_of_a_short_render(ha, scenes, scene):
    """Truth: 2,048 samplings of the 96x54 frame.  The relative squared error mean((x - t)^2 / (t^2 + 0.01^2)) of the denoised image at 16 samplings
    is lower than the raw mean's.  Only "lower" is asserted; the ratios printed here (16 and 64 samplings) are the ones in DESIGN.md §4.9."""
    r = _make(ha, scenes(scene)[0])
    r.render(1, 2049)
    truth = r.read_accumulator() / np.float32(2048 * 4)
    ratios = {}
    for s in (16, 64):
        r.clear()
        r.render(1, s + 1)
        raw = r.read_accumulator() / np.float32(s * 4)
        r.denoise()
        e_raw, e_den = _rel_sq_error(raw, truth), _rel_sq_error(r.read_denoised(), truth)
        ratios[s] = e_den / e_raw
        print("%s S=%d: raw %.5g denoised %.5g ratio %.4f" % (scene, s, e_raw, e_den, ratios[s]))
    r.close()
    assert ratios[16] < 1.0


# ---------------------------------------------------------------------------------------------------------------- the CLI

CLI_ARGS = ["--assets", ASSETS, "--scene", "spheres", "-w", "32", "-h", "16"]


def test_cli_denoise_guide_images_and_resume(tmp_path):
    """--denoise end to end, and its resume rule: the filter's mean is accumulator / (4 n) with n the samplings behind the moments, so a
    checkpoint whose moments do not cover every sampling of its accumulator is refused (as --adaptive refuses it), not resolved too bright."""
    r = run_cli(CLI_ARGS + ["-s", "4", "--denoise", "--denoise-levels", "2", "--guide-image", "g", "--checkpoint", "with.ckpt"], tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout
    for name in ("result.png", "g_albedo.png", "g_normal.png", "g_depth.png", "with.ckpt"):
        assert (tmp_path / name).stat().st_size > 0, name
    assert "is not denoised" not in r.stdout
    # a checkpoint written without moments: {"HRA2", w, h, samplings, FNV-1a of the scene name} + the accumulator
    (tmp_path / "plain.ckpt").write_bytes(ckpt.pack(ckpt.new(32, 16, 3, "spheres", np.ones((16, 32, 3), np.float32))))
    r = run_cli(CLI_ARGS + ["-s", "6", "--denoise", "--resume", "plain.ckpt"], tmp_path, timeout=120)
    assert r.returncode == 1 and "--denoise" in r.stdout and "moments" in r.stdout, r.stdout
    r = run_cli(CLI_ARGS + ["-s", "6", "--resume", "plain.ckpt"], tmp_path, timeout=120)                   # without --denoise the file is fine
    assert r.returncode == 0, r.stdout
    r = run_cli(CLI_ARGS + ["-s", "6", "--denoise", "--resume", "with.ckpt"], tmp_path, timeout=120)         # moments that cover its 4 samplings: goes on to 6
    assert r.returncode == 0 and "resumed at 4x4 sampled" in r.stdout and "is not denoised" not in r.stdout, r.stdout
