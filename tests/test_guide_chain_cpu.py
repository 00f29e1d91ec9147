"""Guide planes that follow mirrors and glass to the first rough hit (option "guide_bounces") on the CPU tier: the host form of
csrc/pt_core.h guide_chain_link (tests/guide_chain_harness.cpp, built here with g++) against guide_primary, against the same chain in f64 over the
oracle, and each rule of the definition on a tiny hand-built scene; the variant rows and the CLI's refusals, without a device."""
import os

import numpy as np
import pytest

import guide_chain as gc
from cli import run_cli
from gpu_helpers import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 48, 27
SCENES = ["cornell_mini", "rtcamp6_v3_1"]
# Against the f64 oracle chain, K = 4, 48x27, per sub-sample: 3 x the worst observed on the two scenes (DESIGN §6.5's rule for a measured gate).
# Observed: albedo 1.38e-4 absolute (rtcamp6_v3_1: the fp32 texture fetch and its gamma), normal 8.6e-6 absolute (cornell_mini), path length
# 3.3e-6 relative (rtcamp6_v3_1, three hits).
TOL_ALBEDO, TOL_NORMAL, TOL_LENGTH = 4.2e-4, 2.6e-5, 1.0e-5


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return gc.build_harness(tmp_path_factory.mktemp("guide_chain"))


@pytest.fixture(scope="module")
def host_chain(harness, scenes):
    """name -> HostChain of a named scene"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = gc.HostChain(harness, scenes(name)[0].desc_ptr)
        return cache[name]
    return get


@pytest.mark.parametrize("scene", SCENES)
def test_zero_bounces_is_guide_primary(host_chain, scene):
    hc = host_chain(scene)
    sub, info, pix = hc.chain(W, H, 0)
    sub0, pix0 = hc.primary(W, H)
    assert np.array_equal(bits(sub), bits(sub0)) and np.array_equal(bits(pix), bits(pix0))
    assert (sub[..., 7] == 1.0).sum() > 1000 and set(np.unique(info[..., 0])) == {0, 1}
    assert not np.array_equal(bits(hc.chain(W, H, 4)[2]), bits(pix))           # both scenes have mirrors or glass in view: the chain changes the planes


@pytest.mark.parametrize("scene", SCENES)
def test_against_the_f64_oracle_chain(host_chain, scenes, orc, scene):
    """K = 4, per sub-sample.  A sub-sample is divergent when its chain has another number of hits than the oracle's or ends on another element;
    at most 1 % may be (a condition — measured: none of the 5,184 on either scene).  For the others: albedo within 4.2e-4 and normal within 2.6e-5
    absolute, path length within 1.0e-5 relative, coverage equal — 3 x the worst observed (albedo 1.38e-4, normal 8.6e-6, length 3.3e-6)."""
    sc, osc = scenes(scene)
    sub, info, _ = host_chain(scene).chain(W, H, 4)
    val, oinfo, _ = gc.oracle_chain(orc, osc, sc.desc, W, H, 4)
    divergent = (info != oinfo).any(-1)
    print("%s: %d of %d sub-samples divergent; chain hits %s" % (scene, divergent.sum(), divergent.size, np.bincount(oinfo[..., 0].ravel()).tolist()))
    assert divergent.mean() <= 0.01
    assert (oinfo[..., 0] >= 2).sum() > 50                                       # chains that bounced are there to be compared
    ok = ~divergent
    d = np.abs(sub.astype(np.float64) - val)[ok]
    hit = val[ok][:, 7] == 1.0
    e_alb, e_nrm = d[:, 0:3].max(), d[:, 3:6].max()
    e_len = (d[hit][:, 6] / val[ok][hit][:, 6]).max()
    print("%s: worst albedo %.3g (gate %.3g), normal %.3g (gate %.3g), path length %.3g relative (gate %.3g)" % (scene, e_alb, TOL_ALBEDO, e_nrm, TOL_NORMAL, e_len, TOL_LENGTH))
    assert e_alb <= TOL_ALBEDO and e_nrm <= TOL_NORMAL and e_len <= TOL_LENGTH
    assert (d[:, 7] == 0.0).all() and (sub[ok][~hit] == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------- the rules, one by one
# Camera at (0, 1, 6) looking down -z, 30 degrees, 16 x 9: the centre pixel's four rays are within 2.5 degrees of the axis (one is the axis).

FW, FH, CX, CY = 16, 9, 8, 4
BOX_COLOUR, MIRROR = (0.75, 0.5, 0.25), (0.5, 0.5, 0.5)
FRONT_MIRROR = dict(kind="cuboid", surface=1, albedo=MIRROR, min=(-0.5, 0.5, -1.0), max=(0.5, 1.5, -0.9))        # its +z face looks at the camera
BACK_BOX = dict(kind="cuboid", surface=0, albedo=BOX_COLOUR, min=(-50.0, -50.0, 8.0), max=(50.0, 50.0, 9.0))     # behind the camera, fills every reflection


def _chain(ha, harness, elements, bounces, **camera):
    sc = gc.tiny_scene(ha, elements, **camera)
    hc = gc.HostChain(harness, sc.desc_ptr)
    out = hc.chain(FW, FH, bounces)
    hc.close()
    return sc, out


def _axis_length(sc, *planes_z):
    """The path length of the centre pixel's sub-samples along a chain that runs between planes of constant z, in f64: every segment has the
    same |d_z| (a mirror at constant z flips its sign), so the length is the z distance covered / |d_z|."""
    _, dirs = gc.pinhole_rays(sc.desc, FW, FH)
    dz = np.abs(dirs[CY, CX, :, 2])
    z = [6.0] + list(planes_z)
    return sum(abs(b - a) for a, b in zip(z, z[1:])) / dz


def test_rule_a_planar_mirror_shows_the_box_behind_the_camera(ha, harness):
    sc, (sub, info, pix) = _chain(ha, harness, [FRONT_MIRROR, BACK_BOX], 4)
    s = sub[CY, CX]
    assert (info[CY, CX] == (2, 1)).all()                                        # two hits, the last on the box
    assert (s[:, 0:3] == np.float32(MIRROR) * np.float32(BOX_COLOUR)).all()      # dyadic: the product is exact
    assert (s[:, 3:6] == np.float32([0.0, 0.0, -1.0])).all() and (s[:, 7] == 1.0).all()
    want = _axis_length(sc, -0.9, 8.0)                                           # (the bounce starts 1e-4 off the mirror: 6e-6 of the length)
    assert np.allclose(s[:, 6], want, rtol=2e-5, atol=0)
    assert (pix[CY, CX, 0:3] == np.float32(MIRROR) * np.float32(BOX_COLOUR)).all() and pix[CY, CX, 7] == 1.0
    _, (sub0, info0, _) = _chain(ha, harness, [FRONT_MIRROR, BACK_BOX], 0)
    assert (sub0[CY, CX][:, 0:3] == np.float32(MIRROR)).all() and (sub0[CY, CX][:, 3:6] == np.float32([0.0, 0.0, 1.0])).all() and (info0[CY, CX] == (1, 0)).all()


def test_rule_a_glass_sphere_in_front_of_a_wall_is_a_chain_of_two_hits(ha, harness):
    """The sphere query keeps the near root only, as the reference's (scene.rs): the refracted ray, inside the sphere, does not meet it again and
    goes on to the wall."""
    glass = dict(kind="sphere", surface=2, albedo=(0.5, 1.0, 1.0), param=1.5, center=(0.0, 1.0, 0.0), radius=1.0)
    wall = dict(kind="cuboid", surface=0, albedo=BOX_COLOUR, min=(-50.0, -50.0, -9.0), max=(50.0, 50.0, -8.0))
    for bounces, hits, elem, albedo in ((0, 1, 0, (0.5, 1.0, 1.0)), (1, 2, 1, (0.375, 0.5, 0.25)), (8, 2, 1, (0.375, 0.5, 0.25))):
        _, (sub, info, _) = _chain(ha, harness, [glass, wall], bounces)
        assert (info[CY, CX] == (hits, elem)).all(), bounces
        assert (sub[CY, CX][:, 0:3] == np.float32(albedo)).all(), bounces          # the albedo of every hit, the sampled-bounce scalar is not in it
    s = sub[CY, CX]                                                               # to the sphere and on to the wall: 5 + 9 along the axis, a little more beside it
    assert (s[:, 3:6] == np.float32([0.0, 0.0, 1.0])).all() and ((s[:, 6] > 13.99) & (s[:, 6] < 14.2)).all()


def test_rule_beyond_the_critical_angle_glass_reflects(ha, harness):
    """The camera sits INSIDE a glass slab (y in 0 .. 2, index 1.5: critical angle 41.8 degrees).  Looking at its top face at 80 degrees from the
    normal the ray is totally reflected and lands on the slab's bottom face; looking straight up it leaves through the top and reaches the lid."""
    slab = dict(kind="cuboid", surface=2, albedo=(1.0, 1.0, 1.0), param=1.5, min=(-20.0, 0.0, -20.0), max=(20.0, 2.0, 20.0))
    lid = dict(kind="cuboid", surface=0, albedo=BOX_COLOUR, min=(-50.0, 3.0, -50.0), max=(50.0, 3.5, 50.0))
    _, (sub, info, _) = _chain(ha, harness, [slab, lid], 1, target=(0.0, 2.0, 0.0))
    assert (info[CY, CX] == (2, 0)).all()                                        # the second hit is the slab again,
    assert (sub[CY, CX][:, 3:6] == np.float32([0.0, -1.0, 0.0])).all()           # its bottom face: the reflection.  (Transmitted, the ray meets the lid.)
    assert (sub[CY, CX][:, 0:3] == 1.0).all()
    _, (sub, info, _) = _chain(ha, harness, [slab, lid], 1, target=(0.0, 2.0, 5.9))
    assert (info[CY, CX] == (2, 1)).all() and (sub[CY, CX][:, 0:3] == np.float32(BOX_COLOUR)).all()


def test_rule_a_mirror_that_shows_sky_ends_on_the_mirror_and_a_primary_miss_is_zeros(ha, harness):
    sc, (sub, info, pix) = _chain(ha, harness, [FRONT_MIRROR], 4)
    s = sub[CY, CX]
    assert (info[CY, CX] == (1, 0)).all() and (s[:, 7] == 1.0).all()
    assert (s[:, 0:3] == np.float32(MIRROR)).all() and (s[:, 3:6] == np.float32([0.0, 0.0, 1.0])).all()
    assert np.allclose(s[:, 6], _axis_length(sc, -0.9), rtol=2e-6, atol=0)
    assert pix[CY, CX, 7] == 1.0
    assert (info[0, 0] == (0, -1)).all() and (sub[0, 0] == 0.0).all() and (pix[0, 0] == 0.0).all()     # the corner pixel sees sky: eight zeros
    assert (pix[..., 7] == 0.0).sum() > 50


def test_rule_one_bounce_between_two_mirrors_ends_on_the_second(ha, harness):
    back = dict(BACK_BOX, surface=1, albedo=(0.25, 0.5, 1.0))
    front = dict(FRONT_MIRROR, min=(-2.0, -1.0, -1.0), max=(2.0, 3.0, -0.9))            # wide enough for the rays that come back after 25 units
    for bounces, hits, elem, albedo, nz in ((0, 1, 0, MIRROR, 1.0), (1, 2, 1, (0.125, 0.25, 0.5), -1.0), (2, 3, 0, (0.0625, 0.125, 0.25), 1.0)):
        _, (sub, info, _) = _chain(ha, harness, [front, back], bounces)
        assert (info[CY, CX] == (hits, elem)).all(), bounces
        assert (sub[CY, CX][:, 0:3] == np.float32(albedo)).all() and (sub[CY, CX][:, 5] == nz).all(), bounces


# ---------------------------------------------------------------------------------------------------------------- rows, option, CLI

def test_variant_table_has_the_chain_rows_and_keeps_the_old_ones():
    kv = open(os.path.join(ROOT, "hanamaru-renderer_amd", "csrc", "kernel_variants.h")).read()
    for row in ("HR_VARIANT(guide_chain_kernel, true)", "HR_VARIANT(guide_chain_kernel, false)", "HR_VARIANT(guide_render_kernel, true)",
                "HR_VARIANT(guide_render_kernel, false)", "select_guide_chain_kernel(bool qn)", "select_guide_render_kernel(bool qn)"):
        assert row in kv, row
    api = open(os.path.join(ROOT, "hanamaru-renderer_amd", "csrc", "hr_api.hip")).read()
    assert '"guide_bounces"' in api and "select_guide_chain_kernel(" in api
    assert '"guide_bounces"' in open(os.path.join(ROOT, "include", "hanamaru_hip.h")).read()


def test_cli_help_lists_guide_bounces(tmp_path):
    r = run_cli(["--help"], tmp_path)
    assert r.returncode == 0 and "--guide-bounces K" in r.stdout


@pytest.mark.parametrize("args,word", [(["--denoise", "--guide-bounces", "9"], "--guide-bounces must be"), (["--guide-image", "g", "--guide-bounces", "-1"], "--guide-bounces must be"),
                                       (["--denoise", "--guide-bounces", "two"], "--guide-bounces must be"), (["--guide-bounces", "2"], "--guide-bounces needs")])
def test_cli_refuses_guide_bounces_before_any_device(tmp_path, args, word):
    r = run_cli(["-w", "64", "-h", "48", "-s", "8"] + args, tmp_path)
    assert r.returncode == 1, r.stdout
    assert word in r.stdout
    assert not (tmp_path / "result.txt").exists()
