"""Corner scenes (tests/corner_scenes.py) on the MI355X: hr_debug_path_log against the oracle's path log, path by path, with the accounting and
the limits of the CPU tier (tests/test_corners_cpu.py runs the same cases through the host emulation); the logged radiances are what hr_render
accumulates; and the albedo guide plane of the imaged cuboid against the oracle's material fetch."""
import ctypes as C

import numpy as np
import pytest

import corner_scenes as cs
from gpu_helpers import options

pytestmark = pytest.mark.gpu


def _log_and_render(gpu, s):
    """the path log of sampling 1, checked against one sampling rendered the normal way: 0 + ((s0 + s1) + (s2 + s3)) per pixel and channel, in
    fp32 (tests/test_gpu_parity.py _per_path_accounting (i))"""
    gpu.set_resolution(s.w, s.h)
    g = gpu.debug_path_log(1)
    gpu.clear()
    gpu.render(1, 2)
    acc = gpu.read_accumulator()
    rad = g[0]
    want = (rad[:, :, 0] + rad[:, :, 1]) + (rad[:, :, 2] + rad[:, :, 3])
    assert np.array_equal(acc, want.astype(np.float32)), "the path log's radiances are not what hr_render accumulates"
    return g


@pytest.mark.parametrize("precise", [0, 1])
@pytest.mark.parametrize("name", sorted(cs.CASES))
def test_corner_scene_path_by_path(gpu, ha, orc, name, precise):
    s, ref = cs.get(ha, orc, name)
    gpu.upload_scene(s)
    with options(gpu, {"precise_shading": precise}):
        g = _log_and_render(gpu, s)
    cs.check(name, g, ref, "device, precise_shading %d" % precise)
    if name.startswith("sky_nonsquare"):
        assert (g[1] == 1).all() and ((g[2][..., 0] & 7) == 1).all()          # one ray, one sky lookup


@pytest.mark.parametrize("option,value,default", [("quant_nodes", 0, 1), ("bvh_builder", 2, -1)])
@pytest.mark.parametrize("name", ["cuboid_edges-ggx-ppp", "cuboid_edges-diffuse-nnn", "sphere_poles-north", "sphere_poles-seam"])
def test_corner_scene_on_the_other_trees(gpu, ha, orc, name, option, value, default):
    """the 32-byte nodes and the device-built PLOC tree: the same limits"""
    s, ref = cs.get(ha, orc, name)
    with options(gpu, {option: value, "precise_shading": 0}):
        gpu.upload_scene(s)
        g = _log_and_render(gpu, s)
    cs.check(name, g, ref, "device, %s %d" % (option, value))


@pytest.mark.parametrize("precise", [0, 1])
def test_camera_inside_a_glass_sphere_sees_through_it(gpu, ha, orc, precise):
    """scene.rs:58-64: the near root only — from inside a sphere every primary ray misses it and ends in the sky (the mixed-size faces)"""
    s = cs.inside_glass_sphere(ha)
    ref = orc.OracleScene(s.desc_ptr).path_log(s.w, s.h, 1)
    assert ((ref[2][..., 0] & 7) == 1).all() and (ref[1] == 1).all() and (ref[2][..., 9] == 0).all()
    gpu.upload_scene(s)
    with options(gpu, {"precise_shading": precise}):
        g = _log_and_render(gpu, s)
    cs.check_whole_frame(g, ref)


@pytest.mark.parametrize("precise", [0, 1])
@pytest.mark.parametrize("south", [False, True])
def test_the_ray_that_hits_a_pole_exactly(gpu, ha, orc, south, precise):
    """tests/test_corners_cpu.py test_the_ray_that_hits_a_pole_exactly, on the device: 0 x rsq(0) is a NaN that the clamp before acos turns
    into u = 0 or 1 — a finite path where the reference ends with nothing, and 15 paths that are the oracle's."""
    s = cs.sphere_pole_exact(ha, south)
    ref = orc.OracleScene(s.desc_ptr).path_log(2, 2, 1)
    gpu.upload_scene(s)
    with options(gpu, {"precise_shading": precise}):
        g = _log_and_render(gpu, s)
    cs.check_pole_frame(g, ref, (1, 1, 3))


def _sub_sample_rays(r, desc, w, h):
    """The rays of sampling 1's paths: ray_with_dof (camera.rs:83-96) in f64 from the camera of the scene description, the sub-sample's
    normalized coordinate (renderer.rs:52-53) and the two lens draws of hr_debug_path_draws — which a pinhole's lens radius of 0 multiplies away."""
    draws = np.empty((h, w, 4, 20), dtype=np.float32)
    r._check(r.L.hr_debug_path_draws(r._h, 1, C.c_void_p(draws.ctypes.data)))
    cam = desc.camera
    v = lambda a: np.array([a.x, a.y, a.z], dtype=np.float64)
    y, x, sub = np.meshgrid(np.arange(h), np.arange(w), np.arange(4), indexing="ij")
    m = float(min(w, h))
    ncx = ((x + (sub & 1) * 0.5 - 0.5) * 2.0 - w) / m
    ncy = (((h - y) + (sub >> 1) * 0.5 - 0.5) * 2.0 - h) / m
    lens = draws[..., 0:2].astype(np.float64) * cam.lens_radius
    lens_pos = lens[..., 0:1] * v(cam.right) + lens[..., 1:2] * v(cam.up)
    d = ncx[..., None] * v(cam.plane_half_right) + ncy[..., None] * v(cam.plane_half_up) + cam.focus_distance * v(cam.forward) - lens_pos
    return v(cam.eye) + lens_pos, d / np.sqrt((d * d).sum(-1, keepdims=True))


@pytest.mark.parametrize("view", sorted(cs.CUBOID_VIEWS))
def test_albedo_guide_plane_of_the_imaged_cuboid(ha, orc, view):
    """hr_render_guides' albedo plane on cuboid_edges: where all four sub-samples hit, the mean of the oracle's intersect_material albedo over
    the four rays, to 1e-3 — the 7 x 3 albedo lookup on all six faces (u, v from 0 to 1, the flipped v of the Y faces) with no bounce after it."""
    s = cs.cuboid_edges(ha, view)
    o = orc.OracleScene(s.desc_ptr)
    with ha.Renderer(0) as r:
        r.upload_scene(s)
        r.set_resolution(s.w, s.h)
        org, dirs = _sub_sample_rays(r, s.desc, s.w, s.h)
        r.render_guides()
        g = r.read_guides()
    full = np.argwhere(g[..., 7] == 1.0)
    assert len(full) > 400                                   # the cuboid fills a fifth of the frame
    worst, normals = 0.0, set()
    for y, x in full:
        hits = [o.intersect_material(org[y, x, k], dirs[y, x, k]) for k in range(4)]
        assert all(hh["hit"] for hh in hits), (y, x)
        normals.update(tuple(hh["normal"]) for hh in hits)
        want = np.mean([hh["albedo"] for hh in hits], axis=0)
        worst = max(worst, float(np.abs(g[y, x, 0:3] - want).max()))
    print("cuboid_edges %s: albedo plane against the oracle on %d pixels, worst %.3g" % (view, len(full), worst))
    assert len(normals) == 3                                 # three faces in the view
    assert worst <= 1e-3
