"""Shared by the lens-sampled guide plane tests (hr_render_guides_lens) and tools/guide_lens_quality.py: the g++-built host form
(tests/guide_lens_harness.cpp over csrc/pt_core.h guide_lens_point / guide_lens_ray / guide_chain_link), camera.rs:83-96 in f64 numpy, the same
chain per lens ray in f64 over the oracle, and the hand-built wide-aperture scene.  Not a test module."""
import ctypes as C
import os
import subprocess

import numpy as np

import guide_chain as gc

ROOT = gc.ROOT
CSRC = gc.CSRC
SQUARE, CIRCLE = 0, 1


def build_harness(directory):
    """As guide_chain.build_harness: -mfma for the fmaf spellings of pt_core.h, -ffp-contract=off so that nothing else is fused."""
    so = os.path.join(str(directory), "libguide_lens_harness.so")
    subprocess.run(["g++", "-O2", "-mfma", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "guide_lens_harness.cpp"), os.path.join(CSRC, "flatten.cpp"), os.path.join(CSRC, "bvh_build.cpp"), "-lpthread"],
                   check=True)
    lib = C.CDLL(so)
    u32 = C.c_uint32
    lib.gl_scene_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.gl_scene_destroy.argtypes = [C.c_void_p]
    lib.gl_point.argtypes = [C.c_int, u32, u32, C.c_void_p]
    lib.gl_rays.argtypes = [C.c_void_p, u32, u32, u32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gl_pinhole_rays.argtypes = [C.c_void_p, u32, u32, C.c_void_p, C.c_void_p]
    lib.gl_lens_window.argtypes = [C.c_void_p, u32, u32, u32, u32, u32, u32, u32, u32, u32, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def harness_points(lib, shape, count):
    """guide_lens_point through the harness: (count, 2) float32"""
    uv = np.zeros((count, 2), np.float32)
    for i in range(count):
        lib.gl_point(shape, count, i, uv[i].ctypes.data)
    return uv


class HostLens:
    """The host form over one scene (an hr_scene_desc pointer)."""

    def __init__(self, lib, desc_ptr):
        self.lib = lib
        h = C.c_void_p()
        rc = lib.gl_scene_create(C.cast(desc_ptr, C.c_void_p), C.byref(h))
        if rc != 0:
            raise RuntimeError("gl_scene_create failed: %d" % rc)
        self._h = h

    def close(self):
        if self._h:
            self.lib.gl_scene_destroy(self._h)
            self._h = None

    def rays(self, w, h, uv):
        """guide_lens_ray through the lens points uv [n, 2]: (origins, directions), each [h, w, 4, n, 3] float32"""
        uv = np.ascontiguousarray(uv, np.float32)
        org = np.zeros((h, w, 4, len(uv), 3), np.float32)
        d = np.zeros_like(org)
        self.lib.gl_rays(self._h, w, h, len(uv), uv.ctypes.data, org.ctypes.data, d.ctypes.data)
        return org, d

    def pinhole_rays(self, w, h):
        """debug_camera_ray: (origins, directions), each [h, w, 4, 3] float32"""
        org = np.zeros((h, w, 4, 3), np.float32)
        d = np.zeros_like(org)
        self.lib.gl_pinhole_rays(self._h, w, h, org.ctypes.data, d.ctypes.data)
        return org, d

    def lens(self, w, h, bounces, count, window=None, per_ray=True, step=1):
        """The planes of hr_render_guides_lens(count) with guide_bounces = bounces, of the frame or of its window (x0, y0, ww, wh):
        (per ray [wh, ww, 4, count, 8] float32, info [wh, ww, 4, count, 2] int32 {hits of the chain, element of the last hit or -1}, planes
        [wh, ww, 8]); per_ray False: (None, None, planes).  count 1: the pinhole ray, hr_render_guides' planes.  step > 1: the window's ww x wh
        samples are the frame pixels (x0 + i step, y0 + j step)."""
        x0, y0, ww, wh = window or (0, 0, w, h)
        ray = np.zeros((wh, ww, 4, count, 8), np.float32) if per_ray else None
        info = np.zeros((wh, ww, 4, count, 2), np.int32) if per_ray else None
        pix = np.zeros((wh, ww, 8), np.float32)
        self.lib.gl_lens_window(self._h, w, h, x0, y0, ww, wh, step, bounces, count, ray.ctypes.data if per_ray else None, info.ctypes.data if per_ray else None, pix.ctypes.data)
        return ray, info, pix


def planes_of(ray):
    """The stated sum of per-ray values [.., 4, L, 8] in fp32: per sub-sample over l = 0 .. L - 1 in order, (s0 + s1) + (s2 + s3), x 0.25 / L."""
    ray = ray.astype(np.float32)
    count = ray.shape[-2]
    sub = np.zeros(ray.shape[:-2] + (8,), np.float32)
    for l in range(count):
        sub = sub + ray[..., l, :]
    return ((sub[..., 0, :] + sub[..., 1, :]) + (sub[..., 2, :] + sub[..., 3, :])) * np.float32(0.25 / count)


def lens_rays(desc, w, h, uv, window=None):
    """camera.rs:83-96 in f64 with the lens sample replaced by the points uv [n, 2]: (origins [n, 3], directions [wh, ww, 4, n, 3]) of the window
    (x0, y0, ww, wh) of the w x h frame; the normalised coordinates are guide_chain.pinhole_rays'."""
    cam = desc.camera
    x0, y0, ww, wh = window or (0, 0, w, h)
    y, x, sub = np.meshgrid(np.arange(y0, y0 + wh), np.arange(x0, x0 + ww), np.arange(4), indexing="ij")
    m = float(min(w, h))
    ncx = ((x + (sub & 1) * 0.5 - 0.5) * 2.0 - w) / m
    ncy = (((h - y) + (sub >> 1) * 0.5 - 0.5) * 2.0 - h) / m
    v = gc._v
    through = ncx[..., None] * v(cam.plane_half_right) + ncy[..., None] * v(cam.plane_half_up) + cam.focus_distance * v(cam.forward)
    luv = np.asarray(uv, np.float64) * cam.lens_radius
    lens_pos = luv[:, :1] * v(cam.right) + luv[:, 1:] * v(cam.up)
    d = through[..., None, :] - lens_pos
    return v(cam.eye) + lens_pos, d / np.sqrt((d * d).sum(-1, keepdims=True))


def oracle_lens(orc, osc, desc, w, h, bounces, uv, window=None):
    """The definition in f64, per ray: guide_chain.oracle_chain's loop along lens_rays.  (values [wh, ww, 4, n, 8] float64, info [wh, ww, 4, n, 2]
    as HostLens.lens).  The first hits of all rays go through intersect_material_n in one call; only chains that bounce are walked one by one."""
    org, dirs = lens_rays(desc, w, h, uv, window)
    shape = dirs.shape[:-1]
    n = int(np.prod(shape))
    rays = np.concatenate([np.broadcast_to(org, dirs.shape).reshape(n, 3), dirs.reshape(n, 3)], axis=1)
    rec, elem = osc.intersect_material_n(rays)
    val = np.zeros((n, 8))
    info = np.zeros((n, 2), np.int32)
    info[:, 1] = -1
    hit = rec[:, 0] != 0
    val[hit, 0:3], val[hit, 3:6], val[hit, 6], val[hit, 7] = rec[hit, 12:15], rec[hit, 5:8], rec[hit, 1], 1.0
    info[hit, 0], info[hit, 1] = 1, elem[hit]
    if bounces > 0:
        for i in np.nonzero(hit & np.isin(rec[:, 10], (1.0, 2.0)))[0]:
            o, d = rays[i, 0:3], rays[i, 3:6]
            a, z = np.ones(3), 0.0
            info[i, 0] = 0
            for j in range(bounces + 1):
                it = osc.intersect_material(o, d)
                if not it["hit"]:
                    break
                z += it["distance"]
                a = a * it["albedo"]
                val[i] = np.concatenate([a, it["normal"], [z, 1.0]])
                info[i, 0] += 1
                info[i, 1] = it["element"]
                if j == bounces or it["surface"] not in (1, 2):
                    break
                _, o, d, _ = orc.material_sample(it["surface"], it["param"], it["roughness"], 1.0, 0.0, it["position"], -d, it["normal"])
    return val.reshape(shape + (8,)), info.reshape(shape + (2,))


WIDE_ELEMENTS = [dict(kind="cuboid", surface=0, albedo=(0.6, 0.6, 0.6), min=(-20.0, -1.0, -12.0), max=(20.0, 0.0, 8.0)),
                 dict(kind="cuboid", surface=0, albedo=(0.75, 0.5, 0.25), min=(-20.0, 0.0, -5.0), max=(20.0, 12.0, -4.0)),
                 dict(kind="cuboid", surface=0, albedo=(0.25, 0.75, 0.5), min=(-0.5, 0.0, 2.8), max=(-0.1, 3.0, 3.2)),
                 dict(kind="sphere", surface=3, param=0.5, albedo=(0.5, 0.25, 1.0), center=(0.6, 0.5, 3.0), radius=0.5),
                 dict(kind="sphere", surface=0, albedo=(0.0, 0.0, 0.0), emission=(6.0, 6.0, 6.0), center=(0.0, 9.0, 3.0), radius=2.0)]


def set_camera(ha, sc, eye=(0.0, 1.0, 6.0), target=(0.0, 1.0, 0.0), fov=30.0, lens_shape=CIRCLE, aperture=0.6, focus=10.0):
    """hh_camera_new into the scene holder's descriptor"""
    ha.host_lib().hh_camera_new(ha.Vec3(*eye), ha.Vec3(*target), ha.Vec3(0.0, 1.0, 0.0), float(fov), int(lens_shape), float(aperture), float(focus), C.byref(sc.desc.camera))
    return sc


def tiny_scene(ha, elements, **camera):
    """guide_chain.tiny_scene with the elements' emission (default none) and the camera reset by hh_camera_new (set_camera's defaults: the wide
    aperture; aperture=0.0 for a pinhole)."""
    sc = gc.tiny_scene(ha, elements)
    el = sc.keep[1]
    for e, spec in zip(el, elements):
        if "emission" in spec:
            e.material.emission.color = ha.Vec3(*spec["emission"])
    return set_camera(ha, sc, **camera)


def wide_scene(ha):
    """The hand-built wide-aperture scene: floor, wall, a thin pillar and a GGX sphere in front of the focus plane (focus 10, lens radius 0.3),
    lit by an emissive sphere overhead."""
    return tiny_scene(ha, WIDE_ELEMENTS)


def copy_scene(ha, name, aperture=None, untextured=False):
    """A named scene's descriptor with its own element array: untextured gives every element a distinct dyadic albedo (sixteenths, as
    test_guide_chain_gpu.py's untextured cornell_mini); aperture sets the camera's lens radius to aperture / 2 and leaves everything else."""
    base = ha.Scene(name)
    n = base.desc.num_elements
    el = (ha.Element * n)()
    C.memmove(el, base.desc.elements, C.sizeof(ha.Element) * n)
    if untextured:
        for i in range(n):
            el[i].material.albedo.image = -1
            el[i].material.albedo.color = ha.Vec3((1 + (5 * i) % 15) / 16.0, (1 + (7 * i + 3) % 15) / 16.0, (1 + (11 * i + 6) % 15) / 16.0)
    d = ha.SceneDesc()
    C.memmove(C.byref(d), base.desc_ptr, C.sizeof(d))
    d.elements = C.cast(el, C.POINTER(ha.Element))
    if aperture is not None:
        d.camera.lens_radius = 0.5 * aperture

    class Holder:
        pass
    s = Holder()
    s.desc, s.desc_ptr, s.keep = d, C.pointer(d), [base, el, d]
    return s


def differ_mask(lens_planes, pinhole_planes, threshold=0.02):
    """pixels where the lens and pinhole planes 0 .. 5 (albedo, normal) differ by more than the threshold"""
    return np.abs(lens_planes[..., 0:6].astype(np.float64) - pinhole_planes[..., 0:6]).max(-1) > threshold
