"""Shared by the guide-chain tests (option "guide_bounces") and tools/guide_quality.py: the g++-built host form
(tests/guide_chain_harness.cpp over csrc/pt_core.h guide_chain_link), the same chain in f64 over the oracle's intersect_material and
material_sample(.., r0 = 1, r1 = 0, ..), and tiny hand-built scenes.  Not a test module."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hanamaru-renderer_amd", "csrc")


def build_harness(directory):
    """-mfma: pt_core.h spells its dot / cross products with fmaf (as tests/emu); -ffp-contract=off: nothing else is fused."""
    so = os.path.join(str(directory), "libguide_chain_harness.so")
    subprocess.run(["g++", "-O2", "-mfma", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "guide_chain_harness.cpp"), os.path.join(CSRC, "flatten.cpp"), os.path.join(CSRC, "bvh_build.cpp"), "-lpthread"],
                   check=True)
    lib = C.CDLL(so)
    lib.gc_scene_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.gc_scene_destroy.argtypes = [C.c_void_p]
    lib.gc_chain.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gc_primary.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return lib


class HostChain:
    """The host form over one scene (an hr_scene_desc pointer)."""

    def __init__(self, lib, desc_ptr):
        self.lib = lib
        h = C.c_void_p()
        rc = lib.gc_scene_create(C.cast(desc_ptr, C.c_void_p), C.byref(h))
        if rc != 0:
            raise RuntimeError("gc_scene_create failed: %d" % rc)
        self._h = h

    def close(self):
        if self._h:
            self.lib.gc_scene_destroy(self._h)
            self._h = None

    def chain(self, w, h, bounces):
        """(per sub-sample [h, w, 4, 8] float32, info [h, w, 4, 2] int32 {hits of the chain, element of the last hit or -1}, planes [h, w, 8])"""
        sub = np.zeros((h, w, 4, 8), np.float32)
        info = np.zeros((h, w, 4, 2), np.int32)
        pix = np.zeros((h, w, 8), np.float32)
        self.lib.gc_chain(self._h, w, h, bounces, sub.ctypes.data, info.ctypes.data, pix.ctypes.data)
        return sub, info, pix

    def primary(self, w, h):
        """guide_primary: (per sub-sample [h, w, 4, 8], planes [h, w, 8])"""
        sub = np.zeros((h, w, 4, 8), np.float32)
        pix = np.zeros((h, w, 8), np.float32)
        self.lib.gc_primary(self._h, w, h, sub.ctypes.data, pix.ctypes.data)
        return sub, pix


def _v(v):
    return np.array([v.x, v.y, v.z], dtype=np.float64)


def pinhole_rays(desc, w, h):
    """camera.rs:98-107 in f64, the rays of the debug renderer: (eye [3], directions [h, w, 4, 3]); sub-sample = sx + 2 sy."""
    cam = desc.camera
    y, x, sub = np.meshgrid(np.arange(h), np.arange(w), np.arange(4), indexing="ij")
    m = float(min(w, h))
    ncx = ((x + (sub & 1) * 0.5 - 0.5) * 2.0 - w) / m
    ncy = (((h - y) + (sub >> 1) * 0.5 - 0.5) * 2.0 - h) / m
    d = ncx[..., None] * _v(cam.plane_half_right) + ncy[..., None] * _v(cam.plane_half_up) + cam.focus_distance * _v(cam.forward)
    return _v(cam.eye), d / np.sqrt((d * d).sum(-1, keepdims=True))


def oracle_chain(orc, osc, desc, w, h, bounces):
    """The definition in f64.  (values [h, w, 4, 8] float64, info [h, w, 4, 2] as HostChain.chain, first [h, w, 4, 2] int32 {surface type of the
    primary hit or -1, its element or -1})."""
    eye, dirs = pinhole_rays(desc, w, h)
    val = np.zeros((h, w, 4, 8))
    info = np.zeros((h, w, 4, 2), np.int32)
    first = np.full((h, w, 4, 2), -1, np.int32)
    info[..., 1] = -1
    for y in range(h):
        for x in range(w):
            for s in range(4):
                o, d = eye, dirs[y, x, s]
                a, z = np.ones(3), 0.0
                for j in range(bounces + 1):
                    it = osc.intersect_material(o, d)
                    if not it["hit"]:
                        break
                    if j == 0:
                        first[y, x, s] = (it["surface"], it["element"])
                    z += it["distance"]
                    a = a * it["albedo"]
                    val[y, x, s] = np.concatenate([a, it["normal"], [z, 1.0]])
                    info[y, x, s, 0] += 1
                    info[y, x, s, 1] = it["element"]
                    if j == bounces or it["surface"] not in (1, 2):
                        break
                    _, o, d, _ = orc.material_sample(it["surface"], it["param"], it["roughness"], 1.0, 0.0, it["position"], -d, it["normal"])
    return val, info, first


def planes_of(sub):
    """The planes of per-sub-sample values as the kernel sums them: (s0 + s1) + (s2 + s3), x 0.25."""
    s = sub.astype(np.float64)
    return ((s[..., 0, :] + s[..., 1, :]) + (s[..., 2, :] + s[..., 3, :])) * 0.25


def tiny_scene(ha, elements, eye=(0.0, 1.0, 6.0), target=(0.0, 1.0, 0.0), fov=30.0):
    """elements: dicts {kind: "cuboid" | "sphere", surface, albedo, param (default 1.5), and min / max or center / radius}; constant albedo, no
    emission, roughness 0.3.  Images and skybox are cornell_mini's (as tests/random_scenes.py); pinhole camera."""
    base = ha.Scene("cornell_mini")
    el = (ha.Element * len(elements))()
    for e, spec in zip(el, elements):
        m = e.material
        m.surface = int(spec["surface"])
        m.param = float(spec.get("param", 1.5))
        m.albedo.color, m.albedo.image = ha.Vec3(*spec["albedo"]), -1
        m.emission.color, m.emission.image = ha.Vec3(0.0, 0.0, 0.0), -1
        m.roughness.color, m.roughness.image = ha.Vec3(0.3, 0.3, 0.3), -1
        if spec["kind"] == "sphere":
            e.kind, e.center, e.radius = ha.SPHERE, ha.Vec3(*spec["center"]), float(spec["radius"])
        else:
            e.kind, e.aabb_min, e.aabb_max = ha.CUBOID, ha.Vec3(*spec["min"]), ha.Vec3(*spec["max"])
    d = ha.SceneDesc()
    C.memmove(C.byref(d), base.desc_ptr, C.sizeof(d))
    d.elements = C.cast(el, C.POINTER(ha.Element))
    d.num_elements = len(elements)
    ha.host_lib().hh_camera_new(ha.Vec3(*eye), ha.Vec3(*target), ha.Vec3(0.0, 1.0, 0.0), float(fov), 0, 0.0, 5.0, C.byref(d.camera))

    class Holder:
        pass
    s = Holder()
    s.desc = d
    s.desc_ptr = C.pointer(d)
    s.keep = [base, el, d]
    s.num_elements = len(elements)
    return s


def rel_sq_error(x, t):
    x, t = x.astype(np.float64), t.astype(np.float64)
    return float(np.mean((x - t) ** 2 / (t ** 2 + 0.01 ** 2)))
