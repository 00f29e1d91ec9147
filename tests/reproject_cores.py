"""Shared by the temporal-reuse tests: tests/reproject_harness.cpp (csrc/reproject_core.h for the host) and tests/motion_harness.cpp
(the per-lane functions of motion_kernel with the scalar walk), each built once per process with g++ -ffp-contract=off; the random planes of the
gather tests; the hand-built scene of the motion tests and its f64 numpy reference (ray / box / sphere algebra).  Not a test module.

No GPU in this module."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from reproject_numpy import numpy_motion, numpy_project

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hanamaru-renderer_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-I", os.path.join(ROOT, "include"), "-I", CSRC]
_P, _U32, _U64, _D = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double


@functools.lru_cache(maxsize=None)
def _directory():
    d = tempfile.mkdtemp(prefix="reproject_harness_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def core_lib():
    so = os.path.join(_directory(), "libreproject_harness.so")
    subprocess.run(["g++"] + FLAGS + ["-o", so, os.path.join(ROOT, "tests", "reproject_harness.cpp")], check=True)
    lib = C.CDLL(so)
    lib.rp_project.argtypes = [_P, _P, _P, _U64, _P]
    lib.rp_motion.argtypes = [_P, _U32, _U32, _P, _U64, _P]
    lib.rp_pixels.argtypes = [_P, _P, _P, _P, _U32, _U32, _U32, _P, _P, _P]
    return lib


@functools.lru_cache(maxsize=None)
def motion_lib():
    """-mfma: pt_core.h spells its dot / cross products with fmaf (as tests/guide_chain.py); -ffp-contract=off: nothing else is fused."""
    so = os.path.join(_directory(), "libmotion_harness.so")
    subprocess.run(["g++"] + FLAGS + ["-mfma", "-o", so, os.path.join(ROOT, "tests", "motion_harness.cpp"), os.path.join(CSRC, "flatten.cpp"), os.path.join(CSRC, "bvh_build.cpp"),
                                      "-lpthread"], check=True)
    lib = C.CDLL(so)
    lib.mh_scene_create.argtypes = [_P, C.POINTER(_P)]
    lib.mh_scene_destroy.argtypes = [_P]
    lib.mh_motion.argtypes = [_P, _P, _U32, _U32, _U32, _U32, _U32, _U32, _D, _D, _P, _P]
    return lib


# ---- reproject_core.h over arrays ----
def core_project(cam, x, at_infinity):
    x = np.ascontiguousarray(x, dtype=np.float32)
    inf = np.ascontiguousarray(at_infinity, dtype=np.uint8)
    out = np.zeros((x.shape[0], 6))
    core_lib().rp_project(np.ascontiguousarray(cam, dtype=np.float64).ctypes.data, x.ctypes.data, inf.ctypes.data, x.shape[0], out.ctypes.data)
    return out[:, 0] != 0.0, out[:, 1:4], out[:, 4], out[:, 5]


def core_motion(ncx, ncy, W, H, px, py, sub):
    nc = np.ascontiguousarray(np.stack([ncx, ncy], axis=-1), dtype=np.float64)
    pix = np.ascontiguousarray(np.stack([px, py, sub], axis=-1), dtype=np.uint32)
    out = np.zeros((nc.shape[0], 3))
    core_lib().rp_motion(nc.ctypes.data, W, H, pix.ctypes.data, nc.shape[0], out.ctypes.data)
    return out[:, 0] != 0.0, out[:, 1], out[:, 2]


def core_reproject(motion, acc, counts, mom, max_history):
    motion = np.ascontiguousarray(motion, dtype=np.float32)
    acc = np.ascontiguousarray(acc, dtype=np.float32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    h, w = counts.shape
    assert motion.shape == (h, w, 4, 3) and acc.shape == (h, w, 3)
    mom = None if mom is None else np.ascontiguousarray(mom, dtype=np.float64)
    oa, oc = np.full((h, w, 3), 7.0, np.float32), np.full((h, w), 7, np.uint32)
    om = None if mom is None else np.full((h, w, 6), 7.0)
    core_lib().rp_pixels(motion.ctypes.data, acc.ctypes.data, counts.ctypes.data, None if mom is None else mom.ctypes.data, w, h, int(max_history), oa.ctypes.data, oc.ctypes.data,
                         None if om is None else om.ctypes.data)
    return oa, oc, om


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def random_planes(w=37, h=23, seed=5):
    """The planes of the gather tests: counts 0 .. 40 with a fifth of them 0, radiance-like accumulators and moments, and a motion plane with whole and
    fractional motion, codes 1 to 3, NaN, +-inf and over-range motion, and motion that puts taps across every edge of the region."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 41, size=(h, w)).astype(np.uint32)
    counts[rng.random((h, w)) < 0.2] = 0
    x = rng.gamma(2.0, 0.5, size=(h, w, 3))
    acc = (x * counts[..., None]).astype(np.float32)
    mom = np.concatenate([x * counts[..., None], (x * x + 0.1) * counts[..., None]], axis=-1)
    motion = np.zeros((h, w, 4, 3), np.float32)
    motion[..., 0:2] = rng.uniform(-6.0, 6.0, size=(h, w, 4, 2))
    whole = rng.random((h, w, 4)) < 0.25
    motion[..., 0:2][whole] = np.round(motion[..., 0:2][whole])
    far = rng.random((h, w, 4)) < 0.1                                   # across the whole region and beyond
    motion[..., 0:2][far] = rng.uniform(-1.5 * w, 1.5 * w, size=(int(far.sum()), 2))
    motion[..., 2] = rng.choice([0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 3.0], size=(h, w, 4))
    odd = [np.nan, np.inf, -np.inf, 2.0 ** 21, -(2.0 ** 21), 2.0 ** 20, 3.0e9]
    for k, val in enumerate(odd):                                        # code 0 with a motion that must count as invalid (2^20 itself is valid: off the region)
        for comp in (0, 1):
            y, xx, s = rng.integers(0, h), rng.integers(0, w), rng.integers(0, 4)
            motion[y, xx, s] = (1.25, -0.5, 0.0)
            motion[y, xx, s, comp] = val
    # every edge: the border ring moves half a pixel outwards, code 0
    motion[0, :, 0] = (0.0, -0.5, 0.0)
    motion[h - 1, :, 1] = (0.25, 0.5, 0.0)
    motion[:, 0, 2] = (-0.5, 0.0, 0.0)
    motion[:, w - 1, 3] = (0.5, -0.25, 0.0)
    return motion, acc, counts, mom


# ---- the scene of the motion tests ----
W, H = 50, 30
EYE_A, EYE_B, TARGET_DZ = (0.0, 1.0, 6.0), (0.3, 1.0, 6.0), -6.0          # two cameras 0.3 apart, both looking down -z
EYE_BEHIND = (0.0, 1.0, -3.0)                                             # a `from` that has the near half of the floor behind it
DIFFUSE, MIRROR = 0, 1
ELEMENTS = [
    dict(kind="cuboid", surface=DIFFUSE, albedo=(0.7, 0.7, 0.7), min=(-20.0, -0.5, -9.0), max=(20.0, 0.0, 8.0)),    # floor: no edge of it in view
    dict(kind="cuboid", surface=DIFFUSE, albedo=(0.6, 0.3, 0.3), min=(-20.0, 0.0, -8.5), max=(20.0, 3.0, -8.0)),    # wall, standing on the floor; sky above it
    dict(kind="cuboid", surface=DIFFUSE, albedo=(0.3, 0.6, 0.3), min=(-1.2, 0.0, 1.0), max=(-0.2, 1.6, 2.0)),       # the occluder
    dict(kind="sphere", surface=MIRROR, albedo=(0.9, 0.9, 0.9), center=(1.5, 0.7, 0.0), radius=0.7),
]


def motion_scene(ha):
    from guide_chain import tiny_scene
    return tiny_scene(ha, ELEMENTS, eye=EYE_A, target=(EYE_A[0], EYE_A[1], EYE_A[2] + TARGET_DZ), fov=30.0)


def camera_at(ha, eye):
    cam = ha.Camera()
    ha.host_lib().hh_camera_new(ha.Vec3(*eye), ha.Vec3(eye[0], eye[1], eye[2] + TARGET_DZ), ha.Vec3(0.0, 1.0, 0.0), 30.0, 0, 0.0, 5.0, C.byref(cam))
    return cam


class HostMotion:
    """The host form over one scene (an hr_scene_desc pointer)."""

    def __init__(self, desc_ptr):
        self.lib = motion_lib()
        h = _P()
        rc = self.lib.mh_scene_create(C.cast(desc_ptr, _P), C.byref(h))
        if rc != 0:
            raise RuntimeError("mh_scene_create failed: %d" % rc)
        self._h = h

    def close(self):
        if self._h:
            self.lib.mh_scene_destroy(self._h)
            self._h = None

    def motion(self, from_camera, w=W, h=H, window=None, min_roughness=0.3, depth_tolerance=1e-3):
        x0, y0, ww, hh = window or (0, 0, w, h)
        out, elem = np.zeros((hh, ww, 4, 3), np.float32), np.zeros((hh, ww, 4), np.int32)
        rc = self.lib.mh_motion(self._h, C.cast(C.pointer(from_camera), _P), w, h, x0, y0, ww, hh, min_roughness, depth_tolerance, out.ctypes.data, elem.ctypes.data)
        assert rc == 0
        return out, elem


def _v(p):
    return np.array([p.x, p.y, p.z], dtype=np.float64)


def _closest(o, d):
    """Closest hit of rays o + t d (n, 3) with ELEMENTS in f64: (t, element), t = inf and element -1 for a miss."""
    n = d.shape[0]
    best, elem = np.full(n, np.inf), np.full(n, -1)
    with np.errstate(all="ignore"):
        for k, e in enumerate(ELEMENTS):
            if e["kind"] == "cuboid":
                lo, hi = np.array(e["min"]), np.array(e["max"])
                t0, t1 = (lo - o) / d, (hi - o) / d
                near, far = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
                t = np.where(near > 1e-9, near, far)
                hit = (near <= far) & (far > 1e-9)
            else:
                oc = o - np.array(e["center"])
                b, c = (oc * d).sum(axis=1), (oc * oc).sum(axis=1) - e["radius"] ** 2
                disc = b * b - c
                sq = np.sqrt(np.where(disc > 0, disc, 0.0))
                t = np.where(-b - sq > 1e-9, -b - sq, -b + sq)
                hit = (disc > 0) & (t > 1e-9)
            closer = hit & (t < best)
            best, elem = np.where(closer, t, best), np.where(closer, k, elem)
    return best, elem


def reference_motion(cam, cam_from, w=W, h=H, jitter=None, depth_tolerance=1e-3):
    """The plane in f64 numpy: {mx, my, code} (h, w, 4, 3) float64 and the element hit.  jitter: (h, w, 4, 2) offsets of the primary rays in pixels."""
    from reproject_numpy import cam_array
    yy, xx, ss = np.mgrid[0:h, 0:w, 0:4]
    px, py, sub = xx.ravel(), yy.ravel(), ss.ravel()
    ox, oy = (sub & 1) * 0.5 - 0.5, (sub >> 1) * 0.5 - 0.5
    fx, fy = px + ox, (h - py) + oy
    if jitter is not None:
        fx, fy = fx + jitter[..., 0].ravel(), fy + jitter[..., 1].ravel()
    m = float(min(w, h))
    ncx, ncy = (fx * 2.0 - w) / m, (fy * 2.0 - h) / m
    eye = _v(cam.eye)
    d = ncx[:, None] * _v(cam.plane_half_right) + ncy[:, None] * _v(cam.plane_half_up) + cam.focus_distance * _v(cam.forward)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(eye, d.shape)
    t, elem = _closest(o, d)
    hit = elem >= 0
    x = np.where(hit[:, None], o + np.where(hit, t, 0.0)[:, None] * d, d)
    c0 = cam_array(cam_from)
    eye0, fwd, phr, phu, focus = c0[0:3], c0[3:6], c0[6:9], c0[9:12], c0[12]
    v = np.where(hit[:, None], x - eye0, d)
    c = v @ fwd
    with np.errstate(all="ignore"):
        k = c / focus
        n0x, n0y = (v @ phr) / ((phr @ phr) * k), (v @ phu) / ((phu @ phu) * k)
        f0x, f0y = (n0x * m + w) / 2.0, (n0y * m + h) / 2.0
        mx, my = f0x - (px + ox), ((h - py) + oy) - f0y              # against the sub-sample's OWN coordinate, jittered or not
        inside = (f0x >= -1.0) & (f0x <= w + 1.0) & (f0y >= -1.0) & (f0y <= h + 1.0)
    surface = np.array([e["surface"] for e in ELEMENTS] + [DIFFUSE])[elem]
    code = np.zeros(px.shape[0])
    view_dependent = hit & (surface == MIRROR)
    behind = ~view_dependent & ~(c > 0.0)
    off = ~view_dependent & ~behind & ~inside
    ask = ~view_dependent & ~behind & ~off
    length = np.linalg.norm(v, axis=1)
    t2, e2 = _closest(np.broadcast_to(eye0, v.shape), v / length[:, None])
    visible = np.where(hit, (e2 >= 0) & (np.abs(t2 - length) <= depth_tolerance * length), e2 < 0)
    code[view_dependent] = 3.0
    code[behind | off] = 1.0
    code[ask & ~visible] = 2.0
    zero = view_dependent | behind
    out = np.stack([np.where(zero, 0.0, mx), np.where(zero, 0.0, my), code], axis=-1).reshape(h, w, 4, 3)
    return out, elem.reshape(h, w, 4)


def dilate(mask, r=1):
    """(h, w) bool: true within r pixels (Chebyshev) of a true pixel"""
    h, w = mask.shape
    out = np.zeros_like(mask)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out[max(0, dy):h + min(0, dy), max(0, dx):w + min(0, dx)] |= mask[max(0, -dy):h + min(0, -dy), max(0, -dx):w + min(0, -dx)]
    return out
