"""Shared by tests/test_shade_functions_cpu.py and tests/test_shade_functions_gpu.py: point sets for the material functions of csrc/pt_core.h
(bsdf_eval, bsdf_sample), the f64 forms of precise shading (csrc/prec_core.h) and the tone-map curve (csrc/post_core.h), the f64 oracle's answer
and its own sensitivity at every point, and the check.  The functions are asked through tests/shade_probe (one source, a g++ build and a gfx950
build).  Not a test module, and no GPU code.

Inputs are fp32 values (draws are fp32 as in the hand-off record, unit vectors are fp32-rounded unit vectors); the oracle gets exactly those
values widened to f64, so what is compared is arithmetic alone.

Measure: the project's floor-1 relative error |got - ref| / max(1, |ref|) — per component for directions, against max(1, |pos|) for origins.

Sensitivity, from the oracle alone: `sens` = the largest change of the oracle's output, in the same measure, when ONE input component moves to
its fp32 neighbour, either way (every component of view, n, light / pos, r0, r1, roughness, param: 22 / 26 moved evaluations per point).  A draw
does not leave [0, 1 - 2^-24] and a roughness does not go below 0 (the functions are not defined there).  A point is FRAGILE when such a move
changes an oracle decision — Some / None, reflected / transmitted (total reflection shows as that: beside the critical angle Fresnel's reflectance
is 1 and the outputs of the two branches are the same), the sign of l.n in bsdf — or makes the oracle's own expression non-finite.

A point passes when err <= max(T, K sens), T = 1e-5, K = 8:
  T: two orders under the whole-path bound (SAME_MAX = 1e-3), one order over what a plain fp32 evaluation shows at insensitive points, well over
     the measured v_sin / v_cos error of 1.2e-7 (profiles/NOTES.md);
  K: `sens` is a maximum over single-component moves, up to 13 components are rounded at once and the evaluation's own roundings add to that.
The f64 forms: T64 = 1e-13, no sensitivity clause (the reference's expressions in f64 on identical f64 inputs).
Where a decision differs from the oracle's the point must be fragile, and its values are not compared.  Wherever the oracle's output is finite and
below 1e30 the value under test must be finite: the sensitivity clause never excuses an inf or a NaN."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hanamaru-renderer_amd", "csrc")
PROBE_SRC = os.path.join(ROOT, "tests", "shade_probe", "shade_probe.hip")
DEVICE_PROBE = os.path.join(ROOT, "tests", "shade_probe", "libshade_probe.so")

T = 1e-5
K = 8.0
T64 = 1e-13
BIG = 1e30                   # what path_radiance_in clamps an overflow to: beyond it the oracle's value is not compared
MAX_FRAGILE = 0.01           # share of a set
MAX_CLAUSE = 0.10            # share of a GENERAL set at which K sens exceeds T
F32 = np.float32
ONE_M = float(F32(1.0) - F32(2.0 ** -24))       # the largest draw

DIFFUSE, SPECULAR, REFRACTION, GGX, GGX_REFRACTION = 0, 1, 2, 3, 4
ROUGHNESSES = [1e-3, 1e-2, 0.05, 0.2, 0.5, 1.0]
F0S = [0.0, 0.04, 0.8, 1.0]
IORS = [1.0, 1.0001, 0.8, 1.33, 1.5, 5.0]
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
MIN_NORMAL = 1.17549435e-38
DENORMAL = 1e-40


# ------------------------------------------------------------------------------------------------------------------------------------------
# the probe: ctypes over tests/shade_probe/shade_probe.hip
def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Probe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        for name in ("sp_bsdf_eval", "sp_bsdf_sample", "sp_sincos_2pi_f64", "sp_sample_diffuse_f64", "sp_sample_ggx_half_f64",
                     "sp_sample_refraction_f64", "sp_ggx_refl_f64", "sp_tonemap_gamma", "sp_gamma_to_linear"):
            getattr(self.lib, name).restype = C.c_int
        self.device = bool(self.lib.sp_is_device_build())

    def _call(self, name, n, *arrays):
        f = getattr(self.lib, name)
        rc = f(C.c_size_t(n), *[_ptr(a) for a in arrays])
        if rc != 0:
            raise RuntimeError("%s: HIP error %d" % (name, rc))

    @staticmethod
    def _c(a, dtype):
        return np.ascontiguousarray(a, dtype=dtype)

    def bsdf_eval(self, p):
        n = len(p["surface"])
        out = np.zeros(n, F32)
        self._call("sp_bsdf_eval", n, self._c(p["surface"], np.int32), self._c(p["param"], F32), self._c(p["roughness"], F32),
                   self._c(p["view"], F32), self._c(p["n"], F32), self._c(p["light"], F32), out)
        return out

    def bsdf_sample(self, p):
        """[n, 9] float64 in the oracle's layout {some, origin, direction, reflectance, transmitted} (fp32 values widened)"""
        n = len(p["surface"])
        some, tr = np.zeros(n, np.int32), np.zeros(n, np.int32)
        org, dr, refl = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, F32)
        self._call("sp_bsdf_sample", n, self._c(p["surface"], np.int32), self._c(p["param"], F32), self._c(p["roughness"], F32), self._c(p["r0"], F32),
                   self._c(p["r1"], F32), self._c(p["pos"], F32), self._c(p["view"], F32), self._c(p["n"], F32), some, tr, org, dr, refl)
        return np.concatenate([some[:, None], org, dr, refl[:, None], tr[:, None]], axis=1).astype(np.float64)

    def sincos_2pi_f64(self, r):
        r = self._c(r, np.float64)
        sn, cs = np.zeros_like(r), np.zeros_like(r)
        self._call("sp_sincos_2pi_f64", len(r), r, sn, cs)
        return sn, cs

    def sample_diffuse_f64(self, r0, r1, nrm):
        out = np.zeros((len(r0), 3))
        self._call("sp_sample_diffuse_f64", len(r0), self._c(r0, np.float64), self._c(r1, np.float64), self._c(nrm, np.float64), out)
        return out

    def sample_ggx_half_f64(self, r0, r1, nrm, alpha2):
        out = np.zeros((len(r0), 3))
        self._call("sp_sample_ggx_half_f64", len(r0), self._c(r0, np.float64), self._c(r1, np.float64), self._c(nrm, np.float64), self._c(alpha2, np.float64), out)
        return out

    def sample_refraction_f64(self, r0, pos, ray, nrm, ior):
        n = len(r0)
        tr, org, dr, refl = np.zeros(n, np.int32), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, F32)
        self._call("sp_sample_refraction_f64", n, self._c(r0, np.float64), self._c(pos, np.float64), self._c(ray, np.float64), self._c(nrm, np.float64),
                   self._c(ior, np.float64), tr, org, dr, refl)
        return tr, org, dr, refl.astype(np.float64)

    def ggx_refl_f64(self, ln, vn, vh, hn, alpha2, f0):
        out = np.zeros(len(ln))
        self._call("sp_ggx_refl_f64", len(ln), *[self._c(a, np.float64) for a in (ln, vn, vh, hn)], self._c(alpha2, F32), self._c(f0, F32), out)
        return out

    def tonemap_gamma(self, rgb, scale):
        out = np.zeros((len(scale), 3), F32)
        self._call("sp_tonemap_gamma", len(scale), self._c(rgb, F32), self._c(scale, F32), out)
        return out

    def gamma_to_linear(self, v):
        out = np.zeros(len(v), F32)
        self._call("sp_gamma_to_linear", len(v), self._c(v, F32), out)
        return out


def build_host_probe(directory):
    """The g++ build, with the flags of tests/emu/Makefile (-mfma: pt_core.h spells its dot / cross products with fmaf)."""
    so = os.path.join(str(directory), "libshade_probe_host.so")
    subprocess.run(["g++", "-x", "c++", "-O2", "-mfma", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-parameter", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, "-shared", "-o", so, PROBE_SRC], check=True)
    p = Probe(so)
    assert not p.device
    return p


def load_device_probe():
    if not os.path.exists(DEVICE_PROBE):
        raise RuntimeError("tests/shade_probe/libshade_probe.so is not built — __graft_entry__.build() (make -C hanamaru-renderer_amd shade_probe) makes it")
    p = Probe(DEVICE_PROBE)
    assert p.device, "tests/shade_probe/libshade_probe.so is not the gfx950 build"
    return p


# ------------------------------------------------------------------------------------------------------------------------------------------
# generators (all f64 arithmetic, rounded to fp32 once)
def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _rand_unit(rng, n):
    return _unit(rng.standard_normal((n, 3)))


def _frame(n64):
    nn = _unit(n64)
    a = np.where(np.abs(nn[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    t = _unit(np.cross(a, nn))
    return nn, t, np.cross(nn, t)


def _dir_at(n64, cos, phi):
    """A unit vector at cosine `cos` to n, azimuth phi."""
    nn, t, b = _frame(n64)
    s = np.sqrt(np.maximum(1.0 - cos * cos, 0.0))
    return cos[:, None] * nn + s[:, None] * (np.cos(phi)[:, None] * t + np.sin(phi)[:, None] * b)


def _hemisphere(rng, n64, lo=0.02):
    m = len(n64)
    return _dir_at(n64, lo + (1.0 - lo) * rng.random(m), 2 * np.pi * rng.random(m))


def _axis_dir(rng, axis, comp):
    """Unit vectors whose component along AXES[axis] is EXACTLY comp (so that the dot product with that normal is comp, signed zeros and
    denormals included); the other two components fill the unit length."""
    m = len(axis)
    k = axis // 2
    sign = np.where(axis % 2 == 0, 1.0, -1.0)
    phi = 2 * np.pi * rng.random(m)
    s = np.sqrt(np.maximum(1.0 - comp * comp, 0.0))
    out = np.zeros((m, 3))
    out[np.arange(m), (k + 1) % 3] = s * np.cos(phi)
    out[np.arange(m), (k + 2) % 3] = s * np.sin(phi)
    out[np.arange(m), k] = sign * comp
    return out


def _normals(rng, m):
    """Half axes, half general directions; an eighth of the general ones straddle tangent_basis's threshold fabsf(n.x) > EPS_F.
    Returns (normals [m, 3] f64 holding fp32 values, axis index or -1)."""
    e = F32(1e-4)
    xs = np.array([0.0, 5e-5, -5e-5, e, np.nextafter(e, F32(1)), np.nextafter(e, F32(0)), -e, -np.nextafter(e, F32(1)), -np.nextafter(e, F32(0)), 2e-4, -2e-4],
                  dtype=np.float64)
    axis = np.full(m, -1)
    out = _rand_unit(rng, m)
    half = m // 2
    axis[:half] = np.arange(half) % 6
    out[:half] = AXES[axis[:half]]
    ns = (m - half) // 8
    nx = xs[np.arange(ns) % len(xs)]
    phi = 2 * np.pi * rng.random(ns)
    s = np.sqrt(1.0 - nx * nx)
    out[half:half + ns] = np.stack([nx, s * np.cos(phi), s * np.sin(phi)], axis=1)
    perm = rng.permutation(m)
    return out[perm].astype(F32).astype(np.float64), axis[perm]


def _pick(rng, values, m):
    return np.asarray(values, dtype=np.float64)[rng.integers(0, len(values), m)]


def _draws(rng, m, special_share=0.25):
    """fp32 draws in [0, 1 - 2^-24]: random, and the corners {0, 2^-24, 1/4, 1/2, 3/4, 1 - 2^-24}."""
    d = rng.random(m).astype(F32).astype(np.float64)
    d = np.minimum(d, ONE_M)
    sp = rng.random(m) < special_share
    d[sp] = _pick(rng, [0.0, 2.0 ** -24, 0.25, 0.5, 0.75, ONE_M], int(sp.sum()))
    return d


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(F32)


def _eval_set(surface, param, roughness, view, n, light, **extra):
    p = {"kind": "eval", "surface": np.asarray(surface, np.int32), "param": _f32(param), "roughness": _f32(roughness), "view": _f32(view), "n": _f32(n),
         "light": _f32(light), "general": False, "may_be_nan": False}
    p["zero_expected"] = np.zeros(len(p["surface"]), bool)
    p.update(extra)
    return p


def _sample_set(surface, param, roughness, r0, r1, pos, view, n, **extra):
    p = {"kind": "sample", "surface": np.asarray(surface, np.int32), "param": _f32(param), "roughness": _f32(roughness), "r0": _f32(r0), "r1": _f32(r1),
         "pos": _f32(pos), "view": _f32(view), "n": _f32(n), "general": False, "may_be_nan": False}
    p.update(extra)
    return p


def gen_eval_general():
    rng = np.random.default_rng(101)
    per = 120
    combos = [(GGX, r, f) for r in ROUGHNESSES for f in F0S] + [(DIFFUSE, 0.3, 1.5)]
    m = per * len(combos)
    n, _ = _normals(rng, m)
    c = np.repeat(np.arange(len(combos)), per)
    tab = np.array(combos)
    return _eval_set(tab[c, 0].astype(np.int32), tab[c, 2], tab[c, 1], _hemisphere(rng, n), n, _hemisphere(rng, n), general=True)


def gen_eval_lobe():
    """light = the mirror direction tilted by roughness x {0, 0.5, 1, 2, 5, 20} (capped at 1 rad), towards a random azimuth."""
    rng = np.random.default_rng(102)
    rough = [1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 0.05, 0.2]
    tilts = [0.0, 0.5, 1.0, 2.0, 5.0, 20.0]
    per = 60
    m = per * len(rough) * len(tilts)
    n, _ = _normals(rng, m)
    r = np.repeat(np.asarray(rough), per * len(tilts))
    t = np.tile(np.repeat(np.asarray(tilts), per), len(rough))
    view = _f32(_hemisphere(rng, n, 0.3)).astype(np.float64)
    nn = _unit(n)
    mirror = _unit(2.0 * (view * nn).sum(-1, keepdims=True) * nn - view)
    delta = np.minimum(r * t, 1.0)
    light = _dir_at(mirror, np.cos(delta), 2 * np.pi * rng.random(m))
    return _eval_set(np.full(m, GGX), _pick(rng, [0.04, 0.8, 1.0], m), r, view, n, light)


def gen_eval_grazing():
    """v.n and l.n in {1e-3 .. a denormal}, each alone and both together, EXACT on axis normals; l.n also exactly +0, -0 and -1e-8 (compared with
    0: bsdf_eval's `!(ln > 0)` rule, test_ggx_nee_sample_exactly_at_the_horizon_adds_nothing); general normals at the one level rounding leaves exact
    enough (1e-3)."""
    rng = np.random.default_rng(103)
    levels = [1e-3, 1e-5, 1e-8, 1e-12, 1e-20, 1e-30, MIN_NORMAL, DENORMAL]
    rough = [1e-2, 0.05, 0.2, 0.5, 1.0]
    per = 16
    rows = [(mode, lv, r) for mode in range(3) for lv in levels for r in rough]
    m = per * len(rows)
    tab = np.array(rows)
    c = np.repeat(np.arange(len(rows)), per)
    mode, lv, r = tab[c, 0].astype(int), _f32(tab[c, 1]).astype(np.float64), tab[c, 2]
    axis = rng.integers(0, 6, m)
    n = AXES[axis]
    free_v, free_l = 0.02 + 0.98 * rng.random(m), 0.02 + 0.98 * rng.random(m)
    view = _axis_dir(rng, axis, np.where(mode != 1, lv, free_v))
    light = _axis_dir(rng, axis, np.where(mode != 0, lv, free_l))
    # the horizon itself
    zs = np.array([0.0, -0.0, -1e-8])
    mz = 12 * len(zs)
    az = rng.integers(0, 6, mz)
    zl = _axis_dir(rng, az, np.repeat(zs, 12))
    zv = _axis_dir(rng, az, 0.02 + 0.98 * rng.random(mz))
    # general normals, 1e-3
    mg = 480
    ng, _ = _normals(rng, mg)
    gm = rng.integers(0, 3, mg)
    gv = _dir_at(ng, np.where(gm != 1, 1e-3, 0.02 + 0.98 * rng.random(mg)), 2 * np.pi * rng.random(mg))
    gl = _dir_at(ng, np.where(gm != 0, 1e-3, 0.02 + 0.98 * rng.random(mg)), 2 * np.pi * rng.random(mg))
    zero = np.concatenate([np.zeros(m, bool), np.ones(mz, bool), np.zeros(mg, bool)])
    tot = m + mz + mg
    return _eval_set(np.full(tot, GGX), _pick(rng, [0.04, 0.8], tot), np.concatenate([r, _pick(rng, rough, mz), _pick(rng, rough, mg)]),
                     np.concatenate([view, zv, gv]), np.concatenate([n, AXES[az], ng]), np.concatenate([light, zl, gl]), zero_expected=zero)


def gen_eval_rough0():
    """roughness exactly 0 and 1e-30 (alpha2 underflows in fp32): random directions, and the mirror direction itself."""
    rng = np.random.default_rng(104)
    m = 1200
    n, _ = _normals(rng, m)
    view = _f32(_hemisphere(rng, n)).astype(np.float64)
    nn = _unit(n)
    mirror = 2.0 * (view * nn).sum(-1, keepdims=True) * nn - view
    light = np.where((np.arange(m) % 2 == 0)[:, None], mirror, _hemisphere(rng, n))
    return _eval_set(np.full(m, GGX), _pick(rng, F0S, m), _pick(rng, [0.0, 1e-30], m), view, n, light, may_be_nan=True)


def _positions(rng, m):
    return _rand_unit(rng, m) * _pick(rng, [0.3, 30.0, 3000.0], m)[:, None]


def gen_sample_general():
    rng = np.random.default_rng(105)
    per = 800
    m = 5 * per
    surface = np.repeat(np.arange(5), per)
    n, _ = _normals(rng, m)
    view = _hemisphere(rng, n)
    refr = (surface == REFRACTION) | (surface == GGX_REFRACTION)
    view = np.where((refr & (rng.random(m) < 0.5))[:, None], -view, view)       # both sides of a dielectric
    param = np.where(refr, _pick(rng, IORS, m), _pick(rng, F0S, m))
    return _sample_set(surface, param, _pick(rng, ROUGHNESSES, m), _draws(rng, m), _draws(rng, m), _positions(rng, m), view, n, general=True)


def gen_sample_mirror_limit():
    """GGX and GGXRefraction towards roughness 0, r1 up to 1 - 2^-24 where 1 + (alpha2 - 1) r1 cancels."""
    rng = np.random.default_rng(106)
    rough = [0.0, 1e-8, 1e-6, 1e-4, 1e-3]
    r1s = [-1.0, 0.5, 0.99, 1.0 - 2.0 ** -12, 1.0 - 2.0 ** -20, ONE_M]
    per = 40
    rows = [(s, r, q) for s in (GGX, GGX_REFRACTION) for r in rough for q in r1s]
    m = per * len(rows)
    tab = np.array(rows)
    c = np.repeat(np.arange(len(rows)), per)
    surface = tab[c, 0].astype(np.int32)
    r1 = np.where(tab[c, 2] < 0, _draws(rng, m, 0.0), tab[c, 2])
    n, _ = _normals(rng, m)
    view = _hemisphere(rng, n, 0.05)
    param = np.where(surface == GGX, _pick(rng, F0S, m), _pick(rng, [1.33, 1.5, 5.0], m))
    return _sample_set(surface, param, tab[c, 1], _draws(rng, m), r1, _positions(rng, m), view, n)


def gen_sample_grazing():
    """GGX with v.n down to the smallest normal (exact, on axis normals) — half vectors whose h.n v.n underflows: r1 at 1 - 2^-24 with roughness 1;
    refraction beside the critical angle (a few ulps to a few thousand) and at normal incidence."""
    rng = np.random.default_rng(107)
    levels = [1e-3, 1e-5, 1e-8, 1e-12, 1e-20, 1e-30, 1e-36, MIN_NORMAL]
    rough = [1e-3, 0.05, 0.5, 1.0]
    per = 24
    rows = [(lv, r) for lv in levels for r in rough]
    m = per * len(rows)
    tab = np.array(rows)
    c = np.repeat(np.arange(len(rows)), per)
    axis = rng.integers(0, 6, m)
    view = _axis_dir(rng, axis, _f32(tab[c, 0]).astype(np.float64))
    r1 = _draws(rng, m, 0.0)
    r1[::3] = ONE_M
    parts = [dict(surface=np.full(m, GGX), param=_pick(rng, [0.04, 0.8], m), roughness=tab[c, 1], r0=_draws(rng, m), r1=r1, view=view, n=AXES[axis])]
    # the critical angle from inside glass / water: view.n = -cos(theta_c) (1 + k 2^-23)
    ks = np.array([0, 1, -1, 2, -2, 4, -4, 64, -64, 4096, -4096], dtype=np.float64)
    mc = 40 * len(ks)
    axis = rng.integers(0, 6, mc)
    ior = _pick(rng, [1.33, 1.5], mc)
    cosc = np.sqrt(1.0 - 1.0 / (ior * ior))
    comp = -(_f32(cosc).astype(np.float64) * (1.0 + np.repeat(ks, 40) * 2.0 ** -23))
    parts.append(dict(surface=np.full(mc, REFRACTION), param=ior, roughness=np.full(mc, 0.3), r0=_draws(rng, mc), r1=_draws(rng, mc),
                      view=_axis_dir(rng, axis, comp), n=AXES[axis]))
    # normal incidence, either side, exact and to rounding
    mn = 240
    nn, _ = _normals(rng, mn)
    side = np.where(rng.random(mn) < 0.5, 1.0, -1.0)[:, None]
    parts.append(dict(surface=_pick(rng, [REFRACTION, GGX_REFRACTION], mn).astype(np.int32), param=_pick(rng, IORS, mn), roughness=_pick(rng, [1e-3, 0.05], mn),
                      r0=_draws(rng, mn), r1=_draws(rng, mn), view=side * nn, n=nn))
    cat = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    tot = len(cat["surface"])
    return _sample_set(cat["surface"], cat["param"], cat["roughness"], cat["r0"], cat["r1"], _positions(rng, tot), cat["view"], cat["n"])


GENERATORS = {"eval_general": gen_eval_general, "eval_lobe": gen_eval_lobe, "eval_grazing": gen_eval_grazing, "eval_rough0": gen_eval_rough0,
              "sample_general": gen_sample_general, "sample_mirror_limit": gen_sample_mirror_limit, "sample_grazing": gen_sample_grazing}
SETS = sorted(GENERATORS)
GENERAL_SETS = ["eval_general", "sample_general"]


# ------------------------------------------------------------------------------------------------------------------------------------------
# the oracle's answer and its sensitivity
def _orc():
    import oracle_py
    return oracle_py


def _w(a):
    return np.asarray(a, dtype=F32).astype(np.float64)


def oracle_outputs(p):
    """(values [n, m], denominators' floor [n, m] or None, decision [n] int) for a dict of fp32 inputs."""
    orc = _orc()
    if p["kind"] == "eval":
        v, n, l = _w(p["view"]), _w(p["n"]), _w(p["light"])
        val = orc.material_bsdf_n(p["surface"], _w(p["param"]), _w(p["roughness"]), v, n, l)
        ln = (l[:, 0] * n[:, 0] + l[:, 1] * n[:, 1]) + l[:, 2] * n[:, 2]            # the oracle's dot(), term by term
        dec = np.where(p["surface"] == GGX, np.signbit(ln).astype(int), 0)
        return val[:, None], dec
    o = orc.material_sample_n(p["surface"], _w(p["param"]), _w(p["roughness"]), _w(p["r0"]), _w(p["r1"]), _w(p["pos"]), _w(p["view"]), _w(p["n"]))
    return sample_values(o), sample_decision(o)


def sample_values(o):
    """[n, 9] {some, origin, direction, reflectance, transmitted} -> [n, 7] {direction, origin, reflectance}"""
    return np.concatenate([o[:, 4:7], o[:, 1:4], o[:, 7:8]], axis=1)


def sample_decision(o):
    return (o[:, 0] != 0).astype(int) + 2 * (o[:, 8] != 0).astype(int)


def floors(p, ref):
    """The denominators of the measure: max(1, |ref|) per component; origins against max(1, |pos|)."""
    den = np.maximum(1.0, np.abs(np.where(np.isfinite(ref), ref, 0.0)))
    if p["kind"] == "sample":
        den[:, 3:6] = np.maximum(1.0, np.sqrt((_w(p["pos"]) ** 2).sum(-1)))[:, None]
    return den


def measure(a, ref, den):
    """max over the components of |a - ref| / den; inf where either is not finite."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(a - ref) / den
    e = np.where(np.isfinite(e), e, np.inf)
    return e.max(axis=1)


MOVED = {"eval": [("view", 3), ("n", 3), ("light", 3), ("roughness", 0), ("param", 0)],
         "sample": [("view", 3), ("n", 3), ("pos", 3), ("r0", 0), ("r1", 0), ("roughness", 0), ("param", 0)]}


def _neighbours(p):
    """Every input with ONE component moved to its fp32 neighbour, either way."""
    for field, comps in MOVED[p["kind"]]:
        for j in range(max(comps, 1)):
            for toward in (np.inf, -np.inf):
                q = dict(p)
                a = np.array(p[field], dtype=F32)
                col = a[:, j] if comps else a
                moved = np.nextafter(col, F32(toward))
                if field in ("r0", "r1"):
                    moved = np.where((moved >= 0) & (moved <= F32(ONE_M)), moved, col)
                if field == "roughness":
                    moved = np.where(moved >= 0, moved, col)
                if comps:
                    a[:, j] = moved
                else:
                    a = moved
                q[field] = a
                yield q


_cache = {}


def get(name):
    """The set with the oracle's answer: ref [n, m], den, decision, sens [n], fragile [n].  Built once per process and left unchanged."""
    if name not in _cache:
        p = GENERATORS[name]()
        ref, dec = oracle_outputs(p)
        if not p["may_be_nan"]:
            # a generator may produce a point at which the reference's own expression is not finite (sqrt(1 - cos^2) of a quotient that rounded above
            # 1: roughness 1e-8; 0 / 0 on the horizon): such points are dropped here, from the oracle alone — except the horizon points, compared with 0
            keep = np.isfinite(ref).all(axis=1)
            if p["kind"] == "eval":
                keep |= p["zero_expected"]
            if not keep.all():
                for k, v in list(p.items()):
                    if isinstance(v, np.ndarray):
                        p[k] = v[keep]
                p["dropped"] = int((~keep).sum())
                ref, dec = ref[keep], dec[keep]
        p.setdefault("dropped", 0)
        den = floors(p, ref)
        sens = np.zeros(len(ref))
        fragile = np.zeros(len(ref), bool)
        for q in _neighbours(p):
            r2, d2 = oracle_outputs(q)
            flip = d2 != dec
            broken = ~np.isfinite(r2).all(axis=1) & np.isfinite(ref).all(axis=1)
            fragile |= flip if p["may_be_nan"] else flip | broken         # (eval_rough0 is finite whatever the oracle is: nothing to excuse there)
            s = measure(r2, ref, den)
            sens = np.maximum(sens, np.where(flip | broken, 0.0, s))
        p.update(name=name, ref=ref, den=den, decision=dec, sens=sens, fragile=fragile)
        for v in p.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = p
    return _cache[name]


def oracle_conditions(p):
    """What the oracle alone must meet on a set (asserted by the CPU tier): returns the figures, raises on a miss."""
    n = len(p["ref"])
    live = ~p["zero_expected"] if p["kind"] == "eval" else np.ones(n, bool)
    finite = np.isfinite(p["ref"]).all(axis=1)
    fig = {"points": n, "dropped": p["dropped"], "fragile": float((p["fragile"] & live).mean()), "clause": float((K * p["sens"] > T)[live].mean()),
           "oracle_not_finite": int((~finite & live).sum()), "oracle_beyond_big": int((np.abs(np.where(finite[:, None], p["ref"], 0.0)).max(axis=1) >= BIG).sum())}
    assert n >= 1000, (p["name"], n)
    assert fig["fragile"] <= MAX_FRAGILE, (p["name"], fig)
    if p["general"]:
        assert fig["clause"] <= MAX_CLAUSE, (p["name"], fig)
    if not p["may_be_nan"]:
        assert fig["oracle_not_finite"] == 0, (p["name"], fig)
    return fig


# ------------------------------------------------------------------------------------------------------------------------------------------
# the check
def run_probe(probe, p):
    """(values [n, m], decision [n]) of the build under test, in the oracle's layout."""
    if p["kind"] == "eval":
        got = probe.bsdf_eval(p).astype(np.float64)
        return got[:, None], None
    o = probe.bsdf_sample(p)
    return sample_values(o), sample_decision(o)


def check(p, got, got_dec, label, t=T, k=K):
    """Every point: finite where the oracle is finite and below BIG; the decision the oracle's, or the point fragile; err <= max(t, k sens).
    Returns (figures, list of failures); the caller asserts the list empty after printing the figures."""
    ref, den, sens, fragile = p["ref"], p["den"], p["sens"], p["fragile"]
    n = len(ref)
    ref_ok = np.isfinite(ref).all(axis=1) & (np.abs(np.where(np.isfinite(ref), ref, 0.0)).max(axis=1) < BIG)
    got_finite = np.isfinite(got).all(axis=1)
    target = ref
    zero = p["zero_expected"] if p["kind"] == "eval" else np.zeros(n, bool)
    if zero.any():
        target = np.where(zero[:, None], 0.0, ref)
        ref_ok = ref_ok | zero
    if p["kind"] == "eval":
        # bsdf_eval has one decision, the sign of l.n, seen as an exact 0: differing there is excused at a fragile point only
        mismatch = ((got[:, 0] == 0) != (target[:, 0] == 0)) & fragile
        hard_mismatch = np.zeros(n, bool)
    else:
        mismatch = got_dec != p["decision"]
        hard_mismatch = mismatch & ~fragile
    err = measure(got, target, np.where(zero[:, None], 1.0, den))
    bound = np.maximum(t, k * np.where(zero, 0.0, sens))
    compared = ref_ok & ~mismatch
    value_bad = compared & ~(err <= bound)
    not_finite = ref_ok & ~mismatch & ~got_finite
    if p["may_be_nan"]:
        not_finite = ~got_finite          # this set: finite everywhere, whatever the oracle's own expression gives
    bad = value_bad | not_finite | hard_mismatch
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(compared & np.isfinite(err), err, 0.0)
        over = e > t
        ratio_s = np.where(over, e / (k * np.where(sens > 0, sens, np.inf)), 0.0)
    fig = {"label": label, "set": p["name"], "points": n, "compared": int(compared.sum()), "clause_share": float(over.sum()) / max(1, int(compared.sum())),
           "worst_err_over_T": float(e.max() / t), "worst_err_over_Ksens": float(ratio_s.max()),
           "fragile_mismatches": int((mismatch & fragile).sum()), "not_finite": int(not_finite.sum()), "oracle_not_compared": int((~ref_ok).sum()),
           "failures": int(bad.sum())}
    fails = []
    for i in np.flatnonzero(bad)[:12]:
        why = "not finite" if not_finite[i] else "decision" if hard_mismatch[i] else "value"
        inputs = {f: np.asarray(p[f][i]).tolist() for f, _ in MOVED[p["kind"]]}
        fails.append("%s #%d (%s): got %s ref %s err %.3g bound %.3g sens %.3g surface %d %s" % (
            p["name"], i, why, got[i].tolist(), target[i].tolist(), err[i], bound[i], sens[i], int(p["surface"][i]), inputs))
    return fig, fails


def report_line(fig):
    return ("%(set)s [%(label)s]: %(points)d points, %(compared)d compared, %(clause_share).4f need K sens, worst err/T %(worst_err_over_T).3f, "
            "worst err/(K sens) %(worst_err_over_Ksens).3f, fragile mismatches %(fragile_mismatches)d, not finite %(not_finite)d, "
            "oracle not comparable %(oracle_not_compared)d, failures %(failures)d" % fig)


def check_set(probe, name, label):
    p = get(name)
    got, dec = run_probe(probe, p)
    fig, fails = check(p, got, dec, label)
    print(report_line(fig))
    assert not fails, "%d points of %s fail on %s:\n%s" % (fig["failures"], name, label, "\n".join(fails))
    return fig


# ------------------------------------------------------------------------------------------------------------------------------------------
# the f64 forms and the post curve: plain comparisons (no sensitivity clause)
def f64_inputs():
    """The draws and normals of sample_general as f64 values — the fp32 value plus a residual, as precise shading reads them."""
    if "f64" not in _cache:
        rng = np.random.default_rng(108)
        g = get("sample_general")
        m = len(g["r0"])
        r0 = np.clip(_w(g["r0"]) + (rng.random(m) - 0.5) * 2.0 ** -25, 0.0, 1.0 - 2.0 ** -53)
        r1 = np.clip(_w(g["r1"]) + (rng.random(m) - 0.5) * 2.0 ** -25, 0.0, 1.0 - 2.0 ** -53)
        n = _unit(_w(g["n"]))                                  # unit to f64, as the f64 normal of a hit is
        n[::2] = _w(g["n"])[::2]                               # and the fp32 values themselves (axes, the straddle of 1e-4)
        _cache["f64"] = {"r0": r0, "r1": r1, "n": n, "pos": _w(g["pos"]), "view": _w(g["view"]), "m": m, "rng_seed": 108,
                         "roughness": _pick(rng, [1e-2, 0.05, 0.2, 0.5, 1.0], m), "ior": _pick(rng, IORS, m), "f0": _pick(rng, F0S, m)}
    return _cache["f64"]


def sincos_points():
    """Quadrant boundaries to a few f64 ulps, 0, 1 - 2^-53, the fp32 corners and random draws."""
    rng = np.random.default_rng(109)
    q = np.array([0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875])
    near = np.concatenate([q + k * 2.0 ** -53 for k in (-4, -2, -1, 0, 1, 2, 4)])
    return np.clip(np.concatenate([near, [1.0 - 2.0 ** -53, 2.0 ** -24, ONE_M, 5e-324, 1e-300], rng.random(2000)]), 0.0, 1.0 - 2.0 ** -53)


def sincos_reference(r):
    """sin / cos of 2 pi r with the quadrant taken off exactly first (r - q / 4 is exact), so that the reference has no argument-reduction error."""
    q = np.floor(r * 4.0 + 0.5)
    x = (r - q * 0.25) * (2 * np.pi)
    sx, cx = np.sin(x), np.cos(x)
    k = q.astype(int) & 3
    return np.choose(k, [sx, cx, -sx, -cx]), np.choose(k, [cx, -sx, -cx, sx])


def post_points():
    """(rgb [n, 3] fp32, accumulator values) for tonemap_gamma: 0, denormals, 1e30 (what path_radiance_in clamps to), 4096 x 1e30 (that, summed over the
    longest render), the top of fp32, greys and colours log-uniform over [1e-12, 3e38]."""
    rng = np.random.default_rng(110)
    m = 2000
    grey = 10.0 ** rng.uniform(-12, np.log10(3e38), m)
    rgb = grey[:, None] * np.where((rng.random((m, 1)) < 0.5), 1.0, rng.random((m, 3)))
    sp = np.array([0.0, 1e-45, DENORMAL, MIN_NORMAL, 1e-30, 1.0, 20.0, 1e30, 4096e30, 3e38])
    special = np.concatenate([np.repeat(sp[:, None], 3, axis=1), np.stack([sp, np.zeros_like(sp), sp[::-1]], axis=1)])
    return np.minimum(np.concatenate([special, rgb]), 3e38).astype(F32)


def gamma_points():
    rng = np.random.default_rng(111)
    k = np.arange(256) / 255.0
    sums = (k[rng.integers(0, 256, 500)] * 0.25 + k[rng.integers(0, 256, 500)] * 0.75)          # bilinear blends of texels
    return np.concatenate([k, sums, [0.0, 1e-45, DENORMAL, MIN_NORMAL, 1e-30, 1e-10], rng.random(1000)]).astype(F32)


def _plain(what, got, ref, den, tol, label, worst):
    err = measure(np.asarray(got).reshape(len(ref), -1), np.asarray(ref).reshape(len(ref), -1), np.asarray(den).reshape(len(ref), -1))
    worst[what] = float(err.max())
    i = int(err.argmax())
    assert err.max() <= tol, "%s on %s: point %d of %d is off by %.3g (bound %.3g): got %s, expected %s" % (
        what, label, i, len(ref), err[i], tol, np.asarray(got)[i].tolist(), np.asarray(ref)[i].tolist())


def check_f64_forms(probe, label, skew=0.0):
    """The f64 forms of precise shading against the oracle's expressions on identical f64 inputs: T64, no sensitivity clause.  `skew`: a relative
    error put on the EXPECTED values (the tests of the check itself).  Returns the worst error per entry."""
    orc = _orc()
    worst = {}
    k = 1.0 + skew
    r = sincos_points()
    sn, cs = probe.sincos_2pi_f64(r)
    rs, rc = sincos_reference(r)
    _plain("sincos_2pi_f64", np.stack([sn, cs], 1), np.stack([rs, rc], 1) * k, np.ones((len(r), 2)), T64, label, worst)
    f = f64_inputs()
    m = f["m"]
    r0, r1, n, pos, view = f["r0"], f["r1"], f["n"], f["pos"], f["view"]
    one = np.ones((m, 3))
    ref = orc.material_sample_n(np.full(m, DIFFUSE), np.ones(m), np.ones(m), r0, r1, pos, view, n)
    _plain("sample_diffuse_f64", probe.sample_diffuse_f64(r0, r1, n), ref[:, 4:7] * k, one, T64, label, worst)
    rough = _w(f["roughness"])
    half = orc.ggx_half_n(r0, r1, n, rough * rough)
    assert np.isfinite(half).all()
    # The reference takes the sine as sqrt(1 - cos^2): a rounding of cos^2 (1.1e-16, and which products are fused decides which way) is 5.5e-17 / sin
    # of the half vector — beyond T64 from sin = 5.5e-4 down, whatever evaluates the expression.  Compared where sin^2 >= 1e-4 (5.5e-15 from that rounding), and at r1 = 0,
    # where cos is 1 exactly; the narrow lobes are the fp32 sets' business (sample_mirror_limit), which hold the direction itself to T.
    sin2 = rough * rough * r1 / (1.0 + (rough * rough - 1.0) * r1)
    wide = (sin2 >= 1e-4) | (r1 == 0.0)
    assert wide.sum() > m // 2
    worst["half vectors compared"] = int(wide.sum())
    _plain("sample_ggx_half_f64", probe.sample_ggx_half_f64(r0[wide], r1[wide], n[wide], (rough * rough)[wide]), half[wide] * k, one[wide], T64, label, worst)
    ior = _w(f["ior"])
    ref = orc.material_sample_n(np.full(m, REFRACTION), ior, np.ones(m), r0, r1, pos, view, n)
    tr, org, dr, refl = probe.sample_refraction_f64(r0, pos, -view, n, ior)
    assert np.array_equal(tr != 0, ref[:, 8] != 0), "%s: sample_refraction_f64 transmits where the oracle reflects (or the reverse) at %s" % (
        label, np.flatnonzero((tr != 0) != (ref[:, 8] != 0))[:8].tolist())
    worst["transmitted"] = int((tr != 0).sum())
    _plain("sample_refraction_f64 direction", dr, ref[:, 4:7] * k, one, T64, label, worst)
    _plain("sample_refraction_f64 origin", org, ref[:, 1:4] * k, np.maximum(1.0, np.sqrt((pos * pos).sum(-1)))[:, None] * one, T64, label, worst)
    # (the scalar leaves as a float: one fp32 rounding, 2^-24 of the value, on top of T64)
    _plain("sample_refraction_f64 reflectance", refl, ref[:, 7] * k, np.maximum(1.0, np.abs(ref[:, 7])), T64 + 2.0 ** -24, label, worst)
    # the GGX bounce's scalar from its four dot products, those of the bounce the oracle's half vector gives
    d = -view
    nd = d - 2.0 * (d * half).sum(-1, keepdims=True) * half
    ln, vn, vh, hn = (nd * n).sum(-1), (view * n).sum(-1), (view * half).sum(-1), (half * n).sum(-1)
    up = (ln > 0) & wide
    a2 = (f["roughness"].astype(F32) * f["roughness"].astype(F32))
    f0 = f["f0"].astype(F32)
    ref = orc.ggx_scalar_n(ln[up], vn[up], vh[up], hn[up], _w(a2[up]), _w(f0[up]))
    assert up.sum() > m // 4 and np.isfinite(ref).all()
    _plain("ggx_refl_f64", probe.ggx_refl_f64(ln[up], vn[up], vh[up], hn[up], a2[up], f0[up]), ref * k, np.maximum(1.0, np.abs(ref)), T64, label, worst)
    print("f64 forms [%s]: worst error %s (T64 = %.0e)" % (label, ", ".join("%s %.3g" % kv for kv in sorted(worst.items())), T64))
    return worst


def check_post(probe, label, skew=0.0):
    """tonemap_gamma against the tone-map stage of orc_resolve (1 x N images, one sampling: scale = 1 / SUPERSAMPLING^2 = 0.25, exact in fp32) and
    gamma_to_linear against x^2.2 in f64: tolerance T, every output finite."""
    orc = _orc()
    worst = {}
    rgb = post_points()
    _, stage = orc.resolve(rgb.astype(np.float64)[None, :, :], 1, want_stage=True)
    got = probe.tonemap_gamma(rgb, np.full(len(rgb), 0.25, F32))
    assert np.isfinite(stage).all() and np.isfinite(got).all(), "%s: tonemap_gamma is not finite at %s" % (label, rgb[~np.isfinite(got).all(axis=1)][:8].tolist())
    _plain("tonemap_gamma", got, stage[0] * (1.0 + skew), np.ones((len(rgb), 3)), T, label, worst)
    v = gamma_points()
    got = probe.gamma_to_linear(v)
    assert np.isfinite(got).all()
    _plain("gamma_to_linear", got, v.astype(np.float64) ** 2.2 * (1.0 + skew), np.ones(len(v)), T, label, worst)
    print("post [%s]: %d + %d points, worst error %s (T = %.0e)" % (label, len(rgb), len(v), ", ".join("%s %.3g" % kv for kv in sorted(worst.items())), T))
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------------
# bsdf in numpy f64 with its constants open to change — the deliberately wrong EXPECTED values that show the check has teeth
def numpy_bsdf(p, schlick_exponent=5, inv_pi=1.0 / np.pi, alpha_power=2):
    v, n, l = _w(p["view"]), _w(p["n"]), _w(p["light"])
    a2 = _w(p["roughness"]) ** alpha_power
    f0 = _w(p["param"])
    h = _unit(l + v)
    ln, vn, vh, hn = (l * n).sum(-1), (v * n).sum(-1), (v * h).sum(-1), (h * n).sum(-1)
    with np.errstate(all="ignore"):
        tmp = 1.0 - (1.0 - a2) * hn * hn
        d = a2 * inv_pi / (tmp * tmp)
        lam = lambda x: 0.5 * np.sqrt(1.0 + a2 * (1.0 / (x * x) - 1.0)) - 0.5
        g = 1.0 / (1.0 + lam(ln) + lam(vn))
        f = f0 + (1.0 - f0) * (1.0 - vh) ** schlick_exponent
        out = np.where(np.signbit(ln), 0.0, d * g * f / (4.0 * ln * vn))
    return np.where(p["surface"] == DIFFUSE, inv_pi, out)
