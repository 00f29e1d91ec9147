"""Shared by tests/test_lookups_cpu.py and tests/test_lookups_gpu.py: one small scene, point sets for what lies between "the walk found primitive k
at distance t" and "the BSDF is evaluated" — hit_surface, material_at, tex_sample / sample_bilinear / texel, sky_sample in both of its forms, and
the geometry half of shade_hit_f64 (csrc/pt_core.h, csrc/prec_core.h) —, the f64 oracle's answer with its own sensitivity at every point, and the
check.  The functions are asked through hr_debug_surface / hr_debug_sky / hr_debug_texture on the device and through their twins in the host
emulation (csrc/query_core.h is the one written form of both).  Not a test module, and no GPU code.

Every input is an fp32 value and the oracle gets it widened; a ray with a fix is hi + lo on both sides.  One exception, the ray's direction: the
oracle gets the widened direction NORMALISED in f64 (_oracle_surface says why: the reference's sphere quadratic takes |d| = 1 for granted, an
fp32 direction is a unit vector to 6e-8 only and stands for the unit vector along it) — the same line, the oracle's distance in units 6e-8 off the
device's, which T absorbs.  The rule and its constants are
shade_sweeps.py's: the measure is |got - ref| / max(1, |ref|) (positions against max(1, |pos|)), `sens` is the oracle's largest change when ONE input
component moves to its fp32 neighbour, a point passes within max(T, K sens), and wherever the oracle is finite and below BIG the value must be finite.

Decisions are hit / miss, the element, the cuboid face and a sphere u that wraps (a change > 0.5): they may differ from the oracle's only at a
FRAGILE point, one where such a move flips the oracle's own decision (or makes its expression non-finite).  The sky face is not even excused there:
three comparisons and a sign test on inputs both sides hold identically.  A texel quad is not a decision (bilinear interpolation is continuous
across it): how many differ is counted.

Precise mode (shade_hit_f64) splits by how an output is computed: what is computed in f64 and narrowed once (the normal, a cuboid's u, v) passes
within one fp32 ulp (2^-23 of the measure's denominator) + K sens48, sens48 = the oracle's change when a ray component moves by 2^-48 relative, the
resolution of hi + lo; the next ray (out64) within max(T64, K sens48), against the oracle's PointMaterial::sample at the oracle's hit — with the
roughness the device itself reports, widened: that input of the BSDF is an fp32 value by design, and the BSDFs have their own sweeps
(shade_sweeps.py) —; what stays fp32 in precise mode (distance, position, a sphere's or a triangle's u, v, albedo, emission, roughness) by the
fp32 rule.  The texture query's f64 roughness read (roughness_map_f64) passes at T, and the corner it started from is the
oracle's at every point that is not a NaN: a floor in f64 of the same product."""
import ctypes as C

import numpy as np

import corner_scenes as cs
from shade_sweeps import BIG, F32, K, MAX_CLAUSE, MAX_FRAGILE, T, T64, measure

ULP32 = 2.0 ** -23
MAX_FRAGILE_EDGE = 0.5       # the sets made of edges, poles and silhouettes
MIN_COMPARED = 200

# ------------------------------------------------------------------------------------------------------------------------------------------
# the scene
A_LO, A_HI = np.array([-1.0, -0.5, -0.75]), np.array([1.0, 0.5, 0.75])              # fp32-exact corners
B_SHIFT = np.array([2048.0, 0.0, 1024.0])                                              # |pos| > 1700: hit_surface's nearest-face fallback
C_LO, C_HI = np.array([-4.1, 1.3, -0.7]), np.array([-2.3, 2.9, 0.9])                # no fp32 numbers: cuboid_lo != 0
S1 = (np.array([0.3, 1.7, 2.1]), 0.1)                                                 # no fp32 numbers: sphere_lo != 0
S2 = (np.array([4.0, 0.25, -3.0]), 1.0)
S3 = (np.array([300.1, 0.1, 200.3]), 0.1)
QUAD = np.array([[-1.0, -1.0, -6.0], [1.0, -1.0, -6.0], [1.0, 1.0, -6.0], [-1.0, 1.0, -6.0]])
QUAD_FACES = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.uint64)
BOXES = {"A": (A_LO, A_HI), "B": (A_LO + B_SHIFT, A_HI + B_SHIFT), "C": (C_LO, C_HI)}
SPHERES = {"S1": S1, "S2": S2, "S3": S3}
ELEMENT = {"A": 0, "B": 1, "C": 2, "S1": 3, "S2": 4, "S3": 5, "mesh": 6}
KIND = np.array([2, 2, 2, 1, 1, 1, 0])        # per element, TraceState::type: 0 triangle, 1 sphere, 2 cuboid
SKIES = {"nonsquare": cs.SKY_NONSQUARE, "mixed": cs.SKY_MIXED}
EXPECTED_FORM = {"nonsquare": 1, "mixed": 0}   # 1: the footprint table (Scene::sky_quads), 0: the per-face lookup


def set_image(s, k, arr):
    """replace image k of a corner_scenes.Scene (before it is handed to anything)"""
    arr = np.ascontiguousarray(arr)
    s.arrays[k] = arr
    s.img[k].rgba = arr.ctypes.data_as(C.POINTER(C.c_uint8))
    s.img[k].width, s.img[k].height = arr.shape[1], arr.shape[0]


def build_scene(ha, sky, mutate=None, s1_centre=None, s1_radius=None):
    s = cs.Scene(ha, SKIES[sky])
    if mutate:
        mutate(s)
    for name in ("A", "B", "C"):
        s.cuboid(BOXES[name][0], BOXES[name][1], s.material(ha.GGX, 0.8, emission=(0.8, 0.7, 0.9)))
    for name, surf in (("S1", ha.GGX), ("S2", ha.DIFFUSE), ("S3", ha.GGX)):
        m = s.material(surf, 0.8 if surf == ha.GGX else 0.0, emission=(0.5, 0.6, 0.4))
        m.roughness.image = s.ROUGHNESS_2D
        c, r = SPHERES[name]
        if name == "S1" and s1_centre is not None:
            c, r = s1_centre, s1_radius
        s.sphere(c, r, m)
    m = s.material(ha.DIFFUSE, 0.0)
    m.roughness.image = -1
    e = ha.Element()
    e.kind, e.material = ha.MESH, m
    verts, faces = np.ascontiguousarray(QUAD), np.ascontiguousarray(QUAD_FACES)
    e.vertexes = verts.ctypes.data_as(C.POINTER(ha.Vec3)); e.num_vertexes = verts.shape[0]
    e.faces = faces.ctypes.data_as(C.POINTER(C.c_uint64)); e.num_faces = faces.shape[0]
    s.keep += [verts, faces]
    s.elements.append(e)
    return s.finish((0.5, 1.0, 7.0), (0.0, 0.0, 0.0), cs.Y_UP, 30.0)


_made = {}


def scene(ha, orc, sky):
    """(scene, oracle scene): made once per process"""
    if sky not in _made:
        s = build_scene(ha, sky)
        _made[sky] = (s, orc.OracleScene(s.desc_ptr))
    return _made[sky]


# ------------------------------------------------------------------------------------------------------------------------------------------
# helpers
def _w(a):
    return np.asarray(a, dtype=F32).astype(np.float64)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _finite_rows(a):
    return np.isfinite(a).all(axis=1)


def _rays_to(origins, targets):
    """f64 rays from origins to targets: [n, 6]"""
    o, t = np.asarray(origins, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    return np.concatenate([o, _unit(t - o)], axis=1)


def _surface_set(name, rays64, with_fix=False, **extra):
    """rays: the f64 rays rounded to fp32; residual: what the rounding took away; with_fix: the rows that carry it in fp32 mode, as a path's first
    ray does (the others stand for themselves there).  Precise shading carries every ray as fp32 + residual: in precise mode every row has it."""
    rays64 = np.asarray(rays64, dtype=np.float64)
    hi = rays64.astype(F32)
    rng = np.random.default_rng(len(rays64) + 7)
    p = {"kind": "surface", "name": name, "rays": hi, "residual": (rays64 - hi.astype(np.float64)).astype(F32),
         "with_fix": np.broadcast_to(np.asarray(with_fix, dtype=bool), (len(hi),)).copy(), "draws": 0.05 + 0.9 * rng.random((len(hi), 2)),
         "uncapped": np.zeros(len(hi), bool), "must_be_solid": np.zeros(len(hi), bool)}
    p.update(extra)
    return p


# ------------------------------------------------------------------------------------------------------------------------------------------
# point sets: the sky
def _tie_xy(d):
    """|x| == |y| with z zero — or a denormal, the ulp neighbours of zero: the tie falls through to a Z face, whose quotients by z overflow the
    texel arithmetic (texture.rs:29-49 divides 0 by 0) — the reference is not finite there"""
    return (np.abs(d[:, 0]) == np.abs(d[:, 1])) & (np.abs(d[:, 2]) < 1.17549435e-38)


def gen_sky_seams():
    from test_corners_cpu import _sky_directions
    base = np.array(_sky_directions(), dtype=np.float64).astype(F32)
    out = [base]
    for j in range(3):                     # beside: every component by +-1 and +-2 fp32 ulps
        for k in (1, -1, 2, -2):
            m = base.copy()
            for _ in range(abs(k)):
                m[:, j] = np.nextafter(m[:, j], F32(np.inf if k > 0 else -np.inf))
            out.append(m)
    d = np.concatenate(out)
    d = np.concatenate([d, _unit(d.astype(np.float64)).astype(F32)])       # each also normalised, then rounded
    d = np.unique(d[_finite_rows(d)], axis=0)
    ties = _tie_xy(d)
    return {"kind": "sky", "name": "sky_seams", "dirs": d[~ties], "undefined": d[ties]}


_FACE_DIR = [lambda u, v: (1.0, v, -u), lambda u, v: (-1.0, v, u), lambda u, v: (u, 1.0, -v), lambda u, v: (u, -1.0, v), lambda u, v: (u, v, 1.0),
             lambda u, v: (-u, v, -1.0)]


def _texel_coords(n):
    """every interior k / n, rounded to fp32, and one fp32 ulp on either side — as 0-centred coordinates 2 U - 1 in (-1, 1)"""
    out = []
    for k in range(1, n):
        c = F32(2.0 * k / n - 1.0)
        out += [c, np.nextafter(c, F32(2)), np.nextafter(c, F32(-2))]
    return [float(c) for c in out]


def gen_sky_texels(sky):
    """Per face: u on every interior texel border k / w and an ulp beside it at three values of v (two that are nothing special, one border), and v
    on every k / h at three such values of u — a cross, not the product of the two sweeps (4,200 points per variant of its own); u or v exactly 0 and exactly 1 at two points per face, 0 and 1 taking turns (there
    the direction ties with the face's own axis: every such point is fragile, the seams set has the rest of them); 2,000 random directions."""
    rng = np.random.default_rng(301)
    dirs = []
    for f, (w, h) in enumerate(SKIES[sky]):
        us, vs = _texel_coords(w), _texel_coords(h)
        few_u, few_v = [-0.26, 0.55] + us[len(us) // 2:len(us) // 2 + 1], [0.31, -0.62] + vs[len(vs) // 2:len(vs) // 2 + 1]
        pts = [(u, v) for u in us for v in few_v] + [(u, v) for u in few_u for v in vs] + ([(-1.0, 0.31), (0.55, 1.0)] if f % 2 == 0 else [(1.0, -0.62), (-0.26, -1.0)])
        dirs += [_FACE_DIR[f](u, v) for u, v in pts]
    d = np.concatenate([np.array(dirs), _unit(rng.standard_normal((2000, 3)))]).astype(F32)
    d = np.unique(d, axis=0)
    return {"kind": "sky", "name": "sky_texels", "dirs": d[~_tie_xy(d)], "undefined": d[:0]}


# ------------------------------------------------------------------------------------------------------------------------------------------
# point sets: textures
SATURATING = [-2.0 ** -30, 1.0 + 2.0 ** -23, -3.0, 5e9, 1e10]


def _coords32(n):
    """test_corners_cpu._coords(n) rounded to fp32 (its 2^-40 neighbours become the value itself), with the fp32 ulp neighbours"""
    from test_corners_cpu import _coords
    out = set()
    for c in _coords(n):
        c = F32(c)
        out |= {float(c), float(np.nextafter(c, F32(2))), float(np.nextafter(c, F32(-2)))}
    return sorted(out)


def gen_texture(s):
    """Every image of the scene.  The small surface images (7 x 3, 1 x 5, 6 x 5: up to 35 texels) get the whole product _coords(w) x _coords(h), so
    that every pair with BOTH coordinates on a texel border is there; the larger ones (40 x 1, the sky faces) get every u at five values of v (0, 1,
    a border, one beside 0, one nothing special) and every v at five such values of u — a cross, not the product, which would be 10,000 points of its
    own.  Then the `as u32` saturation values in pairs and alone, and NaN."""
    image, uv = [], []
    for k, im in enumerate(s.arrays):
        h, w = im.shape[:2]
        us, vs = _coords32(w), _coords32(h)
        few_u, few_v = [0.0, 1.0, 0.37, us[len(us) // 2], -2.0 ** -30], [0.0, 1.0, 0.37, vs[len(vs) // 2], -2.0 ** -30]
        cross = [(u, v) for u in us for v in few_v] + [(u, v) for u in few_u for v in vs]
        pts = ([(u, v) for u in us for v in vs] if w * h <= 35 else cross) + [(u, v) for u in SATURATING for v in SATURATING]
        pts += [(u, 0.37) for u in SATURATING] + [(0.37, v) for v in SATURATING] + [(np.nan, 0.37), (0.37, np.nan), (np.nan, np.nan)]
        image += [k] * len(pts)
        uv += pts
    uv = np.array(uv, dtype=np.float64).astype(F32).astype(np.float64)
    return {"kind": "texture", "name": "texture", "image": np.array(image, dtype=np.int32), "uv": uv}


# ------------------------------------------------------------------------------------------------------------------------------------------
# point sets: surfaces
DELTAS = [0.0, 2.5e-5, 0.9e-4, 1.1e-4, 1e-3]          # from an edge; EPS = 1e-4 is the cascade's band
OBLIQUE = [np.array([0.0, 0.0]), np.array([0.41, 0.17]), np.array([-0.23, 0.52]), np.array([0.3, -0.45])]


def _face_frame(axis, side):
    n = np.zeros(3); n[axis] = 1.0 if side else -1.0
    a, b = [k for k in range(3) if k != axis]
    ta, tb = np.zeros(3), np.zeros(3)
    ta[a], tb[b] = 1.0, 1.0
    return n, ta, tb, a, b


def gen_cuboid_faces():
    rays, box_of, centre, edge = [], [], [], []
    for name, (lo, hi) in BOXES.items():
        mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)

        def add(origin, target, is_centre=False, is_edge=False):
            rays.append(_rays_to(origin[None], target[None])[0]); box_of.append(name); centre.append(is_centre); edge.append(is_edge)

        for axis in range(3):
            for side in (0, 1):
                n, ta, tb, a, b = _face_frame(axis, side)
                c = mid + n * half[axis]
                for ob in OBLIQUE:                                       # face centres: head on and along three oblique directions
                    add(c + 3.0 * (n + ob[0] * ta + ob[1] * tb), c, is_centre=True)
                add(mid + 0.1 * half * np.array([0.3, -0.2, 0.1]), c + 0.21 * half[a] * ta - 0.13 * half[b] * tb)      # from inside: the exit face
                # the four edges of this face, every one also approached on the adjoining face when its turn comes: 12 edges x 2 faces
                for t_ax, o_ax, tv, ov in ((a, b, ta, tb), (b, a, tb, ta)):
                    for o_side in (-1.0, 1.0):
                        for dlt in DELTAS:
                            p = c + 0.37 * half[t_ax] * tv + o_side * (half[o_ax] - dlt) * ov
                            add(p + 2.5 * (n + 0.2 * tv + 0.1 * o_side * ov), p, is_edge=True)
                        p = c + 0.37 * half[t_ax] * tv + o_side * (half[o_ax] - 1.1e-4) * ov
                        add(mid + 0.05 * half, p, is_edge=True)                                                        # the same edge from inside
        for sx in (-1.0, 1.0):                                           # the 8 corners, along the diagonal
            for sy in (-1.0, 1.0):
                for sz in (-1.0, 1.0):
                    sg = np.array([sx, sy, sz])
                    add(mid + sg * half + 2.0 * sg * np.array([1.0, 0.8, 0.9]), mid + sg * half, is_edge=True)
    box_of = np.array(box_of)
    return _surface_set("cuboid_faces", np.array(rays), box=box_of, must_be_solid=np.array(centre), edge=np.array(edge))


def gen_axis_rays():
    """One or two direction components exactly +0.0 / -0.0; the origin strictly off every slab plane (targets sit a little beside the centres)."""
    rays = []

    def add(target, axis, side):
        n, ta, tb, a, b = _face_frame(axis, side)
        for za in (0.0, -0.0):
            for zb in (0.0, -0.0):                       # two zeros
                d = -n.copy(); d[a], d[b] = za, zb
                rays.append(np.concatenate([target + 3.0 * n, d]))
            for sl in (0.3, -0.3):                       # one zero, on either tangential axis
                for zero_ax, free_ax in ((a, b), (b, a)):
                    d = -n.copy(); d[free_ax] = sl
                    d = _unit(d); d[zero_ax] = za
                    rays.append(np.concatenate([target - 3.0 * np.where(np.arange(3) == zero_ax, 0.0, d), d]))

    for lo, hi in (BOXES["A"], BOXES["C"]):
        mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        for axis in range(3):
            for side in (0, 1):
                n, ta, tb, a, b = _face_frame(axis, side)
                add(mid + n * half[axis] + 0.013 * ta - 0.007 * tb, axis, side)
    c, r = S2
    for axis in range(3):
        for side in (0, 1):
            n, ta, tb, a, b = _face_frame(axis, side)
            add(c + n * r * 0.98 + 0.113 * ta - 0.057 * tb, axis, side)
    return _surface_set("axis_rays", np.array(rays))


def _sphere_normal(theta, phi):
    """theta from +y, phi from +x towards +z (scene.rs:67-71: v = 1 - theta / pi, u = 0.5 - sign(n.z) acos(n.x / |n.xz|) / 2 pi)"""
    return np.array([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)])


def gen_sphere_uv():
    thetas = [0.0, 1e-6, 1e-3, 0.7, np.pi / 2, 2.1, np.pi - 1e-3, np.pi - 1e-6, np.pi]
    phis = [0.0, 1.0, np.pi / 2, np.pi - 1e-6, np.pi, -np.pi + 1e-6, -np.pi / 2, -2.0, -1e-6, 1e-6]
    rays, fix = [], []
    for c, r in SPHERES.values():
        for th in thetas:
            for ph in phis:
                n = _sphere_normal(th, ph)
                if ph == np.pi:
                    n[2] = 0.0 if th not in (0.0, np.pi) else n[2]          # the u seam itself: n.z = +0 at n.x < 0
                t = _unit(np.cross(n, [0.3, 0.5, -0.8]))
                for away in (n, _unit(n + 0.5 * t)):
                    for f in (False, True):
                        rays.append(_rays_to((c + r * n + 4.0 * away)[None], (c + r * n)[None])[0]); fix.append(f)
    return _surface_set("sphere_uv", np.array(rays), with_fix=np.array(fix))


GRAZING = [0.0, 0.5, 0.99, 0.9999, 1.0 - 1e-6, 1.0, 1.0 + 1e-6]


def gen_sphere_grazing():
    """impact parameter b / r from 0 to just past the silhouette, the origin 1, 10 and 1000 radii from the centre — on S1 and S2: at S3 one fp32 ulp of an
    origin coordinate (3e-5) is more than the 1e-5 between b / r = 0.9999 and the silhouette of an r = 0.1 sphere, a point that must not be fragile —;
    and the origin inside every sphere, where the reference misses (scene.rs:61-63: the near root only)."""
    rng = np.random.default_rng(302)
    rays, solid = [], []
    for name in ("S1", "S2"):
        c, r = SPHERES[name]
        for _ in range(8):
            d = _unit(rng.standard_normal(3))
            side = _unit(np.cross(d, rng.standard_normal(3)))
            for dist in (1.0, 10.0, 1000.0):
                for b in GRAZING:
                    rays.append(np.concatenate([c + b * r * side - (1.0 + dist) * r * d, d])); solid.append(b <= 0.9999)
    for c, r in SPHERES.values():
        for _ in range(8):
            rays.append(np.concatenate([c + 0.5 * r * _unit(rng.standard_normal(3)), _unit(rng.standard_normal(3))])); solid.append(False)
    return _surface_set("sphere_grazing", np.array(rays), must_be_solid=np.array(solid))


def gen_mesh_uv():
    rng = np.random.default_rng(303)
    targets = []
    for f in QUAD_FACES:
        v = QUAD[f.astype(int)]
        e = 1e-3       # edge midpoints and vertices a little INSIDE: on the outline a hit is a silhouette, on the diagonal either triangle's
        bary = [(1 / 3, 1 / 3), (0.6, 0.3), (0.1, 0.2), (0.05, 0.9), (0.45, 0.1)] + [(0.5 - e, 0.5 - e), (0.5, e), (e, 0.5)] + [(e, e), (1.0 - 3 * e, e), (e, 1.0 - 3 * e)]
        targets += [v[0] + a * (v[1] - v[0]) + b * (v[2] - v[0]) for a, b in bary]
    rays = []
    for t in targets:
        for _ in range(10):
            rays.append(_rays_to((t + np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(2.0, 5.0)]))[None], t[None])[0])
    return _surface_set("mesh_uv", np.array(rays))


def gen_general():
    """4,000 rays of test_gpu_parity._query_rays' kind: origins scattered round the eye, targets uniform over the box that holds everything near the
    origin; one ray in twenty towards the far cuboid B or the far sphere S3."""
    rng = np.random.default_rng(304)
    n = 4000
    org = np.array([0.5, 1.0, 7.0]) + rng.normal(size=(n, 3)) * 0.3
    tgt = rng.uniform(-1.0, 1.0, size=(n, 3)) * np.array([5.0, 2.0, 4.5]) + np.array([0.0, 1.0, -2.0])
    far = rng.random(n) < 0.05
    far_t = np.where((rng.random(n) < 0.5)[:, None], B_SHIFT + rng.uniform(-1.2, 1.2, size=(n, 3)), S3[0] + rng.uniform(-0.15, 0.15, size=(n, 3)))
    tgt = np.where(far[:, None], far_t, tgt)
    return _surface_set("general", _rays_to(org, tgt), with_fix=rng.random(n) < 0.5)


SURFACE_GENERATORS = {"cuboid_faces": gen_cuboid_faces, "axis_rays": gen_axis_rays, "sphere_uv": gen_sphere_uv, "sphere_grazing": gen_sphere_grazing,
                      "mesh_uv": gen_mesh_uv, "general": gen_general}
SURFACE_SETS = sorted(SURFACE_GENERATORS)
EDGE_SETS = ("cuboid_faces", "sphere_uv", "sphere_grazing")
SKY_SETS = ("sky_seams", "sky_texels")


# ------------------------------------------------------------------------------------------------------------------------------------------
# the oracle's answer and its sensitivity
# value columns of orc_intersect_material's record {hit, t, pos 3, n 3, u, v, surface, param, albedo 3, emission 3, roughness}
VALUE_COLS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17, 18]
POS_COLS, N_COLS, UV_COLS = [2, 3, 4], [5, 6, 7], [8, 9]


def cuboid_face_of(n):
    """pt_core.h cuboid_face_of on rows of normals"""
    f = np.full(len(n), 6)
    for code, (col, sign) in reversed(list(enumerate([(1, 1), (1, -1), (0, -1), (0, 1), (2, -1), (2, 1)]))):
        f = np.where(n[:, col] * sign > 0, code, f)
    return f


def _decisions(rec, elem):
    """[n, 3]: hit, element, cuboid face (-1: not a cuboid, or a miss)"""
    hit = rec[:, 0] != 0
    kind = np.where(hit, KIND[np.clip(elem, 0, len(KIND) - 1)], -1)
    face = np.where(kind == 2, cuboid_face_of(rec[:, N_COLS]), -1)
    return np.stack([hit.astype(int), np.where(hit, elem, -1), face], axis=1)


def _den(rec):
    den = np.maximum(1.0, np.abs(np.where(np.isfinite(rec), rec, 0.0)))
    den[:, POS_COLS] = np.maximum(1.0, np.sqrt((np.where(np.isfinite(rec[:, POS_COLS]), rec[:, POS_COLS], 0.0) ** 2).sum(-1)))[:, None]
    return den


def _oracle_surface(o, orc, rays64, draws, roughness=None):
    """(record [n, 19], decisions [n, 3], next ray [n, 7] = {origin, direction, some}) of the oracle on f64 rays.  The direction is normalised in
    f64 first: the reference's rays are unit vectors to f64 rounding and its sphere quadratic takes that for granted (scene.rs:58-66), an fp32
    direction is one to 6e-8 only and stands for the unit vector along it (sphere_root and shade_hit_f64 divide |d|^2 out) — the same line."""
    rays64 = np.concatenate([rays64[:, :3], _unit(rays64[:, 3:6])], axis=1)
    rec, elem = o.intersect_material_n(rays64)
    dec = _decisions(rec, elem)
    hit = dec[:, 0] != 0
    rough = rec[:, 18] if roughness is None else roughness
    safe = lambda a, fill: np.where(hit[:, None] if a.ndim == 2 else hit, np.where(np.isfinite(a), a, fill), fill)
    ms = orc.material_sample_n(np.where(hit, rec[:, 10], 0).astype(np.int32), safe(rec[:, 11], 0.0), safe(rough, 0.5), draws[:, 0], draws[:, 1],
                               safe(rec[:, POS_COLS], 0.0), -rays64[:, 3:6], safe(rec[:, N_COLS], 1.0))
    nxt = np.concatenate([ms[:, 1:7], ms[:, 0:1]], axis=1)
    nxt[~hit] = 0.0
    return rec, dec, nxt


def _moved(flip, rec2, rec, den, cols, kind_sphere):
    """what a moved evaluation adds: (flip or broken [n], change [n] over `cols`)"""
    wrap = kind_sphere & (np.abs(rec2[:, 8] - rec[:, 8]) > 0.5)
    broken = ~_finite_rows(rec2[:, VALUE_COLS]) & _finite_rows(rec[:, VALUE_COLS])
    bad = flip | wrap | broken
    return bad, np.where(bad, 0.0, measure(rec2[:, cols], rec[:, cols], den[:, cols]))


_cache = {}


def get_surface(ha, orc, name, precise=False):
    """The set, as the mode is given it, with the oracle's answer: the hit record, the next ray, sens, sens48, fragile.  Made once, left unchanged."""
    if (name, precise) in _cache:
        return _cache[(name, precise)]
    _, o = scene(ha, orc, "nonsquare")
    p = SURFACE_GENERATORS[name]()
    p["fix"] = np.where((p["with_fix"] | precise)[:, None], p["residual"], F32(0))
    if "box" in p and not precise:          # B's edge points in fp32 mode: an ulp of the origin there is larger than EPS — recorded, not capped
        p["uncapped"] = p["edge"] & (p["box"] == "B")
    hi, lo = p["rays"].astype(np.float64), p["fix"].astype(np.float64)
    rays64 = hi + lo
    rec, dec, nxt = _oracle_surface(o, orc, rays64, p["draws"])
    den = _den(rec)
    sphere = (dec[:, 0] != 0) & (KIND[np.clip(dec[:, 1], 0, 6)] == 1)
    n = len(rec)
    sens, sens48, sens48_next, fragile, fragile48 = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, bool), np.zeros(n, bool)
    den_next = np.concatenate([np.repeat(den[:, 2:3], 3, axis=1), np.ones((n, 3))], axis=1)
    for j in range(6):
        for toward in (np.inf, -np.inf):
            h2 = p["rays"].copy()
            h2[:, j] = np.nextafter(h2[:, j], F32(toward))
            r2, d2, _ = _oracle_surface(o, orc, h2.astype(np.float64) + lo, p["draws"])
            bad, s = _moved((d2 != dec).any(axis=1), r2, rec, den, VALUE_COLS, sphere)
            fragile |= bad
            sens = np.maximum(sens, s)
            m2 = rays64.copy()
            m2[:, j] *= 1.0 + (2.0 ** -48 if toward > 0 else -2.0 ** -48)
            r2, d2, n2 = _oracle_surface(o, orc, m2, p["draws"], rec[:, 18])
            bad, s = _moved((d2 != dec).any(axis=1) | (n2[:, 6] != nxt[:, 6]), r2, rec, den, N_COLS + UV_COLS, sphere)
            fragile48 |= bad
            sens48 = np.maximum(sens48, s)
            sens48_next = np.maximum(sens48_next, np.where(bad, 0.0, measure(n2[:, :6], nxt[:, :6], den_next)))
    p.update(ref=rec, decision=dec, next=nxt, den=den, den_next=den_next, sens=sens, sens48=sens48, sens48_next=sens48_next, fragile=fragile,
             fragile48=fragile48, sphere=sphere, rays64=rays64)
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[(name, precise)] = p
    return p


def surface_conditions(p):
    """what the oracle alone must meet on a surface set (the CPU tier asserts it): returns the figures"""
    n = len(p["ref"])
    capped = ~p["uncapped"]
    ok = _finite_rows(p["ref"][:, VALUE_COLS])
    fig = {"points": n, "hits": int((p["decision"][:, 0] != 0).sum()), "fragile": float(p["fragile"][capped].mean()),
           "fragile_uncapped": float(p["fragile"][~capped].mean()) if (~capped).any() else 0.0, "clause": float((K * p["sens"] > T)[ok & ~p["fragile"]].mean()),
           "oracle_not_finite": int((~ok).sum()), "compared": int((ok & ~p["fragile"]).sum())}
    name = p["name"]
    assert fig["fragile"] <= (MAX_FRAGILE_EDGE if name in EDGE_SETS else MAX_FRAGILE), (name, fig)
    assert not (p["fragile"] & p["must_be_solid"]).any(), (name, "a point that must not be fragile is", np.flatnonzero(p["fragile"] & p["must_be_solid"])[:8])
    assert (p["decision"][p["must_be_solid"], 0] != 0).all(), name
    assert fig["compared"] >= MIN_COMPARED, (name, fig)
    if name == "general":
        assert fig["clause"] <= MAX_CLAUSE, fig
    return fig


def device_record(out24):
    """hr_debug_surface's record in the oracle's layout [n, 19], and the face it reports"""
    o = np.asarray(out24, dtype=np.float64)
    return np.concatenate([o[:, 0:10], o[:, 11:20]], axis=1), o[:, 10].astype(int)


def check_surface(p, out24, out64, elem, label, precise):
    """Returns (figures, failures)."""
    got, face = device_record(out24)
    ref, den, dec, fragile = p["ref"], p["den"], p["decision"], p["fragile"] | (p["fragile48"] if precise else False)
    n = len(ref)
    hit = got[:, 0] != 0
    got_dec = np.stack([hit.astype(int), np.where(hit, elem, -1), np.where(hit, face, -1)], axis=1)
    with np.errstate(invalid="ignore"):
        wrap = p["sphere"] & hit & (np.abs(got[:, 8] - ref[:, 8]) > 0.5)
    mismatch = (got_dec != dec).any(axis=1) | wrap
    both_hit = hit & (dec[:, 0] != 0) & ~mismatch
    ref_ok = _finite_rows(ref[:, VALUE_COLS]) & (np.abs(np.where(np.isfinite(ref[:, VALUE_COLS]), ref[:, VALUE_COLS], 0.0)).max(axis=1) < BIG)
    compared = both_hit & ref_ok
    exact_bad = compared & (got[:, 10] != ref[:, 10])                                  # the surface type is the element's
    if not precise:
        err = measure(got[:, VALUE_COLS], ref[:, VALUE_COLS], den[:, VALUE_COLS])
        bound = np.maximum(T, K * p["sens"])
        parts = {"fp32": (err, bound)}
    else:
        cub = dec[:, 2] >= 0
        f64_cols_err = np.maximum(measure(got[:, N_COLS], ref[:, N_COLS], den[:, N_COLS]), np.where(cub, measure(got[:, UV_COLS], ref[:, UV_COLS], den[:, UV_COLS]), 0.0))
        rest = [c for c in VALUE_COLS if c not in N_COLS + UV_COLS]
        fp32_err = np.maximum(measure(got[:, rest], ref[:, rest], den[:, rest]), np.where(cub, 0.0, measure(got[:, UV_COLS], ref[:, UV_COLS], den[:, UV_COLS])))
        # the next ray, against the oracle's sample at the oracle's hit with the roughness the device reports
        nxt = p["next_for"](got[:, 18])
        some = np.asarray(out24)[:, 21] != 0
        # Some / None is a decision: the device's must be the oracle's own (with its own roughness) — and the one the reference below is made from
        next_mismatch = compared & ((some != (nxt[:, 6] != 0)) | (some != (p["next"][:, 6] != 0)))
        mismatch = mismatch | next_mismatch
        compared = compared & ~next_mismatch
        next_err = np.where(some, measure(np.asarray(out64, dtype=np.float64), nxt[:, :6], p["den_next"]), 0.0)
        parts = {"f64 once": (f64_cols_err, ULP32 + K * p["sens48"]), "fp32": (fp32_err, np.maximum(T, K * p["sens"])),
                 "next ray": (next_err, np.maximum(T64, K * p["sens48_next"]))}
    value_bad = np.zeros(n, bool)
    worst = {}
    for what, (e, b) in parts.items():
        value_bad |= compared & ~(e <= b)
        with np.errstate(invalid="ignore"):
            worst[what] = float(np.where(compared & np.isfinite(e), e / b, 0.0).max()) if compared.any() else 0.0
    not_finite = compared & ~_finite_rows(got[:, VALUE_COLS])
    hard = mismatch & ~fragile
    bad = value_bad | not_finite | hard | exact_bad
    e0, b0 = parts["fp32"]
    fig = {"label": label, "set": p["name"], "mode": "precise" if precise else "fp32", "points": n, "fragile": int(fragile.sum()), "compared": int(compared.sum()),
           "decisions_differ": int(mismatch.sum()), "worst_over_bound": worst, "worst_err": float(np.where(compared & np.isfinite(e0), e0, 0.0).max()) if compared.any() else 0.0,
           "above_T": float((compared & (e0 > T)).sum()) / max(1, int(compared.sum())), "oracle_not_finite": int((~ref_ok & (dec[:, 0] != 0)).sum()),
           "device_at_undefined_finite": int((_finite_rows(got[:, VALUE_COLS]) & ~ref_ok & (dec[:, 0] != 0)).sum()), "quads_differ": 0, "failures": int(bad.sum())}
    fails = []
    for i in np.flatnonzero(bad)[:10]:
        why = "not finite" if not_finite[i] else "decision" if hard[i] else "surface type" if exact_bad[i] else "value"
        detail = ", ".join("%s %.3g / %.3g" % (w, e[i], b[i]) for w, (e, b) in parts.items())
        fails.append("%s #%d (%s, %s): ray %s fix %s\n    got %s elem %d face %d\n    ref %s dec %s; %s; sens %.3g" % (
            p["name"], i, why, fig["mode"], p["rays"][i].tolist(), p["fix"][i].tolist(), np.round(got[i], 7).tolist(), elem[i], face[i], np.round(ref[i], 7).tolist(),
            dec[i].tolist(), detail, p["sens"][i]))
    return fig, fails


def run_surface(ha, orc, backend, name, precise, label):
    """backend: an object with debug_surface (an emulated scene, or a Renderer holding the scene)"""
    p = dict(get_surface(ha, orc, name, precise))
    _, o = scene(ha, orc, "nonsquare")
    p["next_for"] = lambda rough: _oracle_surface(o, orc, p["rays64"], p["draws"], rough)[2]
    out, out64, elem = backend.debug_surface(p["rays"], p["fix"], p["draws"], precise)
    fig, fails = check_surface(p, out, out64, elem, label, precise)
    print(report_line(fig))
    return fig, fails, (out, out64, elem)


# ------------------------------------------------------------------------------------------------------------------------------------------
# sky and textures
def get_sky(ha, orc, sky, name):
    key = (sky, name)
    if key in _cache:
        return _cache[key]
    _, o = scene(ha, orc, sky)
    p = gen_sky_seams() if name == "sky_seams" else gen_sky_texels(sky)
    d = p["dirs"]
    ref, where = o.skybox_n(_w(d))
    sens, fragile, quad_fragile = np.zeros(len(d)), np.zeros(len(d), bool), np.zeros(len(d), bool)
    for j in range(3):
        for toward in (np.inf, -np.inf):
            m = d.copy()
            m[:, j] = np.nextafter(m[:, j], F32(toward))
            r2, w2 = o.skybox_n(_w(m))
            bad = (w2[:, 0] != where[:, 0]) | (~_finite_rows(r2) & _finite_rows(ref))
            fragile |= bad
            quad_fragile |= (w2 != where).any(axis=1)
            sens = np.maximum(sens, np.where(bad, 0.0, measure(r2, ref, np.maximum(1.0, np.abs(np.where(np.isfinite(ref), ref, 0.0))))))
    p.update(sky=sky, ref=ref, where=where, sens=sens, fragile=fragile, quad_fragile=quad_fragile, undefined_ref=o.skybox_n(_w(p["undefined"]))[0] if len(p["undefined"]) else np.zeros((0, 3)))
    _cache[key] = p
    return p


def sky_conditions(p):
    fig = {"points": len(p["dirs"]), "fragile": float(p["fragile"].mean()), "faces": sorted(set(p["where"][:, 0].tolist())),
           "oracle_not_finite": int((~_finite_rows(p["ref"])).sum()), "undefined": len(p["undefined"])}
    assert fig["faces"] == list(range(6)) and fig["points"] - fig["oracle_not_finite"] >= MIN_COMPARED, fig
    assert fig["oracle_not_finite"] == 0, fig
    assert not np.isfinite(p["undefined_ref"]).all(axis=1).any(), "the oracle is finite on an x == y, z == 0 tie"
    if p["name"] == "sky_texels":
        assert fig["fragile"] <= MAX_FRAGILE, fig
    return fig


def check_sky(p, rgb, where, label):
    ref = p["ref"]
    n = len(ref)
    got = np.asarray(rgb, dtype=np.float64)
    face_bad = (np.asarray(where)[:, 0] & 7) != p["where"][:, 0]                     # never excused
    form_bad = (np.asarray(where)[:, 0] >> 3) != EXPECTED_FORM[p["sky"]]
    den = np.maximum(1.0, np.abs(ref))
    err = measure(got, ref, den)
    bound = np.maximum(T, K * p["sens"])
    compared = ~face_bad & _finite_rows(ref)
    value_bad = compared & ~(err <= bound)
    quads = compared & (np.asarray(where)[:, 1:3] != p["where"][:, 1:3]).any(axis=1)
    bad = face_bad | form_bad | value_bad
    e = np.where(compared & np.isfinite(err), err, 0.0)
    fig = {"label": label, "set": "%s/%s" % (p["name"], p["sky"]), "mode": "fp32", "points": n, "fragile": int(p["fragile"].sum()), "compared": int(compared.sum()),
           "decisions_differ": int(face_bad.sum()), "quads_differ": int(quads.sum()), "worst_err": float(e.max()), "above_T": float((e > T).mean()),
           "worst_over_bound": {"fp32": float((e / bound).max())}, "failures": int(bad.sum())}
    fails = ["%s #%d: dir %s got %s where %s, ref %s where %s, err %.3g bound %.3g" % (fig["set"], i, p["dirs"][i].tolist(), got[i].tolist(), np.asarray(where)[i].tolist(),
                                                                                       ref[i].tolist(), p["where"][i].tolist(), err[i], bound[i]) for i in np.flatnonzero(bad)[:10]]
    return fig, fails


def get_texture(ha, orc, sky):
    key = (sky, "texture")
    if key in _cache:
        return _cache[key]
    s, o = scene(ha, orc, sky)
    p = gen_texture(s)
    im, uv = p["image"], p["uv"]
    ok_in = _finite_rows(uv)
    q = np.where(ok_in[:, None], uv, 0.37)
    ref, quad = o.image_bilinear_n(im, q)
    ref[~ok_in] = np.nan
    sens, fragile, quad_fragile = np.zeros(len(uv)), np.zeros(len(uv), bool), ~ok_in
    den = np.maximum(1.0, np.abs(np.where(np.isfinite(ref), ref, 0.0)))
    for j in range(2):
        for toward in (np.inf, -np.inf):
            m = q.astype(F32)
            m[:, j] = np.nextafter(m[:, j], F32(toward))
            r2, q2 = o.image_bilinear_n(im, m.astype(np.float64))
            quad_fragile |= (q2 != quad).any(axis=1)
            sens = np.maximum(sens, np.where(ok_in, measure(r2, np.where(ok_in[:, None], ref, 0.0), den), 0.0))
    p.update(sky=sky, ref=ref, quad=quad, sens=sens, fragile=fragile, quad_fragile=quad_fragile, den=den, nan=~ok_in)
    _cache[key] = p
    return p


def texture_conditions(p):
    fig = {"points": len(p["uv"]), "nan_inputs": int(p["nan"].sum()), "fragile": float(p["fragile"].mean()), "images": len(set(p["image"].tolist()))}
    assert fig["points"] - fig["nan_inputs"] >= MIN_COMPARED and fig["fragile"] <= MAX_FRAGILE, fig
    assert not np.isfinite(p["ref"][p["nan"]]).any()
    return fig


def check_texture(p, rgb, rough64, quad, label):
    ref, den, nan = p["ref"], p["den"], p["nan"]
    got, r64 = np.asarray(rgb, dtype=np.float64), np.asarray(rough64, dtype=np.float64)
    err = measure(got, np.where(nan[:, None], 0.0, ref), den)
    bound = np.maximum(T, K * p["sens"])
    err64 = measure(r64[:, None], np.where(nan, 0.0, ref[:, 0])[:, None], den[:, :1])
    value_bad = ~nan & (~(err <= bound) | ~(err64 <= T))
    nan_bad = nan & (np.isfinite(got).all(axis=1) | np.isfinite(r64))            # a NaN coordinate: non-finite on both sides
    quad = np.asarray(quad)
    quads = ~nan & (quad[:, :2] != p["quad"]).any(axis=1)
    corner64_bad = ~nan & (quad[:, 2:4] != p["quad"]).any(axis=1)       # the f64 read's corner: a floor in f64 of the oracle's own product
    bad = value_bad | nan_bad | corner64_bad
    e = np.where(~nan & np.isfinite(err), err, 0.0)
    fig = {"label": label, "set": "texture/%s" % p["sky"], "mode": "fp32 + f64 read", "points": len(ref), "fragile": 0, "compared": int((~nan).sum()), "decisions_differ": 0,
           "quads_differ": int(quads.sum()), "worst_err": float(e.max()), "above_T": float((e > T).mean()),
           "worst_over_bound": {"fp32": float((e / bound).max()), "f64 read": float(np.where(~nan & np.isfinite(err64), err64, 0.0).max() / T)},
           "f64_corners_differ": int(corner64_bad.sum()), "failures": int(bad.sum())}
    fails = ["%s #%d: image %d uv %s got %s rough64 %.9g quad %s, ref %s quad %s, err %.3g bound %.3g, f64 read err %.3g" % (
        fig["set"], i, p["image"][i], p["uv"][i].tolist(), got[i].tolist(), r64[i], np.asarray(quad)[i].tolist(), ref[i].tolist(), p["quad"][i].tolist(), err[i],
        bound[i], err64[i]) for i in np.flatnonzero(bad)[:10]]
    return fig, fails


def same_where(p, got, emulated, what):
    """The device's face / texel-quad corner against the emulation's: equal except where a move of an input to its fp32 neighbour changes the
    oracle's own (the device divides with v_rcp_f32, the host with a division: an ulp of the coordinate)."""
    differ = (np.asarray(got) != np.asarray(emulated)).any(axis=1)
    hard = differ & ~p["quad_fragile"]
    if np.asarray(got).shape[1] == 4:        # the texture query: its f64 corner is the emulation's everywhere (one f64 product, one floor)
        hard |= (np.asarray(got)[:, 2:4] != np.asarray(emulated)[:, 2:4]).any(axis=1) & ~p["nan"]
    print("lookups %s: %d of %d corners differ from the emulation's, %d of them where the oracle's own corner is not fragile" % (what, differ.sum(), len(differ), hard.sum()))
    assert not hard.any(), (what, np.flatnonzero(hard)[:8], np.asarray(got)[hard][:8], np.asarray(emulated)[hard][:8])


def report_line(fig):
    return ("lookups %(set)s [%(label)s, %(mode)s]: %(points)d points, %(fragile)d fragile, %(compared)d compared, decisions differ %(decisions_differ)d, "
            "quads differ %(quads_differ)d, worst error %(worst_err).3g, share above T %(above_T).4f, worst err / bound %(worst_over_bound)s, failures %(failures)d" % fig)
