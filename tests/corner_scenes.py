"""Corner scenes: small scenes in which a corner of the texture, sky and glass code is the COMMON case, for a path-by-path comparison with the
f64 oracle (tests/path_parity.py).  Every other synthetic scene of the suite borrows the three square power-of-two images and the six 16 x 16
sky faces of `cornell_mini`; here every scene brings its own images and its own skybox:

  sky_nonsquare   six 12 x 5 faces (Scene::sky_quads with w != h: flatten.cpp's footprint table, pt_core.h sky_sample), no visible geometry
  sky_mixed       faces of six different sizes, 1 x 1, N x 1, 1 x N and 5 x 7 among them (no footprint table: sample_bilinear on sky_image[face],
                  and the log helper plog_sky's other branch), a Specular cuboid in front of the camera
  cuboid_edges    one cuboid whose albedo, emission and roughness come from a 7 x 3, a 1 x 5 and a 40 x 1 image; the whole silhouette in the frame
  sphere_poles    three spheres of radius 1 (Diffuse, GGX, GGXRefraction), everything imaged (the roughness from a 6 x 5 map); views onto the
                  poles and the -x seam of scene.rs:67-71
  inside_glass    the camera inside a Refraction / GGXRefraction cuboid or a closed glass mesh: primary hits beyond the critical angle

Image content: green ramps by >= 4/255 per texel in x, blue in y, red along the diagonal (in x AND in y: roughness reads .x), and every image
of a scene (every sky face) starts from other offsets — a lookup displaced by a texel, taken from another face or image moves a channel by
~1e-2 after the 2.2 gamma (every value is >= 96/255, where the gamma curve's slope is >= 0.68), a coordinate error of 1e-2 texel stays
below 1e-3.  No value wraps around: bilinear interpolation of a ramp is continuous across texel-quad borders.

Cameras are pinholes (lens radius 0).  Views are aimed a little beside the symmetric direction their name says: with the symmetric aim a
column of sub-samples lies EXACTLY in a seam plane (|x| == |z|, n.z == 0), where the strict comparisons of scene.rs:300-318 resolve a tie
that any rounding breaks — the reference is discontinuous on ~1 % of such a frame's paths, ten times what `nudge_count` allows.  (The oracle's
exact ties are pinned direction by direction in tests/test_corners_cpu.py.)

No GPU in this module: tests/test_corners_cpu.py runs the cases through the emulation, tests/test_corners_gpu.py on the device."""
import ctypes as C

import numpy as np

W, H = 64, 48
NUDGE = 2.0 ** -22


# ------------------------------------------------------------------------------------------ images

def ramp_image(w, h, off_r, off_g, off_b):
    """RGBA8 (h, w, 4), row 0 = top.  red = off_r + step (x + y): it ramps in BOTH directions (roughness reads .x, and a roughness map must notice
    a wrong u as well as a wrong v); green = off_g + step x; blue = off_b + step y.  step = 4 where the image is long, up to 12 where it is short;
    every value in 96 .. 255, nothing wraps."""
    def ramp(n, off):
        assert 96 <= off <= 255
        step = 4 if n <= 1 else max(4, min(12, (255 - off) // (n - 1)))
        v = off + step * np.arange(n)
        assert v.max() <= 255, (n, off)
        return v
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    im = np.empty((h, w, 4), dtype=np.uint8)
    im[..., 0] = ramp(w + h - 1, off_r)[x + y]
    im[..., 1] = ramp(w, off_g)[x]
    im[..., 2] = ramp(h, off_b)[y]
    im[..., 3] = 255
    return np.ascontiguousarray(im)


SKY_NONSQUARE = [(12, 5)] * 6
SKY_MIXED = [(1, 1), (9, 1), (1, 6), (5, 7), (4, 4), (3, 2)]            # +x, -x, +y, -y, +z, -z
SURFACE_IMAGES = [(7, 3), (1, 5), (40, 1), (6, 5)]                       # albedo, emission, roughness, and a roughness map with two dimensions for the spheres


def sky_images(shapes):
    """six faces, every one from offsets of its own"""
    return [ramp_image(w, h, 100 + 11 * f, 170 - 13 * f, 120 + 7 * f) for f, (w, h) in enumerate(shapes)]


def surface_images():
    return [ramp_image(7, 3, 120, 150, 100), ramp_image(1, 5, 96, 110, 130), ramp_image(40, 1, 98, 97, 140), ramp_image(6, 5, 130, 105, 115)]


# ------------------------------------------------------------------------------------------ scene descriptions

class Scene:
    """An hr_scene_desc with its own images, skybox, elements and camera; .desc_ptr is what Renderer.upload_scene, EmuScene and OracleScene take."""

    def __init__(self, ha, sky_shapes, with_surface_images=True):
        self.ha = ha
        self.arrays = sky_images(sky_shapes) + (surface_images() if with_surface_images else [])
        self.img = (ha.Image * len(self.arrays))()
        for k, a in enumerate(self.arrays):
            self.img[k].rgba = a.ctypes.data_as(C.POINTER(C.c_uint8))
            self.img[k].width, self.img[k].height = a.shape[1], a.shape[0]
        self.elements = []
        self.keep = []
        self.desc = ha.SceneDesc()
        self.desc.images = C.cast(self.img, C.POINTER(ha.Image))
        self.desc.num_images = len(self.arrays)
        for f in range(6):
            self.desc.skybox.face_image[f] = f
        self.desc.skybox.intensity = ha.Vec3(1.0, 0.9, 0.8)
        self.desc_ptr = C.pointer(self.desc)
        self.w, self.h = W, H

    ALBEDO, EMISSION, ROUGHNESS, ROUGHNESS_2D = 6, 7, 8, 9          # image indices of surface_images()

    def material(self, surface, param, albedo=(0.9, 0.9, 0.9), emission=(0.0, 0.0, 0.0), roughness=0.6, imaged=True):
        ha = self.ha
        m = ha.Material()
        m.surface, m.param = int(surface), float(param)
        m.albedo.color, m.albedo.image = ha.Vec3(*albedo), self.ALBEDO if imaged else -1
        m.emission.color, m.emission.image = ha.Vec3(*emission), self.EMISSION if imaged and any(emission) else -1
        m.roughness.color, m.roughness.image = ha.Vec3(roughness, roughness, roughness), self.ROUGHNESS if imaged else -1
        return m

    def sphere(self, center, radius, material):
        e = self.ha.Element()
        e.kind, e.center, e.radius, e.material = self.ha.SPHERE, self.ha.Vec3(*center), float(radius), material
        self.elements.append(e)

    def cuboid(self, lo, hi, material):
        e = self.ha.Element()
        e.kind, e.aabb_min, e.aabb_max, e.material = self.ha.CUBOID, self.ha.Vec3(*lo), self.ha.Vec3(*hi), material
        self.elements.append(e)

    def octahedron(self, center, size, material):
        """the closed mesh of tests/random_scenes.py, axis-aligned"""
        octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
        verts = np.ascontiguousarray(octa * size + np.asarray(center, dtype=np.float64))
        faces = np.ascontiguousarray(np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.uint64))
        e = self.ha.Element()
        e.kind, e.material = self.ha.MESH, material
        e.vertexes = verts.ctypes.data_as(C.POINTER(self.ha.Vec3)); e.num_vertexes = verts.shape[0]
        e.faces = faces.ctypes.data_as(C.POINTER(C.c_uint64)); e.num_faces = faces.shape[0]
        self.keep += [verts, faces]
        self.elements.append(e)

    def finish(self, eye, target, up, fov, nudge=False, size=None):
        """Camera::new (camera.rs:45-64) through hh_camera_new: pinhole.  nudge: the eye displaced by 2^-22 of its distance to the target in
        each coordinate — about four fp32 roundings of an O(1) coordinate —, the target kept."""
        ha = self.ha
        eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
        if nudge:
            eye = eye + NUDGE * np.linalg.norm(target - eye)
        self.el = (ha.Element * len(self.elements))(*self.elements)
        self.desc.elements = C.cast(self.el, C.POINTER(ha.Element))
        self.desc.num_elements = len(self.elements)
        ha.host_lib().hh_camera_new(ha.Vec3(*eye), ha.Vec3(*target), ha.Vec3(*up), float(fov), 0, 0.0, 5.0, C.byref(self.desc.camera))
        if size:
            self.w, self.h = size
        return self


Y_UP, X_UP = (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)
AIM = np.array([0.0137, -0.0071, 0.0043])            # what every view is aimed beside its symmetric direction by (see the module's header)

# eye at the origin; (target, v_fov — the half angle, camera.rs:48 —): the corner views see three faces and their three seams, the edge views
# two faces and the seam between them, +x the whole +x face and a strip of its four neighbours (tan 50 deg = 1.19 > 1)
SKY_VIEWS = {
    "corner_ppp": ((1.0, 1.0, 1.0), 24.0),
    "corner_nnn": ((-1.0, -1.0, -1.0), 24.0),
    "edge_x_z": ((1.0, 0.0, 1.0), 24.0),
    "edge_ny_z": ((0.0, -1.0, 1.0), 24.0),
    "face_px": ((1.0, 0.0, 0.0), 50.0),
}


def sky_nonsquare(ha, view, nudge=False):
    s = Scene(ha, SKY_NONSQUARE, with_surface_images=False)
    target, fov = SKY_VIEWS[view]
    target = np.asarray(target) + AIM
    # hr_upload_scene refuses an empty element list: a small diffuse sphere parked behind the camera
    s.sphere(-4.0 * target / np.linalg.norm(target), 0.25, s.material(ha.DIFFUSE, 0.0, imaged=False))
    return s.finish((0.0, 0.0, 0.0), target, Y_UP, fov, nudge)


def sky_mixed(ha, view, nudge=False):
    s = Scene(ha, SKY_MIXED, with_surface_images=False)
    target, fov = SKY_VIEWS[view]
    target = np.asarray(target) + AIM
    c = 3.0 * target / np.linalg.norm(target)
    s.cuboid(c - np.array([0.45, 0.35, 0.4]), c + np.array([0.45, 0.35, 0.4]), s.material(ha.SPECULAR, 0.0, albedo=(0.95, 0.9, 0.85), imaged=False))
    return s.finish((0.0, 0.0, 0.0), target, Y_UP, fov, nudge)


CUBOID_VIEWS = {"ppp": (4.0, 3.0, 5.0), "nnn": (-4.0, -3.0, -5.0)}


def cuboid_edges(ha, view, surface="ggx", nudge=False):
    s = Scene(ha, SKY_NONSQUARE)
    surf, param = (ha.GGX, 0.8) if surface == "ggx" else (ha.DIFFUSE, 0.0)
    s.cuboid((-1.0, -0.6, -0.8), (1.0, 0.6, 0.8), s.material(surf, param, emission=(0.8, 0.7, 0.9)))
    return s.finish(np.asarray(CUBOID_VIEWS[view]) + AIM, (0.0, 0.0, 0.0), Y_UP, 15.0, nudge)


# the spheres stand side by side along z, each a little off the symmetric place; the pole views look along y with x up (z runs across the frame)
SPHERE_Z = (-2.4 + 0.0171, 0.0093, 2.4 - 0.0127)
SPHERE_VIEWS = {
    "north": ((0.011, 7.0, 0.007), X_UP, 26.0),
    "south": ((-0.009, -7.0, 0.013), X_UP, 26.0),
    "seam": ((-7.0, 0.006, 0.004), Y_UP, 26.0),
}


def _three_spheres(s):
    ha = s.ha
    for z, (surf, param) in zip(SPHERE_Z, ((ha.DIFFUSE, 0.0), (ha.GGX, 0.8), (ha.GGX_REFRACTION, 1.5))):
        m = s.material(surf, param, emission=(0.5, 0.6, 0.4))
        m.roughness.image = s.ROUGHNESS_2D           # (a 40 x 1 map would not notice a wrong v)
        s.sphere((0.0, 0.0, z), 1.0, m)


def sphere_poles(ha, view, nudge=False):
    s = Scene(ha, SKY_NONSQUARE)
    _three_spheres(s)
    eye, up, fov = SPHERE_VIEWS[view]
    return s.finish(eye, (0.0, 0.0, 0.0), up, fov, nudge)


def sphere_pole_exact(ha, south=False):
    """2 x 2 pixels aimed EXACTLY at a pole of the middle sphere: the sub-sample (1, 1, sx 1, sy 1) is the frame's centre (nc = 0, 0), its ray
    hits the pole, where scene.rs:69-70 divides 0 by 0."""
    s = Scene(ha, SKY_NONSQUARE)
    _three_spheres(s)
    y = -7.0 if south else 7.0
    return s.finish((0.0, y, SPHERE_Z[1]), (0.0, 0.0, SPHERE_Z[1]), X_UP, 2.0, size=(2, 2))


GLASS_VIEWS = ("refraction", "ggx_refraction", "mesh")


def inside_glass(ha, view, nudge=False):
    """The eye inside glass (ior 1.5, critical angle 41.8 deg) with a 50 deg half angle of view; outside an imaged diffuse floor and the mixed
    skybox."""
    s = Scene(ha, SKY_MIXED)
    s.cuboid((-6.0, -3.0, -6.0), (6.0, -2.0, 6.0), s.material(ha.DIFFUSE, 0.0))
    if view == "mesh":
        s.octahedron((0.0, 0.0, 0.0), 1.5, s.material(ha.REFRACTION, 1.5, albedo=(0.95, 0.97, 0.9), imaged=False))
        return s.finish((0.11, 0.07, -0.05), (0.06, -0.09, -1.5), Y_UP, 22.0, nudge)      # towards a vertex, whose four faces are seen at 55 deg; narrower: the rays beyond the critical angle are the ones near the axis
    if view == "refraction":
        m = s.material(ha.REFRACTION, 1.5, albedo=(0.95, 0.97, 0.9), imaged=False)
    else:
        m = s.material(ha.GGX_REFRACTION, 1.5, albedo=(0.95, 0.97, 0.9), roughness=0.5, imaged=False)
        m.roughness.image = s.ROUGHNESS
    s.cuboid((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), m)
    return s.finish((0.13, 0.06, 0.21), (0.45, -0.3, -1.0), Y_UP, 50.0, nudge)


def inside_glass_sphere(ha):
    """The reference never hits a sphere from inside (scene.rs:61-63: the near root only): a camera inside a glass sphere sees through it."""
    s = Scene(ha, SKY_MIXED, with_surface_images=False)
    s.sphere((0.0, 0.0, 0.0), 1.0, s.material(ha.REFRACTION, 1.5, imaged=False))
    return s.finish((0.1, 0.05, 0.2), (0.4, -0.3, -1.0), Y_UP, 40.0, size=(16, 12))


# ------------------------------------------------------------------------------------------ the cases and their limits

SKY, GLASS, SOLID = "sky", "glass", "solid"
# what a divergent path may be, by scene (path_parity.account's divergent_by_class_ppm):
#   sky     another cube-map face at a seam
#   glass   the Fresnel coin / total internal reflection deciding the other way, and a hit at the box's own edge: another face (same events),
#           which may leave the glass where the oracle stays inside (hit_vs_miss further on)
#   solid   the silhouette, and another cuboid face at an edge
ALLOWED = {
    SKY: {"other_element_same_events"},
    GLASS: {"reflect_vs_transmit", "other_element_same_events", "hit_vs_miss"},
    SOLID: {"hit_vs_miss", "other_element_same_events"},
}

CASES = {}
for _v in SKY_VIEWS:
    CASES["sky_nonsquare-" + _v] = (SKY, lambda ha, nudge=False, v=_v: sky_nonsquare(ha, v, nudge))
for _v in SKY_VIEWS:
    CASES["sky_mixed-" + _v] = (SKY, lambda ha, nudge=False, v=_v: sky_mixed(ha, v, nudge))
for _s in ("ggx", "diffuse"):
    for _v in CUBOID_VIEWS:
        CASES["cuboid_edges-%s-%s" % (_s, _v)] = (SOLID, lambda ha, nudge=False, v=_v, s=_s: cuboid_edges(ha, v, s, nudge))
for _v in SPHERE_VIEWS:
    CASES["sphere_poles-" + _v] = (SOLID, lambda ha, nudge=False, v=_v: sphere_poles(ha, v, nudge))
for _v in GLASS_VIEWS:
    CASES["inside_glass-" + _v] = (GLASS, lambda ha, nudge=False, v=_v: inside_glass(ha, v, nudge))

SAME_MAX = 1e-3          # the project's bound for scenes without small spheres (tests/test_gpu_parity.py PATH_LIMITS rtcamp6_v3_1 / cornell_mini)
MAX_NUDGE_SHARE = 1e-3   # a view whose reference is discontinuous on more than 0.1 % of its paths is re-aimed, not given a larger cap

# How discontinuous the REFERENCE is, measured on the oracle alone (nudge_count below; profiles/corner_scenes.txt holds these figures, the caps
# and what the emulation and the device measured): paths of sampling 1 whose events, hash or radiance (beyond 1e-3) change when the eye moves
# by 2^-22 of its distance to the target.  cap = 3 x the count (the kernel rounds several times per decision where the nudge is one
# perturbation), never below 3 paths (one path of a 64 x 48 frame is 81 ppm).  `same_max`: the bound on the worst same-branch path — 1e-3, or,
# where the issue allows a measured one (the seam view, paths that refract twice), max(1e-3, 3 x the worst radiance change between the two oracle
# runs among the paths that kept their branch).
#   case: (nudge count, worst same-branch change between the two oracle runs)
NUDGE_MEASURED = {
    "sky_nonsquare-corner_ppp": (0, 4.3e-9),
    "sky_nonsquare-corner_nnn": (0, 2.0e-9),
    "sky_nonsquare-edge_x_z": (0, 2.1e-7),
    "sky_nonsquare-edge_ny_z": (0, 5.4e-7),
    "sky_nonsquare-face_px": (0, 4.4e-7),
    "sky_mixed-corner_ppp": (0, 9.5e-9),
    "sky_mixed-corner_nnn": (0, 5.1e-9),
    "sky_mixed-edge_x_z": (0, 1.8e-7),
    "sky_mixed-edge_ny_z": (0, 1.7e-6),
    "sky_mixed-face_px": (0, 1.1e-6),
    "cuboid_edges-ggx-ppp": (0, 7.8e-7),
    "cuboid_edges-ggx-nnn": (0, 9.5e-7),
    "cuboid_edges-diffuse-ppp": (0, 7.8e-7),
    "cuboid_edges-diffuse-nnn": (0, 8.6e-7),
    "sphere_poles-north": (0, 1.6e-5),
    "sphere_poles-south": (0, 1.2e-5),
    "sphere_poles-seam": (0, 9.7e-6),
    "inside_glass-refraction": (1, 3.2e-6),
    "inside_glass-ggx_refraction": (0, 3.5e-4),
    "inside_glass-mesh": (0, 4.3e-6),
}
MEASURED_SAME_MAX = ("sphere_poles-seam", "inside_glass-refraction", "inside_glass-ggx_refraction", "inside_glass-mesh")


def limits(name):
    """(cap on divergent paths + same-branch paths beyond 1e-3, bound on the worst same-branch path)"""
    count, worst = NUDGE_MEASURED[name]
    same_max = max(SAME_MAX, 3.0 * worst) if name in MEASURED_SAME_MAX else SAME_MAX
    return max(3, 3 * count), same_max


def nudge_count(ha, orc, name):
    """(paths that change, worst radiance change among those that kept their branch, paths) between the oracle on the case as built and on
    the case with the eye nudged"""
    import path_parity
    _, build = CASES[name]
    a, b = build(ha), build(ha, True)
    la = orc.OracleScene(a.desc_ptr).path_log(a.w, a.h, 1)
    lb = orc.OracleScene(b.desc_ptr).path_log(b.w, b.h, 1)
    acc = path_parity.account(lb, la)
    n = acc["paths"]
    over = int(round(acc["same_branch"]["over_1e-3_floor1_ppm"] * n / 1e6))
    return acc["divergent"] + over, acc["same_branch"]["max_rel_floor1"], n


_made = {}


def get(ha, orc, name):
    """(scene, oracle path log of sampling 1): made once per process and not changed afterwards"""
    if name not in _made:
        s = CASES[name][1](ha)
        _made[name] = (s, orc.OracleScene(s.desc_ptr).path_log(s.w, s.h, 1))
    return _made[name]


def check(name, got, ref, what):
    """What every path-by-path case asserts (both tiers): equal ray counts on same-branch paths; no same-branch path beyond the bound; divergent
    paths (and, where the bound is a measured one, same-branch paths beyond 1e-3) within the cap and of the classes the corner predicts; the
    worst path that interpolated between other texels within 1e-3 (a ramp is continuous across quad borders, a wrong clamp is not)."""
    cap, same_max = limits(name)
    return check_against(name, ALLOWED[CASES[name][0]], cap, same_max, got, ref, what)


def check_against(name, allowed, cap, same_max, got, ref, what):
    """check() with the limits handed in: tests/light_material_scenes.py asserts the same things of its own cases"""
    import path_parity
    a = path_parity.account(got, ref)
    sb = a["same_branch"]
    n = a["paths"]
    over = int(round(sb["over_1e-3_floor1_ppm"] * n / 1e6))
    oq = sb["other_texel_quad"]
    print("corner %s [%s]: %d paths, divergent %d %s, same-branch beyond 1e-3: %d, worst %.3g (bound %.3g), cap %d; other texel quad %.0f ppm, worst %.3g" % (
        name, what, n, a["divergent"], a["divergent_by_class_ppm"], over, sb["max_rel_floor1"], same_max, cap, oq["ppm"], oq["max_rel_floor1"]))
    assert np.isfinite(got[0]).all() and np.isfinite(ref[0]).all(), (name, what)
    assert sb["rays_equal"], (name, what)
    assert sb["max_rel_floor1"] <= same_max, (name, what, sb)
    assert a["divergent"] + over <= cap, (name, what, a)
    assert set(a["divergent_by_class_ppm"]) <= allowed, (name, what, a["divergent_by_class_ppm"])
    assert oq["max_rel_floor1"] <= SAME_MAX, (name, what, oq)
    return a


def check_pole_frame(got, ref, pole):
    """sphere_pole_exact's 16 paths: the one onto the pole is a GGX hit with a finite, positive radiance (the oracle's ends with nothing: see
    tests/test_corners_cpu.py), the others took the oracle's branches and are within 1e-3"""
    assert np.isfinite(got[0]).all()
    assert int(got[2][pole][0]) & 7 == 5 and got[0][pole].min() > 0.0, (got[2][pole], got[0][pole])
    others = np.ones(ref[1].shape, dtype=bool)
    others[pole] = False
    assert np.array_equal(got[2][others][:, :10], ref[2][others][:, :10]) and np.array_equal(got[3][others], ref[3][others])
    assert np.array_equal(got[1][others], ref[1][others])
    rel = np.abs(got[0].astype(np.float64) - ref[0]) / np.maximum(1.0, np.abs(ref[0]))
    assert rel[others].max() <= SAME_MAX, rel[others].max()


def check_whole_frame(got, ref):
    """a tiny frame without an fp32-fragile decision: every path took the oracle's branches, traced its rays and is within 1e-3"""
    assert np.array_equal(got[2][..., :10], ref[2][..., :10]) and np.array_equal(got[3], ref[3]) and np.array_equal(got[1], ref[1])
    rel = np.abs(got[0].astype(np.float64) - ref[0]) / np.maximum(1.0, np.abs(ref[0]))
    assert np.isfinite(got[0]).all() and rel.max() <= SAME_MAX, rel.max()
