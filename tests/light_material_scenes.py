"""Light and material scenes: small scenes in which a corner of next-event estimation (pt_core.h nee_setup, shadow_early_out and the shadow
branch of path_advance) or a material parameter at the end of its range is the COMMON case, for a path-by-path comparison with the f64 oracle
(tests/path_parity.py) — the recipe of tests/corner_scenes.py, whose Scene class, images and check these cases reuse.

Every case is 64 x 48, a pinhole, under six 12 x 5 sky faces of intensity 0.05.  All but the corridor stand on one floor cuboid and are seen
from (0.31, 2.5, 7.0); every light case exists with a Diffuse and with a GGX floor (the GGX floor is what nee_setup's second shortcut, the
emitter below a GGX surface's horizon, needs).  "Emitter" below: a Diffuse sphere of albedo 0.5 with an emission tint, no image.

  tiny          an emitter of radius 0.005: its whole diameter lies inside the 0.02 proximity window of renderer.rs:280, so a sample on its FAR
                side is "seen" through the near side — the far-side cull of nee_setup must not fire (x > 0.0221 can not hold with x <= r)
  marginal      radius 0.0105 (2 r at the window's edge: far-side samples seen near the silhouette only) and radius 0.03 (2 r just past the
                cull's slack of 0.0221: the cull begins to fire)
  large         radii 50 and 70, far above the scene: shadow rays of length 10 .. 130, the slack's 1e-6 len term, the walk limit len + 0.03
  touching      emitters cut by the floor, resting 4e-4 above it and hovering 0.01 above it: the floor inside the proximity window of samples
  close         emitters 2e-3, 2.1e-2 and 5e-2 above a GGX floor of roughness 0.2: shaded points a few 1e-3 from an emitter (len exceeds the
                far-side cull's 2 x by no more than that)
  overlap       two emitters that intersect, and one inside a concentric glass shell 0.01 larger: the shadow ray's closest hit inside the
                window is ANOTHER element (without emission: the verdict is "visible", what is added is nothing)
  shell_emits   the same shell with an emission of its own, read from the 1 x 5 image: hit_element / tex_sample in the shadow phase
  inside        the camera and every shaded point inside an emitter of radius 12 (scene.rs:61-63: the near root only — never hit from inside)
  many          nine emitters (the log folds emitter k into bit k mod 4; nine one-emitter variants tell them apart)
  mat_ggx       GGX with roughness 1e-3 and 1.0, F0 0 and 1
  mat_ior       Refraction with index 1.0, 1.0001, 0.8 (total reflection on the way IN) and 5.0
  mat_ggx_ior   GGXRefraction with (index, roughness) (1.0, 0.2), (1.5, 1e-3), (0.8, 0.3), (1.5, 1.0)
  mat_albedo    albedo exactly 0 (the is_zero(refl) stop) and exactly 1 on Diffuse, Specular, GGX and Refraction; one-channel albedos
  corridor      a closed box of six mirrors (albedo 0.93 .. 0.97): the iteration-9 stop is how every path ends

NOT a case: an emitter of radius 700 at a distance of 1000.  The sample's offset of 1e-4 from the surface is then below one fp32 ulp of the
sample's coordinates (6e-5 at 1000), so the fp32 scene can not say on which side of the surface the sample lies: NEE visibility differed on 244 ppm
of the paths, in fp32 and precise shading alike, while the reference's own nudge count was 0.  That is a limit of the fp32 scene format,
not a corner of the code.

No object shares a plane with the floor: the material cases' cuboids are sunk a few hundredths into it.  With a glass cuboid's bottom face IN
the floor's plane, a ray inside the glass meets two faces at the same distance, the reference resolves the tie by the order of its elements
and the fp32 walk by whichever rounding comes first — six paths of mat_ggx_ior left the cuboid where the oracle stayed inside, and the nudge
(which moves neither face) counted none of them.  An exact tie of the reference is no corner of the code (tests/corner_scenes.py aims its
views beside the cube map's seams for the same reason).  The spheres rest on the floor in one point; the light cases say how near they come.

The nudged variant of a case moves the eye as corner_scenes.Scene.finish does and, besides, every emitter's centre and radius by 2^-22
relative: a light case's discontinuities (a shadow ray grazing the emitter, a sample at the window's edge) hang on the emitter as much as on
the eye.

No GPU in this module: tests/test_light_material_cpu.py runs the cases through the emulation, tests/test_light_material_gpu.py on the device."""
import corner_scenes as cs
from corner_scenes import NUDGE, Y_UP

SKY_INTENSITY = (0.05, 0.05, 0.05)
EYE, TARGET = (0.31, 2.5, 7.0), (0.013, 0.3, 0.007)
LIGHT_FOV, MATERIAL_FOV = 14.0, 16.0
FLOORS = ("diffuse", "ggx")


def _scene(ha):
    s = cs.Scene(ha, cs.SKY_NONSQUARE)
    s.desc.skybox.intensity = ha.Vec3(*SKY_INTENSITY)
    return s


def _floor(s, floor, roughness=0.5):
    ha = s.ha
    surf, param = (ha.GGX, 0.8) if floor == "ggx" else (ha.DIFFUSE, 0.0)
    s.cuboid((-6.0, -1.0, -6.0), (6.0, 0.0, 6.0), s.material(surf, param, albedo=(0.8, 0.7, 0.6), roughness=roughness, imaged=False))


def _emitter(s, center, radius, tint):
    s.sphere(center, radius, s.material(s.ha.DIFFUSE, 0.0, albedo=(0.5, 0.5, 0.5), emission=tint, imaged=False))


def emitters_of(s):
    """indices into s.elements of the emitters, in the order of Scene::emissions (scene.rs:356-358: spheres with an emission tint)"""
    return [k for k, e in enumerate(s.elements) if e.kind == s.ha.SPHERE and any(e.material.emission.color.tuple())]


def _finish(s, eye, target, fov, nudge, vary):
    """vary: None, or one change to the scene as built —
         ("radius", k, f)      emitter k's radius times f
         ("roughness", i, f)   element i's roughness times f            ("param", i, f)   element i's index / F0 times f
         ("only", k)           every emitter but k loses its emission (the geometry stays)
         ("tint", k, rgb)      emitter k's emission tint"""
    ha = s.ha
    em = emitters_of(s)
    if nudge:
        for k in em:
            e = s.elements[k]
            e.center = ha.Vec3(*(c * (1.0 + NUDGE) for c in e.center.tuple()))
            e.radius = e.radius * (1.0 + NUDGE)
    if vary:
        what, k = vary[0], vary[1]
        if what == "radius":
            s.elements[em[k]].radius *= vary[2]
        elif what == "roughness":
            r = s.elements[k].material.roughness.color.x * vary[2]
            s.elements[k].material.roughness.color = ha.Vec3(r, r, r)
        elif what == "param":
            s.elements[k].material.param *= vary[2]
        elif what == "only":
            for j in em:
                if j != em[k]:
                    s.elements[j].material.emission.color = ha.Vec3(0.0, 0.0, 0.0)
        elif what == "tint":
            s.elements[em[k]].material.emission.color = ha.Vec3(*vary[2])
        else:
            raise ValueError(vary)
    return s.finish(eye, target, Y_UP, fov, nudge)


# ------------------------------------------------------------------------------------------ light cases

TINT = (8.0, 7.0, 6.0)
LIGHTS = {
    "tiny": [((0.1, 0.4, 0.2), 0.005, (4000.0, 3500.0, 3000.0))],
    "marginal": [((0.1, 0.4, 0.2), 0.0105, (1000.0, 900.0, 800.0)), ((-0.9, 0.3, -0.4), 0.03, (200.0, 200.0, 150.0))],
    "large": [((3.0, 60.0, -5.0), 50.0, (1.0, 0.9, 0.8)), ((-40.0, 90.0, 30.0), 70.0, (0.5, 0.5, 0.6))],
    "touching": [((0.2, 0.25, 0.1), 0.3, TINT), ((-1.0, 0.5004, 0.3), 0.5, TINT), ((1.2, 0.21, -0.5), 0.2, TINT)],
    "close": [((0.0, 0.302, 0.0), 0.3, TINT), ((1.0, 0.221, 0.3), 0.2, TINT), ((-1.0, 0.2, -0.2), 0.15, TINT)],
    "overlap": [((0.0, 0.7, 0.0), 0.4, TINT), ((0.5, 0.8, 0.1), 0.4, (3.0, 6.0, 9.0)), ((-1.2, 0.6, 0.4), 0.3, (9.0, 3.0, 3.0))],
    "shell_emits": [((0.3, 0.7, 0.0), 0.3, (9.0, 3.0, 3.0))],
    "inside": [((0.0, 1.0, 0.0), 12.0, (1.0, 1.0, 1.0)), ((0.4, 0.6, 0.2), 0.3, (8.0, 8.0, 8.0))],
    "many": [((-2.0 + 0.5 * k, 0.4 + 0.05 * k, -1.0 + 0.27 * k), 0.08 + 0.02 * k, (3.0 + k, 9.0 - k, 4.0)) for k in range(9)],
}
FLOOR_ROUGHNESS = {"close": 0.2, "many": 0.3}
SHELL_TINT = (2.0, 5.0, 2.0)
# the emitter whose radius the sensitivity test changes by 1 %: the first, except where the first is never seen (inside: scene.rs:61-63)
SENSITIVE_EMITTER = {"inside": 1}


def light(ha, case, floor, nudge=False, vary=None):
    s = _scene(ha)
    _floor(s, floor, FLOOR_ROUGHNESS.get(case, 0.5))
    for c, r, e in LIGHTS[case]:
        _emitter(s, c, r, e)
    if case == "overlap":
        c, r, _ = LIGHTS[case][2]
        s.sphere(c, r + 0.01, s.material(ha.REFRACTION, 1.5, albedo=(0.95, 0.97, 0.9), imaged=False))
    if case == "shell_emits":
        c, r, _ = LIGHTS[case][0]
        s.sphere(c, r + 0.008, s.material(ha.REFRACTION, 1.5, albedo=(0.95, 0.97, 0.9), emission=SHELL_TINT, imaged=True))
    return _finish(s, EYE, TARGET, LIGHT_FOV, nudge, vary)


# ------------------------------------------------------------------------------------------ material cases

# eight places in a row: spheres of radius 0.4 on the floor at the even ones, cuboids 0.6 wide behind them at the odd ones, nothing symmetric
ROW_X = (-2.41, -1.72, -1.03, -0.36, 0.33, 1.02, 1.69, 2.38)
ROW_DZ = (0.03, -0.05, -0.02, 0.04, 0.05, -0.03, 0.01, -0.04)
CUBOID_H = (0.0, 0.58, 0.0, 0.63, 0.0, 0.6, 0.0, 0.57)
CUBOID_SUNK = (0.0, 0.05, 0.0, 0.08, 0.0, 0.06, 0.0, 0.07)         # (see the module's header: no face in the floor's plane)
ALBEDO = (0.9, 0.85, 0.8)
MAT_EMITTER = ((0.0, 2.2, 0.5), 0.4, (20.0, 18.0, 16.0))

# (surface, param, roughness, albedo) of the eight objects; each parameter pair once on a sphere (even) and once on a cuboid (odd), the
# cuboids in another order so that no pair stands beside itself
def _materials(ha, case):
    if case == "mat_ggx":
        pairs = [(ha.GGX, f0, rough, ALBEDO) for rough, f0 in ((1e-3, 0.8), (1.0, 0.8), (0.3, 0.0), (0.3, 1.0))]
    elif case == "mat_ior":
        pairs = [(ha.REFRACTION, ior, 0.6, ALBEDO) for ior in (1.0, 1.0001, 0.8, 5.0)]
    elif case == "mat_ggx_ior":
        pairs = [(ha.GGX_REFRACTION, ior, rough, ALBEDO) for ior, rough in ((1.0, 0.2), (1.5, 1e-3), (0.8, 0.3), (1.5, 1.0))]
    else:
        one, zero = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
        return [(ha.DIFFUSE, 0.0, 0.6, zero), (ha.SPECULAR, 0.0, 0.6, zero), (ha.DIFFUSE, 0.0, 0.6, one), (ha.SPECULAR, 0.0, 0.6, one),
                (ha.GGX, 0.8, 0.3, zero), (ha.REFRACTION, 1.5, 0.6, zero), (ha.DIFFUSE, 0.0, 0.6, (1.0, 0.0, 0.0)), (ha.GGX, 0.8, 0.3, (0.0, 1.0, 0.0))]
    return [pairs[(k // 2) if k % 2 == 0 else (k // 2 + 2) % 4] for k in range(8)]


MATERIAL_CASES = ("mat_ggx", "mat_ior", "mat_ggx_ior", "mat_albedo")
FIRST_OBJECT = 1                     # elements: the floor, the eight objects, the emitter
# the sensitivity test's 1 % change: (what, element) — a roughness or an index in the middle of the path's arithmetic, not one at the end of
# its range (roughness 1e-3 times 1.01 is still a mirror)
SENSITIVE_OBJECT = {"mat_ggx": ("roughness", FIRST_OBJECT + 6), "mat_ior": ("param", FIRST_OBJECT + 6), "mat_ggx_ior": ("roughness", FIRST_OBJECT + 4),
                    "mat_albedo": ("roughness", FIRST_OBJECT + 7)}


def material(ha, case, nudge=False, vary=None):
    s = _scene(ha)
    _floor(s, "diffuse")
    for k, (surf, param, rough, albedo) in enumerate(_materials(ha, case)):
        m = s.material(surf, param, albedo=albedo, roughness=rough, imaged=False)
        x = ROW_X[k]
        if k % 2 == 0:
            s.sphere((x, 0.4, 0.5 + ROW_DZ[k]), 0.4, m)
        else:
            z = -0.6 + ROW_DZ[k]
            s.cuboid((x - 0.3, -CUBOID_SUNK[k], z - 0.3), (x + 0.3, CUBOID_H[k], z + 0.3), m)
    _emitter(s, *MAT_EMITTER)
    return _finish(s, EYE, TARGET, MATERIAL_FOV, nudge, vary)


# ------------------------------------------------------------------------------------------ the corridor

# (lo, hi, albedo): the inner faces are x = -3, 3, y = 0, 3, z = -4, 10; every slab reaches past its neighbours' inner faces
CORRIDOR_SLABS = [
    ((-3.7, -0.6, -4.8), (3.6, 0.0, 10.7), (0.95, 0.94, 0.93)),
    ((-3.6, 3.0, -4.7), (3.8, 3.8, 10.9), (0.96, 0.95, 0.97)),
    ((-3.9, -0.3, -4.6), (-3.0, 3.4, 10.6), (0.93, 0.96, 0.94)),
    ((3.0, -0.4, -4.5), (3.7, 3.3, 10.5), (0.97, 0.93, 0.95)),
    ((-3.5, -0.2, -4.9), (3.4, 3.5, -4.0), (0.94, 0.97, 0.96)),
    ((-3.3, -0.35, 10.0), (3.45, 3.45, 10.8), (0.95, 0.96, 0.93)),
]


def corridor(ha, nudge=False, vary=None):
    s = _scene(ha)
    for lo, hi, albedo in CORRIDOR_SLABS:
        s.cuboid(lo, hi, s.material(ha.SPECULAR, 0.0, albedo=albedo, imaged=False))
    _emitter(s, (0.4, 1.1, 0.3), 0.3, (20.0, 18.0, 16.0))
    s.sphere((-1.0, 0.8, 1.0), 0.5, s.material(ha.DIFFUSE, 0.0, albedo=ALBEDO, imaged=False))
    return _finish(s, (0.31, 1.5, 7.0), (0.113, 1.31, 0.007), 25.0, nudge, vary)


# ------------------------------------------------------------------------------------------ the cases and their limits

LIGHT, MATERIAL, CORRIDOR = "light", "material", "corridor"
# what a divergent path may be (path_parity.account's divergent_by_class_ppm):
#   light      the shadow ray's proximity test deciding the other way, a silhouette (floor edge, emitter), another cuboid face, and the
#              emitter against the floor (or the shell) it touches as the closest hit
#   material   those, the Fresnel coin / total reflection, and a GGX half vector at the horizon
#   corridor   a mirror's edge (another slab, same events), the emitter's silhouette, the proximity test
ALLOWED = {
    LIGHT: {"nee_visibility", "hit_vs_miss", "other_element_same_events", "other_surface_type"},
    MATERIAL: {"nee_visibility", "hit_vs_miss", "other_element_same_events", "other_surface_type", "reflect_vs_transmit", "ggx_sample_below_horizon"},
    CORRIDOR: {"hit_vs_miss", "other_element_same_events", "nee_visibility"},
}

CASES = {}          # name: (kind, build(ha, nudge=False, vary=None))
for _c in LIGHTS:
    for _f in FLOORS:
        CASES["%s-%s" % (_c, _f)] = (LIGHT, lambda ha, nudge=False, vary=None, c=_c, f=_f: light(ha, c, f, nudge, vary))
for _c in MATERIAL_CASES:
    CASES[_c] = (MATERIAL, lambda ha, nudge=False, vary=None, c=_c: material(ha, c, nudge, vary))
CASES["corridor"] = (CORRIDOR, corridor)
LIGHT_CASES = tuple(n for n in CASES if CASES[n][0] == LIGHT)


def light_case(name):
    return name.rsplit("-", 1)[0]


SAME_MAX = cs.SAME_MAX
MAX_NUDGE_SHARE = cs.MAX_NUDGE_SHARE

# How discontinuous the REFERENCE is, measured on the oracle alone (nudge_count below; profiles/light_material_scenes.txt holds these figures,
# the caps and what the emulation and the device measured): paths of sampling 1 whose events, hash or radiance (beyond 1e-3) change between
# the case as built and the nudged case.  cap = max(3, 3 x the count); the bound on the worst same-branch path is 1e-3, or, for the cases of
# MEASURED_SAME_MAX (paths that refract twice or more, and the corridor's eight mirrors in a row), max(1e-3, 3 x the worst change between
# the two oracle runs among the paths that kept their branch).
#   case: (nudge count, worst same-branch change between the two oracle runs)
NUDGE_MEASURED = {
    "tiny-diffuse": (0, 1.2e-06),
    "tiny-ggx": (0, 6.7e-07),
    "marginal-diffuse": (0, 8.7e-06),
    "marginal-ggx": (0, 7.6e-06),
    "large-diffuse": (0, 4.5e-06),
    "large-ggx": (0, 3.3e-06),
    "touching-diffuse": (0, 1.8e-05),
    "touching-ggx": (0, 1.7e-05),
    "close-diffuse": (0, 2.0e-05),
    "close-ggx": (0, 1.7e-05),
    "overlap-diffuse": (0, 1.1e-05),
    "overlap-ggx": (0, 1.7e-05),
    "shell_emits-diffuse": (0, 1.4e-06),
    "shell_emits-ggx": (0, 9.5e-07),
    "inside-diffuse": (0, 4.1e-06),
    "inside-ggx": (0, 2.3e-06),
    "many-diffuse": (0, 4.3e-05),
    "many-ggx": (0, 4.3e-05),
    "mat_ggx": (0, 1.5e-04),
    "mat_ior": (0, 9.4e-06),
    "mat_ggx_ior": (0, 1.3e-05),
    "mat_albedo": (0, 8.8e-05),
    "corridor": (0, 2.4e-04),
}
MEASURED_SAME_MAX = ("overlap-diffuse", "overlap-ggx", "shell_emits-diffuse", "shell_emits-ggx", "mat_ior", "mat_ggx_ior", "corridor")


def limits(name):
    """(cap on divergent paths + same-branch paths beyond 1e-3, bound on the worst same-branch path)"""
    count, worst = NUDGE_MEASURED[name]
    same_max = max(SAME_MAX, 3.0 * worst) if name in MEASURED_SAME_MAX else SAME_MAX
    return max(3, 3 * count), same_max


def oracle_log(orc, s):
    return orc.OracleScene(s.desc_ptr).path_log(s.w, s.h, 1)


def nudge_count(ha, orc, name):
    """(paths that change, worst radiance change among those that kept their branch, paths) between the oracle on the case as built and on
    the nudged case"""
    import path_parity
    acc = path_parity.account(oracle_log(orc, CASES[name][1](ha, True)), get(ha, orc, name)[1])
    n = acc["paths"]
    over = int(round(acc["same_branch"]["over_1e-3_floor1_ppm"] * n / 1e6))
    return acc["divergent"] + over, acc["same_branch"]["max_rel_floor1"], n


_made = {}


def get(ha, orc, name):
    """(scene, oracle path log of sampling 1): made once per process and not changed afterwards"""
    if name not in _made:
        s = CASES[name][1](ha)
        _made[name] = (s, oracle_log(orc, s))
    return _made[name]


def check(name, got, ref, what):
    """corner_scenes.check with this module's limits and classes"""
    cap, same_max = limits(name)
    return cs.check_against(name, ALLOWED[CASES[name][0]], cap, same_max, got, ref, what)


def nee_visible_share(log):
    """share of the paths with an NEE-visible bit in some iteration"""
    return float(((log[2][..., :9] & 0xf0) != 0).any(axis=-1).mean())
