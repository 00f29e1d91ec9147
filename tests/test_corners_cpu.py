"""Corner scenes (tests/corner_scenes.py), CPU tier: the oracle's texture and sky lookups against numpy restatements of the reference on the
image shapes those scenes use (non-square, 1 x N, N x 1, 1 x 1, non-power-of-two — the oracle had only met square images either), how
discontinuous the reference is on every view (the source of the caps), and the host emulation of the kernels' per-lane code against the
oracle, path by path — the twin of tests/test_corners_gpu.py."""
import math

import numpy as np
import pytest

import corner_scenes as cs
from test_oracle import _bilinear_numpy

TINY = 2.0 ** -40


@pytest.fixture(scope="module")
def lookups(ha, orc):
    """the two skyboxes with the surface images behind them: {name: (scene, oracle scene)}"""
    out = {}
    for name, s in (("nonsquare", cs.cuboid_edges(ha, "ppp")), ("mixed", cs.inside_glass(ha, "refraction"))):
        out[name] = (s, orc.OracleScene(s.desc_ptr))
    return out


def _coords(n):
    """0, 1, every k / n exactly and beside it by 2^-40, a value just below 0 and one just above 1, and one that is nothing special"""
    v = [k / n + d for k in range(n + 1) for d in (0.0, -TINY, TINY)]
    return sorted(set(v + [-2.0 ** -30, 1.0 + 2.0 ** -30, 0.37]))


@pytest.mark.parametrize("which", ["nonsquare", "mixed"])
def test_oracle_bilinear_on_corner_image_shapes(lookups, which):
    """texture.rs:29-49 + 59-63 (tests/test_oracle.py _bilinear_numpy) on every image of the corner scenes: the clamp of x against the WIDTH,
    the flipped and wrapped row against the HEIGHT, at and beside every texel border, below 0 and above 1."""
    s, o = lookups[which]
    seen = set()
    for k, im in enumerate(s.arrays):
        h, w = im.shape[:2]
        seen.add((w, h))
        for u in _coords(w):
            for v in _coords(h):
                got, exp = o.image_bilinear(k, u, v), _bilinear_numpy(im, u, v)
                assert np.allclose(got, exp, rtol=1e-13, atol=1e-15), (k, (w, h), u, v, got, exp)
    assert seen == set(cs.SKY_NONSQUARE + cs.SURFACE_IMAGES if which == "nonsquare" else cs.SKY_MIXED + cs.SURFACE_IMAGES)


def _sky_numpy(s, d):
    """Skybox::sample, scene.rs:295-319: strict comparisons (a tie falls through to the Z faces), is_sign_positive, sample_bilinear_0center
    (texture.rs:22-26) on the face's own image."""
    x, y, z = (float(c) for c in d)
    ax, ay, az = abs(x), abs(y), abs(z)
    pos = lambda c: math.copysign(1.0, c) > 0.0
    if ax > ay and ax > az:
        face, u, v = (0, -z / x, y / x) if pos(x) else (1, -z / x, -y / x)
    elif ay > ax and ay > az:
        face, u, v = (2, x / y, -z / y) if pos(y) else (3, -x / y, -z / y)
    else:
        face, u, v = (4, x / z, y / z) if pos(z) else (5, x / z, -y / z)
    inten = np.array(s.desc.skybox.intensity.tuple())
    return face, inten * _bilinear_numpy(s.arrays[face], 0.5 * (u + 1.0), 0.5 * (v + 1.0))


def _sky_directions():
    dirs = []
    for a in range(3):                                  # the axes
        for sg in (1.0, -1.0):
            d = [0.0, 0.0, 0.0]; d[a] = sg
            dirs.append(d)
    for a, b in ((0, 1), (0, 2), (1, 2)):               # every seam |d_a| == |d_b|: on it (a tie), and beside it by 2^-40 and by 1e-3
        c = 3 - a - b
        for sa in (1.0, -1.0):
            for sb in (1.0, -1.0):
                for third in (0.3, -0.45, 0.0):
                    for eps in (0.0, TINY, -TINY, 1e-3, -1e-3):
                        d = [0.0, 0.0, 0.0]
                        d[a], d[b], d[c] = sa, sb * (1.0 + eps), third
                        if not (a, b) == (0, 1) or third != 0.0 or eps != 0.0:      # (x == y, z == 0: the tie's Z face divides by zero)
                            dirs.append(d)
    for sx in (1.0, -1.0):                              # the eight corners: three-way ties
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                dirs.append([sx, sy, sz])
                dirs.append([sx * (1 + TINY), sy, sz * (1 - TINY)])
    return dirs


@pytest.mark.parametrize("which", ["nonsquare", "mixed"])
def test_oracle_skybox_on_corner_faces(lookups, which):
    """orc_skybox_sample against the numpy restatement: directions on and beside every seam, the ties, the corners, the axes — on faces that are
    not square and on faces of six different sizes, where a lookup in another face's image, or with w and h swapped, shows."""
    s, o = lookups[which]
    faces = set()
    for d in _sky_directions():
        face, exp = _sky_numpy(s, d)
        faces.add(face)
        got = o.skybox(np.array(d, dtype=np.float64))
        assert np.isfinite(exp).all() and np.allclose(got, exp, rtol=1e-13, atol=1e-15), (d, face, got, exp)
    assert faces == set(range(6))
    # a tie goes to a Z face: (1, 1, 0.5) is +z's (scene.rs:300-318)
    assert _sky_numpy(s, [1.0, 1.0, 0.5])[0] == 4 and _sky_numpy(s, [-1.0, 0.3, -1.0])[0] == 5


def test_corner_images_follow_the_content_rule(ha):
    """every image: green ramps by >= 4/255 per texel along x, blue along y, red along both (roughness reads red), nothing wraps or is darker than
    96/255, and no two images of a scene start from the same offsets"""
    for s in (cs.cuboid_edges(ha, "ppp"), cs.inside_glass(ha, "refraction")):
        starts = set()
        for im in s.arrays:
            a = im.astype(int)
            assert (np.diff(a[..., 1], axis=1) >= 4).all() and (np.diff(a[..., 2], axis=0) >= 4).all()
            assert (np.diff(a[..., 0], axis=1) >= 4).all() and (np.diff(a[..., 0], axis=0) >= 4).all()
            assert a[..., :3].min() >= 96
            starts.add(tuple(a[-1, 0, :3]))
        assert len(starts) == len(s.arrays)


@pytest.mark.parametrize("name", sorted(cs.CASES))
def test_reference_discontinuity_is_what_the_caps_were_derived_from(ha, orc, name):
    """The oracle on the case as built against the oracle with the eye nudged by 2^-22 of its distance to the target: the count of paths that
    change IS corner_scenes.NUDGE_MEASURED's (the caps are three times it), and it is at most 0.1 % of the paths."""
    count, worst, n = cs.nudge_count(ha, orc, name)
    print("corner %s: %d of %d paths change under the nudge, worst same-branch change %.3g" % (name, count, n, worst))
    assert count <= cs.MAX_NUDGE_SHARE * n, (name, count, n)
    rec_count, rec_worst = cs.NUDGE_MEASURED[name]
    assert count == rec_count and worst <= rec_worst, (name, count, worst, cs.NUDGE_MEASURED[name])


@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("name", sorted(cs.CASES))
def test_emulation_path_by_path(ha, orc, emu, name, precise):
    """path_advance<.., LOG> (and <.., PREC>) of pt_core.h / prec_core.h on the host against the oracle's path log: corner_scenes.check."""
    s, ref = cs.get(ha, orc, name)
    e = emu.EmuScene(s.desc_ptr)
    try:
        emu.set_precise(precise)
        got = e.path_log(s.w, s.h, 1)
    finally:
        emu.set_precise(False)
    a = cs.check(name, got, ref, "emulation, precise" if precise else "emulation, fp32")
    # the corner is the common case: the sky scenes end every path in a sky lookup, the others hit their subject with a fifth of the paths or more
    first = ref[2][..., 0] & 7
    if name.startswith("sky_nonsquare"):
        assert (first == 1).all() and (ref[1] == 1).all() and (got[1] == 1).all()
    elif name.startswith("sky_mixed"):
        assert (first == 3).any() and (first == 1).mean() > 0.8
    elif name.startswith("inside_glass"):
        assert (first != 1).all() and ((ref[2][..., 0] & 8) == 0).mean() > 0.3 and ((ref[2][..., 0] & 8) != 0).mean() > 0.1   # reflected (TIR, Fresnel) / transmitted
    else:
        assert (first != 1).mean() > 0.15
    assert a["paths"] == s.w * s.h * 4


def test_camera_inside_a_glass_sphere_sees_through_it(ha, orc, emu):
    """scene.rs:58-64 takes the near root only: from inside, t < 0 and the sphere is missed.  Every primary ray of a camera inside a glass sphere
    is a miss that ends in the sky — in the oracle, and in the per-lane code."""
    s = cs.inside_glass_sphere(ha)
    ref = orc.OracleScene(s.desc_ptr).path_log(s.w, s.h, 1)
    assert ((ref[2][..., 0] & 7) == 1).all() and (ref[1] == 1).all() and (ref[2][..., 9] == 0).all()
    e = emu.EmuScene(s.desc_ptr)
    for precise in (False, True):
        try:
            emu.set_precise(precise)
            got = e.path_log(s.w, s.h, 1)
        finally:
            emu.set_precise(False)
        cs.check_whole_frame(got, ref)


@pytest.mark.parametrize("south", [False, True])
def test_the_ray_that_hits_a_pole_exactly(ha, orc, emu, south):
    """A ray down the y axis onto an imaged GGX sphere: n.xz == 0, scene.rs:69-70 divides 0 by 0, u is a NaN, the roughness read at it is one, no
    half vector is sampled (material.rs:119-121's comparison is false) and the reference ends the path there with nothing — one path in a frame
    aimed exactly, none in any other.  The per-lane code clamps the quotient before acos (u = 0 or 1: the texel column the neighbouring rays
    converge to from one side) and goes on: finite, and the frame's other 15 paths are the oracle's."""
    s = cs.sphere_pole_exact(ha, south)
    ref = orc.OracleScene(s.desc_ptr).path_log(2, 2, 1)
    pole = (1, 1, 3)
    assert int(ref[2][pole][0]) & 7 == 7 and ref[1][pole] == 1 and not ref[0][pole].any()      # what the oracle does there
    e = emu.EmuScene(s.desc_ptr)
    for precise in (False, True):
        try:
            emu.set_precise(precise)
            got = e.path_log(2, 2, 1)
        finally:
            emu.set_precise(False)
        cs.check_pole_frame(got, ref, pole)
