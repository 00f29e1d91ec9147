"""Ray sets for the walk itself (csrc/pt_core.h ray_set / ray_quantise, trace_qnode / trace_node, node_advance with its two parked leaves,
trace_leaf with tri_test, sphere_root and cuboid_test; csrc/trace_kernel.h traverse_wave; shadow_early_out) and their judge: the BRUTE FORCE of
tests/bvh_edge_scenes.py — plain numpy f64, every ray against every primitive, no tree — with its `fragile` flag, decided from the brute force
alone.  The rule both tiers assert is ZERO disagreeing usable rays: no fraction gate.

  scenes   sweep_geometry(): a volumetric soup of ~1,500 primitives, the three kinds interleaved, long triangles (split_ratio duplicates their
           records) and triangles in axis planes (boxes of no extent);  ladder_geometry(): ~55 primitives, each >= 0.2 of the scene extent
  sets     1 octants     4,000 rays from all over the padded scene box at primitives' interior points, 500 per direction octant
           2 secondary   from the brute-force hits of set 1, pos +- 1e-4 n, directions uniform over the sphere
           3 near-axis   set 1 with one or two direction components replaced by +-m, m = 1e-3 .. 1e-42 (a denormal) and +-0.0
           4 inside      origins inside spheres (which return no hit from inside) and cuboids (which return their exit face)
           5 ragged      prefixes of set 1 (1, 63, 64, 65 rays) and set 1 plus 37 rays
           6 shadow      the hit rays of sets 1 and 2 with shadow_len = t_c + delta, the miss rays with four lengths; the reference verdict is
                         the reference renderer's: visible <=> the UNBOUNDED closest hit has (t_c - L)^2 < 4e-4
           7 ladder      on the ladder scene, origins D scene extents from the target, D = 1, 10, 100, ... up to the last rung at which the
                         brute force keeps half of the rays (and two rungs further, counted only); far_rays(): the same on the sweep scene,
                         with no judge, for the count of rays that the two record formats answer differently
  judge    sets 1, 2, 4: Brute as it is.  Sets 3 and 7: AxisBrute — Brute's triangle and sphere rules, and for cuboids a per-axis rule: an axis
           with |d_k| < 2^-20 takes no part in the distance (the ray passes that slab iff its origin is strictly inside it, and is fragile within
           64 eps (|o_k| + |plane|) of a plane), every other axis is perturbed by its own resolution 64 eps (|o| + |plane|) |1 / d_k|, and the ray
           is fragile when the perturbation can change hit / miss, the side of the origin or the face.  (Brute multiplies ONE resolution by
           max |1 / d|: right for directions with no small component, useless for these sets — and a +-0.0 component is 0 x inf there.)

Every set keeps ALL the rays it generated, with `usable` (not fragile, no near-tie, and in sets 1, 2, 4 no |d_k| < 1e-3); what is asserted is
asserted of the usable ones, and the order tests also count the others.  check() of every set asserts the conditions that keep this honest,
from the brute force alone.

No GPU in this module: tests/test_trace_sweeps_cpu.py runs the sets through the emulation, tests/test_trace_sweeps_gpu.py on the device."""
import numpy as np

import bvh_edge_scenes as bes
from bvh_edge_scenes import Brute, CUBOID, EPS32, Geometry, SPHERE, TRI, _unit

OFFSET = 1e-4                   # the renderer's surface offset (config.rs:7-8)
TINY_AXIS = 2.0 ** -20          # below this a direction component takes no part in a cuboid's distance
SMALL_COMPONENTS = (1e-3, 1e-6, 1e-12, 1e-20, 1e-30, 1.5e-38, 1e-42, 0.0)
SHADOW_DELTAS = (-1.0, -0.031, -0.029, -0.021, -0.019, -0.01, 0.0, 0.01, 0.019, 0.021, 0.03, 1.0)
MISS_LENGTHS = (1e-3, 1.0, 1e3, 3e38)
SHADOW_MARGIN = 1e-4
RAGGED = (1, 63, 64, 65)
PER_OCTANT = 500
LADDER_RAYS = 600
LADDER_TIE = 64.0 * EPS32       # two hits closer than this x (|o| + t) count as a tie on the ladder: fp32 places t to a few eps (|o| + t), and
                                # Case's 1e-5 — 170 eps — would call every pair of the scene's faces a tie from D = 1,000 on
LADDER_BITS_TOP = 1e3           # up to this rung the quantised walk returns the fp32 walk's bits on EVERY ray


# ------------------------------------------------------------------------------------------ the judge

class AxisBrute(Brute):
    """Brute with the per-axis cuboid rule of the module header"""

    def all_hits(self, r):
        g = self.g
        nt, ns, nc = g.counts
        t, frag = np.zeros((len(r), 0)), np.zeros(len(r), dtype=bool)
        if nt + ns:
            self.g = _without_cuboids(g)
            try:
                t, frag = Brute.all_hits(self, r)
            finally:
                self.g = g
        if nc:
            tc, fc = _cuboids_per_axis(g.cb, r)
            t, frag = np.concatenate([t, tc], axis=1), frag | fc
        return t, frag


def _without_cuboids(g):
    if getattr(g, "_no_cb", None) is None:
        h = object.__new__(Geometry)
        h.__dict__.update(g.__dict__)
        h.cb = g.cb[:0]
        g._no_cb = h
    return g._no_cb


def _cuboids_per_axis(cb, r):
    o, d = r[:, None, :3], r[:, None, 3:]
    mn, mx = cb[None, :, :3], cb[None, :, 3:]
    live = np.broadcast_to(np.abs(d) >= TINY_AXIS, (len(r), len(cb), 3))
    with np.errstate(all="ignore"):
        inv = np.where(np.abs(d) >= TINY_AXIS, 1.0 / np.where(d == 0.0, 1.0, d), 0.0)
        ta, tb = (mn - o) * inv, (mx - o) * inv
        size = np.abs(o).max(axis=-1, keepdims=True) + np.maximum(np.abs(mn), np.abs(mx)).max(axis=-1, keepdims=True)
        res = np.where(live, 64.0 * EPS32 * size * np.abs(inv), 0.0)
        inside = (mn < o) & (o < mx)
        lo = np.where(live, np.minimum(ta, tb), np.where(inside, -np.inf, np.inf))
        hi = np.where(live, np.maximum(ta, tb), np.where(inside, np.inf, -np.inf))
        tmin, tmax = lo.max(axis=-1), hi.min(axis=-1)
        ok = (tmin <= tmax) & (tmax >= 0.0)
        t = np.where(ok, np.where(tmin >= 0.0, tmin, tmax), np.inf)
        tmin_lo, tmin_hi = (lo - res).max(axis=-1), (lo + res).max(axis=-1)
        tmax_lo, tmax_hi = (hi - res).min(axis=-1), (hi + res).min(axis=-1)
        may = tmin_lo <= tmax_hi                                     # some perturbation makes the slabs overlap
        near = may & ~(tmin_hi <= tmax_lo)                           # ... and some does not
        near |= may & ((tmax_lo >= 0.0) != (tmax_hi >= 0.0))         # the box ends at the origin
        near |= may & (tmax_hi >= 0.0) & ((tmin_lo >= 0.0) != (tmin_hi >= 0.0))   # the origin on the entry face
        # the distance is one axis's term (the largest entry; from inside, the smallest exit).  fp32 places that term to res / 64: where an axis
        # that decides the distance, or can come to decide it, carries more than a quarter of ROUND_MAX, fp32 does not resolve t to the bound
        first = np.where(tmin[..., None] >= 0.0, lo, -hi)
        win = first.max(axis=-1, keepdims=True)
        res_win = np.take_along_axis(res, first.argmax(axis=-1)[..., None], axis=-1)
        decides = first + res >= win - res_win
        near |= ok & (decides & (res > 64.0 * 0.25 * bes.ROUND_MAX * np.maximum(1.0, np.abs(win)))).any(axis=-1)
        edge = 64.0 * EPS32
        dead_near = ~live & ((np.abs(o - mn) < edge * (np.abs(o) + np.abs(mn))) | (np.abs(o - mx) < edge * (np.abs(o) + np.abs(mx))))
        # a plane of a dead axis matters only where the other two axes let the ray through the box at all
        lo2, hi2 = np.where(live, lo - res, -np.inf).max(axis=-1), np.where(live, hi + res, np.inf).min(axis=-1)
        near |= dead_near.any(axis=-1) & (lo2 <= hi2) & (hi2 >= 0.0)
    return t, near.any(axis=1)


# ------------------------------------------------------------------------------------------ the scenes

def sweep_geometry(n=1500, seed=4101):
    """~n primitives in clusters inside [-3, 3]^3, kinds interleaved (k % 3), sizes log-uniform 0.05 .. 0.8; the first triangles are long ones
    (24, length 3 .. 5 by 0.15 or 0.002: early split clipping cuts them into several references — the thin ones, whose box has more than 4,000
    times their area, even at split_ratio 1000), the next lie in axis planes (48)"""
    rng = np.random.default_rng(seed)
    clusters = rng.uniform(-2.0, 2.0, (12, 3))
    spread = 10.0 ** rng.uniform(-0.6, 0.0, 12)
    which = rng.integers(0, 12, n)
    centres = np.clip(clusters[which] + rng.normal(size=(n, 3)) * spread[which, None], -3.0, 3.0)
    sizes = 10.0 ** rng.uniform(-1.3, -0.1, n)
    tris, sph, cub, order = [], [], [], []
    for k in range(n):
        c, s = centres[k], sizes[k]
        if k % 3 == TRI:
            j = len(tris)
            if j < 24:
                along = _unit(rng.normal(size=3)) * rng.uniform(3.0, 5.0)
                across = _unit(np.cross(along, rng.normal(size=3))) * (0.15 if j % 2 else 0.002)
                c = 0.3 * c
                tris.append([c - 0.5 * along, c + 0.5 * along, c + across])
            elif j < 72:
                a = j % 3
                t = np.array(bes._small_tri(rng, c, max(s, 0.2)))
                t[:, a] = np.float32(c[a])
                tris.append(t)
            else:
                tris.append(bes._small_tri(rng, c, s))
        elif k % 3 == SPHERE:
            sph.append([c[0], c[1], c[2], 0.5 * s]); order.append(SPHERE)
        else:
            h = 0.5 * s * rng.uniform(0.5, 1.0, 3)
            cub.append(list(c - h) + list(c + h)); order.append(CUBOID)
    return Geometry(tris, sph, cub, order)


def ladder_geometry(seed=4102, spheres=False):
    """~55 primitives, each at least 0.2 of the scene extent in size.  A ray from D extents away is placed to 64 eps D extents: whatever it passes
    closer than that to an edge or a silhouette makes it fragile, so a scene of large primitives strewn about loses every ray by D = 1,000.  The
    primitives are therefore arranged so that a ray at an interior point passes the others through their faces: 18 nested cuboids of three
    aspect orders about one centre (which one a ray enters first depends on its direction), and 36 large triangles on a sphere around them,
    facing the centre.  With `spheres`, 12 spheres about the centre too: Brute's sphere rule (what fp32 resolves of the discriminant,
    64 eps (b^2 + |o - c|^2 + r^2)) calls every ray fragile that passes within 2.8e-3 D extents of a sphere's surface — from D = 100 on that is
    every ray of a scene that holds a sphere at all, whatever the sizes — so the ladder proper climbs without spheres, and the scene with
    spheres is climbed as far as the same half-of-the-rays rule lets it."""
    rng = np.random.default_rng(seed)
    c0 = np.array([0.3, -0.2, 0.1])
    tris, sph, cub, order = [], [], [], []
    aspects = np.array([[1.0, 0.85, 0.7], [0.7, 1.0, 0.85], [0.85, 0.7, 1.0]])
    for k in range(18):
        c = c0 + rng.uniform(-0.05, 0.05, 3)
        h = 1.9 * (3.4 / 1.9) ** (k / 17.0) * aspects[k % 3]
        cub.append(list(c - h) + list(c + h)); order.append(CUBOID)
    for k in range(36):
        c = c0 + _unit(rng.normal(size=3)) * 4.5
        tris.append(bes._facing_tri(rng, c, rng.uniform(4.0, 4.2), c0))
    for k in range(12 if spheres else 0):
        c = c0 + rng.uniform(-0.3, 0.3, 3)
        sph.append([c[0], c[1], c[2], 2.6 + 0.1 * k]); order.append(SPHERE)
    g = Geometry(tris, sph, cub, order)
    ext = extent(g)
    small = [k for k in range(sum(g.counts)) if min(_sizes_of(g, k)) < 0.2 * ext]
    assert not small, ("ladder scene: primitives below 0.2 of the extent", small, ext)
    return g


def extent(g):
    lo, hi = g.bounds()
    return float((hi - lo).max())


def _sizes_of(g, k):
    """the primitive's extents that matter for 'large': a triangle's two record edges, a sphere's radius, a cuboid's three sides"""
    nt, ns, nc = g.counts
    if k < nt:
        return [np.linalg.norm(g.e1[k]), np.linalg.norm(g.e2[k])]
    if k < nt + ns:
        return [g.sp[k - nt, 3]]
    return list(g.cb[k - nt - ns, 3:] - g.cb[k - nt - ns, :3])


# ------------------------------------------------------------------------------------------ a set

class _Sub:
    """what bes.check_against_brute / check_same_hits take: a name and the brute force of the rays in question"""

    def __init__(self, name, ref):
        self.name, self.ref = name, ref


def octant_of(rays):
    """by SIGN BIT, as ray_set: -0.0 counts as negative"""
    s = np.signbit(np.asarray(rays, dtype=np.float32)[:, 3:6])
    return s[:, 0] * 1 + s[:, 1] * 2 + s[:, 2] * 4


class SweepSet:
    """name, geometry, ALL the rays generated (fp32, n x 6), their brute force, `usable`, and `case`: the usable rays as a bes case"""

    def __init__(self, name, g, rays, judge=Brute, min_d=1e-3, classes=None, class_names=None, tie=1e-5):
        self.name, self.g = name, g
        self.rays = np.ascontiguousarray(np.asarray(rays, dtype=np.float32).reshape(-1, 6))
        self.ref = b = judge(g, self.rays)
        ok = ~b.fragile
        if min_d:
            ok &= np.abs(b.rays[:, 3:]).min(axis=1) > min_d
        with np.errstate(invalid="ignore"):
            ok &= ~(b.hit & (b.t2 - b.t < tie * (np.linalg.norm(b.rays[:, :3], axis=1) + b.t)))
        self.usable = ok
        self.idx = np.where(ok)[0]
        self.case = _Sub(name, b.take(self.idx))
        self.octant = octant_of(self.rays)
        self.classes, self.class_names = classes, class_names

    def __len__(self):
        return len(self.rays)

    def counts(self):
        u = self.usable
        return {"generated": len(self), "dropped": int((~u).sum()), "usable_per_octant": [int((u & (self.octant == o)).sum()) for o in range(8)],
                "hits": int(self.ref.hit[u].sum())}

    def check(self, least=1000, per_octant=100, hit_rate=0.6):
        """the conditions that keep the tests honest, from the brute force alone"""
        c = self.counts()
        n_use = len(self.idx)
        assert n_use >= 0.5 * len(self) and n_use >= least, (self.name, c)
        if per_octant:
            assert min(c["usable_per_octant"]) >= per_octant, (self.name, c)
        assert c["hits"] >= hit_rate * n_use, (self.name, c)
        assert not self.case.ref.fragile.any(), self.name
        if self.classes is not None:
            for k, label in enumerate(self.class_names):
                assert (self.usable & (self.classes == k)).sum() >= 100, (self.name, label, int((self.usable & (self.classes == k)).sum()))
        return c


def check_walk(s, got, gel, what):
    """bes.check_against_brute on the usable rays: every hit flag, t within the module's bounds, the element (ties as there)"""
    return bes.check_against_brute(s.case, got[s.idx], gel[s.idx], what)


def t_errors(s, got):
    """worst |dt| against the brute force per primitive kind over the usable hits, in the units of the bounds (triangles / scale, the others / max(1, t))"""
    b, g_ = s.case.ref, got[s.idx]
    out = {}
    for kind, name in ((TRI, "tri"), (SPHERE, "sphere"), (CUBOID, "cuboid")):
        sel = b.hit & (b.kind == kind) & (g_[:, 0] == 1)
        if sel.any():
            out[name] = float((np.abs(g_[sel, 1].astype(np.float64) - b.t[sel]) / (b.scale[sel] if kind == TRI else np.maximum(1.0, b.t[sel]))).max())
    return out


def check_same(s, got, gel, base, base_el, what):
    """bes.check_same_hits on the usable rays"""
    bes.check_same_hits(s.case, got[s.idx], gel[s.idx], base[s.idx], base_el[s.idx], what)


def differing(a, ael, b, bel):
    """per ray: hit flag, t (bits) or element differ"""
    return (a[:, 0] != b[:, 0]) | (a[:, 1].view(np.uint32) != b[:, 1].view(np.uint32)) | (ael != bel)


def check_same_bits(s, got, gel, base, base_el, what, every_ray=False):
    """the usable rays (every_ray: all of them) return the same hit flag, t and element, bit for bit; returns how many of the OTHER rays differ"""
    diff = differing(got, gel, base, base_el)
    must = np.ones(len(s), dtype=bool) if every_ray else s.usable
    bad = np.where(diff & must)[0]
    assert len(bad) == 0, (s.name, what, "rays differ", bad[:10].tolist(), [(s.rays[i].tolist(), got[i, :2].tolist(), base[i, :2].tolist()) for i in bad[:3]])
    return int((diff & ~must).sum())


# ------------------------------------------------------------------------------------------ the sets of the sweep scene

def _fp32_rays(o, d):
    return np.concatenate([np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)], axis=1).astype(np.float32)


def _sphere_dirs(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def make_octants(g, seed=4111):
    """set 1: per octant PER_OCTANT rays; the target is a random primitive's interior point, the origin uniform in the part of the padded scene
    box from which the target lies in that octant"""
    rng = np.random.default_rng(seed)
    lo, hi = g.bounds()
    pad = 0.15 * (hi - lo)
    pts = bes._aim_points(g, rng, sum(g.counts))
    o, tg = [], []
    for octant in range(8):
        p = pts[rng.integers(0, len(pts), PER_OCTANT)]
        neg = np.array([(octant >> a) & 1 for a in range(3)], dtype=bool)
        u = rng.uniform(0.02, 1.0, (PER_OCTANT, 3))
        o.append(np.where(neg, p + u * (hi + pad - p), p - u * (p - (lo - pad))))
        tg.append(p)
    o, tg = np.concatenate(o), np.concatenate(tg)
    order = rng.permutation(len(o))                       # octants mixed in every wave
    o, tg = o[order], tg[order]
    s = SweepSet("octants", g, _fp32_rays(o, _unit(tg - o)))
    s.target = tg
    return s


def hit_points(s):
    """(ray index, position, unit normal) of the usable hits of a set, from the brute force"""
    b, g = s.ref, s.g
    nt, ns, nc = g.counts
    idx = np.where(s.usable & b.hit)[0]
    pos = b.rays[idx, :3] + b.t[idx, None] * b.rays[idx, 3:]
    nrm = np.zeros_like(pos)
    for j, i in enumerate(idx):
        k = int(b.prim[i])
        if k < nt:
            nrm[j] = _unit(np.cross(g.e1[k], g.e2[k]))
        elif k < nt + ns:
            nrm[j] = _unit(pos[j] - g.sp[k - nt, :3])
        else:
            c = g.cb[k - nt - ns]
            dist = np.abs(np.concatenate([pos[j] - c[:3], pos[j] - c[3:]]))
            f = int(dist.argmin())
            nrm[j, f % 3] = -1.0 if f < 3 else 1.0
    return idx, pos, nrm


def make_secondary(s1, seed=4112):
    """set 2: from every usable hit of set 1, pos + 1e-4 n and pos - 1e-4 n, each with a direction uniform over the whole sphere"""
    rng = np.random.default_rng(seed)
    _, pos, nrm = hit_points(s1)
    o = np.concatenate([pos + OFFSET * nrm, pos - OFFSET * nrm])
    return SweepSet("secondary", s1.g, _fp32_rays(o, _sphere_dirs(rng, len(o))))


def make_near_axis(s1, seed=4113):
    """set 3: every ray of set 1 twice — once with one, once with two direction components replaced by +-m (the rest rescaled to unit
    length), the origin moved back along the new direction so that the ray still passes the target.  m cycles through SMALL_COMPONENTS,
    the signs and the axes are drawn."""
    rng = np.random.default_rng(seed)
    n = len(s1)
    d0 = s1.ref.rays[:, 3:]
    dist = np.linalg.norm(s1.target - s1.ref.rays[:, :3], axis=1)
    rays, classes, m_index = [], [], []
    for count in (1, 2):
        d = d0.copy()
        m = np.array(SMALL_COMPONENTS)[(np.arange(n) + count) % len(SMALL_COMPONENTS)]
        m32 = m.astype(np.float32).astype(np.float64)
        axes = np.array([rng.permutation(3) for _ in range(n)])
        sign = rng.choice([-1.0, 1.0], (n, 2))
        small = np.zeros((n, 3), dtype=bool)
        for c in range(count):
            small[np.arange(n), axes[:, c]] = True
            d[np.arange(n), axes[:, c]] = sign[:, c] * m32          # (-1.0 * 0.0 = -0.0: the sign bit is kept)
        rest = np.where(small, 0.0, d)
        rest *= (np.sqrt(1.0 - (np.where(small, d, 0.0) ** 2).sum(axis=1)) / np.linalg.norm(rest, axis=1))[:, None]
        d = np.where(small, d, rest)
        rays.append(_fp32_rays(s1.target - d * dist[:, None], d))
        classes.append((count - 1) * 2 + (sign[:, 0] < 0))
        m_index.append((np.arange(n) + count) % len(SMALL_COMPONENTS))
    s = SweepSet("near_axis", s1.g, np.concatenate(rays), judge=AxisBrute, min_d=0.0, classes=np.concatenate(classes),
                 class_names=["one component +", "one component -", "two components +", "two components -"])
    s.m_index = np.concatenate(m_index)
    return s


def make_inside(g, seed=4114):
    """set 4: origins inside every sphere (2 each) and every cuboid (3 each), centre +- 0.5 of the size, directions uniform over the sphere"""
    rng = np.random.default_rng(seed)
    o = []
    for c in g.sp:
        for _ in range(2):
            o.append(c[:3] + 0.5 * c[3] * _unit(rng.normal(size=3)) * rng.uniform(0.0, 1.0) ** (1.0 / 3.0))
    for c in g.cb:
        for _ in range(3):
            o.append(0.5 * (c[:3] + c[3:]) + 0.5 * 0.5 * (c[3:] - c[:3]) * rng.uniform(-1.0, 1.0, 3))
    o = np.array(o)
    return SweepSet("inside", g, _fp32_rays(o, _sphere_dirs(rng, len(o))))


class ShadowSet:
    """set 6: rays (fp32), length (fp32, the shadow_len of the query), visible (the reference verdict), delta (index into SHADOW_DELTAS, or
    -1 - index into MISS_LENGTHS), keep.  Made from the usable rays of the base sets, one query per ray, delta by turns."""

    def __init__(self, bases, chunk=128):
        g = bases[0].g
        rays, length, tc, hit, delta = [], [], [], [], []
        j = 0
        for s in bases:
            b = s.ref
            for i in s.idx:
                if b.hit[i]:
                    k = j % len(SHADOW_DELTAS)
                    L = np.float32(b.t[i] + SHADOW_DELTAS[k])
                    j += 1
                    if not L > 0.0:
                        continue
                    delta.append(k)
                else:
                    k = j % len(MISS_LENGTHS)
                    L = np.float32(MISS_LENGTHS[k])
                    j += 1
                    delta.append(-1 - k)
                rays.append(s.rays[i]); length.append(L); tc.append(b.t[i]); hit.append(b.hit[i])
        self.name, self.g = "shadow", g
        self.rays = np.ascontiguousarray(np.array(rays, dtype=np.float32))
        self.length = np.array(length, dtype=np.float32)
        self.delta = np.array(delta)
        L = self.length.astype(np.float64)
        tc, hit = np.array(tc), np.array(hit)
        with np.errstate(all="ignore"):
            self.visible = hit & ((tc - L) ** 2 < 4e-4)
        # a query is dropped when ANY primitive's hit distance is within the margin of the early-out threshold or of the search limit
        keep = np.ones(len(L), dtype=bool)
        b = Brute.__new__(Brute)
        b.g = g
        r64 = self.rays.astype(np.float64)
        for a in range(0, len(L), chunk):
            t, frag = Brute.all_hits(b, r64[a:a + chunk])
            Lc = L[a:a + chunk, None]
            with np.errstate(invalid="ignore"):
                near = (np.abs(np.abs(t - Lc) - 0.02) < SHADOW_MARGIN) | (np.abs(t - (Lc + 0.03)) < SHADOW_MARGIN)
            keep[a:a + chunk] = ~(near & np.isfinite(t)).any(axis=1) & ~frag
        self.keep = keep

    def __len__(self):
        return len(self.rays)

    def counts(self):
        k = self.keep
        return {"generated": len(self), "dropped": int((~k).sum()), "visible": int((self.visible & k).sum()), "not_visible": int((~self.visible & k).sum()),
                "per_delta": [int((k & (self.delta == d)).sum()) for d in range(len(SHADOW_DELTAS))],
                "per_miss_length": [int((k & (self.delta == -1 - d)).sum()) for d in range(len(MISS_LENGTHS))]}

    def check(self):
        c = self.counts()
        assert self.keep.sum() >= 0.5 * len(self) and self.keep.sum() >= 1000, c
        assert c["visible"] >= 200 and c["not_visible"] >= 200, c
        assert min(c["per_delta"]) >= 50 and min(c["per_miss_length"]) >= 50, c
        return c


def shadow_verdict(got, length):
    """renderer.rs:280 with vector.rs:89-91 on a query's answer: hit && (t - L)^2 < 4e-4"""
    with np.errstate(all="ignore"):
        return (got[:, 0] == 1) & ((got[:, 1].astype(np.float64) - np.asarray(length, dtype=np.float64)) ** 2 < 4e-4)


def check_shadow(sh, got, gel, closest, closest_el, what):
    """the verdict is the brute force's on every kept query; where visible, t and the element are the closest-hit query's bits for that ray"""
    v = shadow_verdict(got, sh.length)
    bad = np.where(sh.keep & (v != sh.visible))[0]
    assert len(bad) == 0, ("shadow", what, "verdicts differ on queries", bad[:10].tolist(),
                           [(float(sh.length[i]), got[i, :2].tolist(), closest[i, :2].tolist(), int(sh.delta[i])) for i in bad[:5]])
    vis = sh.keep & sh.visible
    same = ~differing(got, gel, closest, closest_el)
    assert same[vis].all(), ("shadow", what, "a visible query's hit is not the closest-hit query's", np.where(vis & ~same)[0][:10].tolist())
    return int(vis.sum())


# ------------------------------------------------------------------------------------------ the ladder

def make_rung(g, D, seed=4120):
    """LADDER_RAYS rays at jittered interior points of the ladder scene's primitives, from D scene extents away in uniform directions"""
    rng = np.random.default_rng(seed)
    pts = bes._aim_points(g, rng, sum(g.counts))
    nt = g.counts[0]                                       # two thirds of the rays at the nest about the centre, one third at the triangles
    k = np.where(rng.uniform(size=LADDER_RAYS) < 2.0 / 3.0, rng.integers(nt, len(pts), LADDER_RAYS), rng.integers(0, nt, LADDER_RAYS))
    p = pts[k]
    d = _sphere_dirs(rng, LADDER_RAYS)
    s = SweepSet("ladder_D%g" % D, g, _fp32_rays(p - d * D * extent(g), d), judge=AxisBrute, min_d=0.0, tie=LADDER_TIE)
    s.D = D
    return s


def origin_sensitivity(s):
    """what a one-ulp move of the origin (every component, away from zero) does to the brute force's own t, in the units of the bounds:
    (triangles: |dt| / scale, spheres and cuboids: |dt| / max(1, t)), the worst over the usable rays that keep their primitive"""
    o = s.rays.copy()
    o[:, :3] = np.nextafter(o[:, :3], np.where(o[:, :3] >= 0, np.inf, -np.inf).astype(np.float32))
    b2 = AxisBrute(s.g, o[s.idx])
    b = s.case.ref
    same = b.hit & b2.hit & (b.prim == b2.prim)
    out = [0.0, 0.0]
    for k, sel in enumerate((same & (b.kind == TRI), same & (b.kind != TRI))):
        if sel.any():
            dt = np.abs(b2.t[sel] - b.t[sel])
            out[k] = float((dt / (b.scale[sel] if k == 0 else np.maximum(1.0, b.t[sel]))).max())
    return tuple(out)


def check_rung(s, got, gel, what):
    """check_against_brute's assertions for a ladder rung: hit flags, elements (ties as there), and t within max(the module's bound, 8 x the brute
    force's own sensitivity to a one-ulp move of the origin at this rung) — the sensitivity is printed, and never comes from `got`"""
    b = s.case.ref
    g_, e_ = got[s.idx], gel[s.idx]
    hit = g_[:, 0] == 1
    assert np.array_equal(hit, b.hit), (s.name, what, "hit flags differ on usable rays", np.where(hit != b.hit)[0][:10].tolist())
    sens_tri, sens_round = origin_sensitivity(s)
    out = {"sens_tri": sens_tri, "sens_round": sens_round}
    tri, rnd = b.hit & (b.kind == TRI), b.hit & (b.kind != TRI)
    if tri.any():
        err = np.abs(g_[tri, 1].astype(np.float64) - b.t[tri]) / b.scale[tri]
        out["tri_max"], out["tri_p90"] = float(err.max()), float(np.quantile(err, 0.9))
    if rnd.any():
        err = np.abs(g_[rnd, 1].astype(np.float64) - b.t[rnd]) / np.maximum(1.0, b.t[rnd])
        out["round_max"], out["round_p99"] = float(err.max()), float(np.quantile(err, 0.99))
    print("%s %s vs brute force: %s" % (s.name, what, ", ".join("%s %.3g" % kv for kv in sorted(out.items()))))
    assert out.get("tri_max", 0.0) < max(bes.TRI_MAX, 8.0 * sens_tri) and out.get("tri_p90", 0.0) < max(bes.TRI_P90, 8.0 * sens_tri), (s.name, what, out)
    assert out.get("round_max", 0.0) < max(bes.ROUND_MAX, 8.0 * sens_round) and out.get("round_p99", 0.0) < max(bes.ROUND_P99, 8.0 * sens_round), (s.name, what, out)
    for i in np.where(b.hit & (e_ != b.elem))[0]:
        tol = 4.0 * max(bes.TRI_MAX * b.scale[i], EPS32 * max(1.0, float(g_[i, 1])), 8.0 * max(sens_tri * b.scale[i], sens_round * max(1.0, b.t[i])))
        assert int(e_[i]) in b.elements_at(i, b.t[i], tol), (s.name, what, "ray", int(i), "element", int(e_[i]), "brute force", int(b.elem[i]))
    return out


# The quantised walk's planes lie QMARGIN = 0.05 grid steps (of 65,532 across the scene) outside the true boxes to cover the fp32 error of
# q * qinv + qc: three roundings of 2^-24 relative on values up to |qmin - o|, i.e. 3 x 2^-24 x (D + 1) x 65,535 = 0.012 (D + 1) steps for an origin
# D extents away.  The margin covers that up to D = 3: within a few extents "same hits as the 32-byte walk" follows from the construction, and the rung
# D = 1 is asserted on EVERY ray of a scene of small primitives.  Further out it is a measurement (the 32-byte walk's own box test is no more
# exact there: it rounds plane - o to 2^-24 D extents as well), counted per rung and recorded in profiles/trace_sweeps.txt.
FAR_EQUAL, FAR_COUNTED = (1.0,), (10.0, 100.0, 300.0, 1e3, 3e3, 1e4, 1e5)
FAR_RAYS = 2000


def far_rays(g, D, n=FAR_RAYS, seed=4130):
    """n rays at interior points of g's primitives from D scene extents away, uniform directions — no judge: on the sweep scene, whose primitives are
    small, the brute force keeps none of them from D = 100 on.  They are for the one claim that needs no judge: the walk on the 16-byte records
    returns the 32-byte walk's bits."""
    rng = np.random.default_rng(seed + int(np.log10(D) * 8))
    pts = bes._aim_points(g, rng, sum(g.counts))
    p = pts[rng.integers(0, len(pts), n)]
    d = _sphere_dirs(rng, n)
    return np.ascontiguousarray(_fp32_rays(p - d * D * extent(g), d))


class Ladder:
    """set 7: rungs D = 1, 10, 100, ... up to the largest at which the brute force alone keeps at least half of the rays"""

    def __init__(self, spheres=False):
        self.g = ladder_geometry(spheres=spheres)
        self.spheres = spheres
        self.rungs = []
        D = 1.0
        while D <= 1e9:
            s = make_rung(self.g, D)
            if len(s.idx) < 0.5 * len(s):
                break
            self.rungs.append(s)
            D *= 10.0
        # two rungs further up, where the brute force keeps too little to judge: only counted (how many rays the two record formats answer differently)
        self.beyond = [make_rung(self.g, D), make_rung(self.g, 10.0 * D)]
        self.check()

    def check(self):
        assert self.rungs and self.rungs[-1].D >= (1.0 if self.spheres else 1e3), [(s.D, len(s.idx)) for s in self.rungs]
        for s in self.rungs:
            assert not s.case.ref.fragile.any() and len(s.idx) >= 0.5 * len(s), s.name
            assert s.ref.hit[s.usable].mean() >= 0.6, (s.name, s.counts())


# ------------------------------------------------------------------------------------------ made once

class Sweep:
    def __init__(self):
        self.g = g = sweep_geometry()
        self.octants = make_octants(g)
        self.secondary = make_secondary(self.octants)
        self.near_axis = make_near_axis(self.octants)
        self.inside = make_inside(g)
        self.shadow = ShadowSet([self.octants, self.secondary])
        self.plus37 = SweepSet("octants_plus_37", g, np.concatenate([self.octants.rays, self.inside.rays[:37]]))
        self.closest = [self.octants, self.secondary, self.near_axis, self.inside]
        self.counts = {}
        for s in self.closest:
            self.counts[s.name] = s.check()
        self.counts["octants_plus_37"] = self.plus37.check(per_octant=0)
        self.counts["shadow"] = self.shadow.check()

    def scene_holder(self, ha):
        if getattr(self, "_holder", None) is None:
            self._holder = self.g.scene(ha)
        return self._holder


_made = {}


def sweep():
    """the sweep scene and its sets, made once per process and not changed afterwards"""
    if "sweep" not in _made:
        _made["sweep"] = Sweep()
    return _made["sweep"]


def ladder(spheres=False):
    if ("ladder", spheres) not in _made:
        L = Ladder(spheres)
        L._holder = None
        _made["ladder", spheres] = L
    return _made["ladder", spheres]


def ladder_holder(ha, spheres=False):
    L = ladder(spheres)
    if L._holder is None:
        L._holder = L.g.scene(ha)
    return L._holder


def report():
    """the sets' counts as text (profiles/trace_sweeps.txt)"""
    out = []
    for name, c in sweep().counts.items():
        out.append("%-16s %s" % (name, c))
    for spheres in (False, True):
        for s in ladder(spheres).rungs:
            out.append("%-16s %s" % (s.name + (" (with spheres)" if spheres else ""), s.counts()))
    return "\n".join(out)
