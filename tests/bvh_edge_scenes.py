"""Edge geometry for the device BVH builders (csrc/lbvh_core.h, gpu_bvh.h, build_bvh_on_device): primitive counts on launch
boundaries, coincident and nested primitives, flat scenes, one huge outlier, slivers, an irregular soup — each with rays and
BRUTE-FORCE hits: plain numpy f64, every ray against every primitive, no tree.

  triangles  the reference's Cramer rule (bvh.rs:266-290) on the fp32 record the kernels see: v0, e1 = fp32(v1 - v0), e2 = fp32(v2 - v0);
             det == 0 rejects, t >= 0, u, v >= 0, u + v <= 1
  spheres    the quadratic (scene.rs:58-64): the near root only, d > 0 and t > 0 — a ray that starts inside a sphere misses it
  cuboids    slabs (bvh.rs:20-39): from inside, the exit face

Every coordinate is rounded to fp32 before it goes into the scene description, so the oracle (f64, the reference's median-split
BVH), the library and the brute force see the same numbers; no direction has a component near zero (the reference's slab test
makes 0 x inf = NaN of an axis-parallel ray in a box face).

What keeps the comparison honest is decided here, from the brute force alone (never from what a tree returns), and asserted by
Case.check(): rays whose hit / miss decision or nearest element hangs on less than fp32 can resolve — a ray that grazes an edge
or a silhouette, two distinct hits closer than 1e-5 — are dropped when the rays are made; at least 90 % of the rays hit; in the
cases A, D, F and G every primitive that can be hit (of the first 2,000) is the closest hit of some ray.

No GPU in this module: tests/test_bvh_edges_cpu.py runs the cases through the emulation, tests/test_bvh_edges_gpu.py on the device."""
import ctypes as C

import numpy as np

EPS32 = 2.0 ** -24
TRI, SPHERE, CUBOID = 0, 1, 2
PER_PRIM_CAP = 2000          # one aimed ray per primitive for the first so many
MESHES = 8                   # triangle k belongs to mesh element k % MESHES: the element says more than "some triangle"


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


class Geometry:
    """Primitives in element order: the meshes first (triangle k in mesh k % MESHES), then every sphere and cuboid as given."""

    def __init__(self, tris=(), spheres=(), cuboids=(), order=None):
        self.tv = _f32(np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3))           # triangle vertices
        self.sp = _f32(np.asarray(spheres, dtype=np.float64).reshape(-1, 4))           # centre, radius
        self.cb = _f32(np.asarray(cuboids, dtype=np.float64).reshape(-1, 6))           # min, max
        nt, ns, nc = len(self.tv), len(self.sp), len(self.cb)
        self.n_mesh = min(MESHES, nt)
        # the record the kernels test (flatten.cpp): v0 rounded, the edges formed in f64 and rounded once
        self.v0 = self.tv[:, 0]
        self.e1 = _f32(self.tv[:, 1] - self.tv[:, 0])
        self.e2 = _f32(self.tv[:, 2] - self.tv[:, 0])
        # spheres and cuboids interleaved in element order (order: 1 = sphere, 2 = cuboid), after the meshes
        if order is None:
            order = [SPHERE] * ns + [CUBOID] * nc
        assert list(order).count(SPHERE) == ns and list(order).count(CUBOID) == nc
        self.order = list(order)
        self.tri_elem = np.arange(nt) % max(1, self.n_mesh)
        el = self.n_mesh + np.arange(ns + nc)
        o = np.asarray(self.order, dtype=np.int64)
        self.sph_elem = el[o == SPHERE] if ns else np.zeros(0, dtype=np.int64)
        self.cub_elem = el[o == CUBOID] if nc else np.zeros(0, dtype=np.int64)
        self.elem = np.concatenate([self.tri_elem, self.sph_elem, self.cub_elem]).astype(np.int64)   # per primitive: tris, spheres, cuboids
        self.kind = np.concatenate([np.full(nt, TRI), np.full(ns, SPHERE), np.full(nc, CUBOID)])
        n = np.cross(self.e1, self.e2)
        self.degenerate = np.concatenate([(n * n).sum(axis=1) == 0.0, self.sp[:, 3] <= 0.0, (self.cb[:, 3:] < self.cb[:, :3]).any(axis=1)])

    @property
    def counts(self):
        return len(self.tv), len(self.sp), len(self.cb)

    def bounds(self):
        lo = [self.tv.reshape(-1, 3).min(axis=0)] if len(self.tv) else []
        hi = [self.tv.reshape(-1, 3).max(axis=0)] if len(self.tv) else []
        if len(self.sp):
            lo.append((self.sp[:, :3] - self.sp[:, 3:]).min(axis=0)); hi.append((self.sp[:, :3] + self.sp[:, 3:]).max(axis=0))
        if len(self.cb):
            lo.append(self.cb[:, :3].min(axis=0)); hi.append(self.cb[:, 3:].max(axis=0))
        return np.min(lo, axis=0), np.max(hi, axis=0)

    def scene(self, ha):
        """A SceneDesc over this geometry (camera / skybox / images borrowed from cornell_mini) in a holder Renderer.upload_scene,
        EmuScene and OracleScene take (.desc_ptr), with everything that must stay alive."""
        nt, ns, nc = self.counts
        base = ha.Scene("cornell_mini")
        el = (ha.Element * (self.n_mesh + ns + nc))()
        keep = [base, el]
        for e in el:
            e.material.albedo.color = ha.Vec3(0.7, 0.7, 0.7)
            e.material.albedo.image = e.material.emission.image = e.material.roughness.image = -1
        for k in range(self.n_mesh):
            verts = np.ascontiguousarray(self.tv[k::self.n_mesh].reshape(-1, 3))
            faces = np.ascontiguousarray(np.arange(verts.shape[0], dtype=np.uint64).reshape(-1, 3))
            keep += [verts, faces]
            el[k].kind = ha.MESH
            el[k].vertexes = verts.ctypes.data_as(C.POINTER(ha.Vec3))
            el[k].num_vertexes = verts.shape[0]
            el[k].faces = faces.ctypes.data_as(C.POINTER(C.c_uint64))
            el[k].num_faces = faces.shape[0]
        si = ci = 0
        for j, kind in enumerate(self.order):
            e = el[self.n_mesh + j]
            if kind == SPHERE:
                e.kind = ha.SPHERE
                e.center = ha.Vec3(*self.sp[si, :3]); e.radius = float(self.sp[si, 3])
                si += 1
            else:
                e.kind = ha.CUBOID
                e.aabb_min = ha.Vec3(*self.cb[ci, :3]); e.aabb_max = ha.Vec3(*self.cb[ci, 3:])
                ci += 1
        d = ha.SceneDesc()
        C.memmove(C.byref(d), base.desc_ptr, C.sizeof(d))
        d.elements = C.cast(el, C.POINTER(ha.Element))
        d.num_elements = len(el)

        class Holder:
            pass
        h = Holder()
        h.desc_ptr = C.pointer(d)
        h.keep = keep + [d]
        return h


class Brute:
    """Every ray against every primitive, f64.  Per ray: hit, t, the primitive (index over triangles, spheres, cuboids) and its element,
    the next distinct distance t2, the triangle-hit scale |o| + |o - v0| + |e1| + |e2| + t, and `fragile`: the decision hangs on less
    than fp32 resolves."""

    def __init__(self, g, rays, chunk=128):
        self.g = g
        r = np.asarray(rays, dtype=np.float32).astype(np.float64).reshape(-1, 6)
        n = len(r)
        self.hit = np.zeros(n, dtype=bool); self.t = np.full(n, np.inf); self.prim = np.full(n, -1, dtype=np.int64)
        self.t2 = np.full(n, np.inf); self.fragile = np.zeros(n, dtype=bool); self.scale = np.ones(n)
        for a in range(0, n, chunk):
            t, frag = self.all_hits(r[a:a + chunk])
            k = np.argmin(t, axis=1)
            t1 = t[np.arange(len(k)), k]
            self.hit[a:a + chunk] = np.isfinite(t1)
            self.t[a:a + chunk] = t1
            self.prim[a:a + chunk] = np.where(np.isfinite(t1), k, -1)
            later = np.where(t > t1[:, None], t, np.inf)
            self.t2[a:a + chunk] = later.min(axis=1)
            self.fragile[a:a + chunk] = frag
        self.elem = np.where(self.hit, g.elem[np.maximum(self.prim, 0)], -1)
        self.kind = np.where(self.hit, g.kind[np.maximum(self.prim, 0)], -1)
        tri = self.kind == TRI
        if tri.any():
            o, k = r[tri, :3], self.prim[tri]
            self.scale[tri] = (np.linalg.norm(o, axis=1) + np.linalg.norm(o - g.v0[k], axis=1) + np.linalg.norm(g.e1[k], axis=1)
                               + np.linalg.norm(g.e2[k], axis=1) + self.t[tri])
        self.rays = r

    FIELDS = ("hit", "t", "prim", "t2", "fragile", "scale", "elem", "kind", "rays")

    def take(self, idx):
        """the same results for a subset of the rays"""
        b = object.__new__(Brute)
        b.g = self.g
        for f in self.FIELDS:
            setattr(b, f, getattr(self, f)[idx])
        return b

    def plus(self, other):
        b = object.__new__(Brute)
        b.g = self.g
        for f in self.FIELDS:
            setattr(b, f, np.concatenate([getattr(self, f), getattr(other, f)]))
        return b

    def all_hits(self, r):
        """t of every (ray, primitive), inf = miss; and per ray whether some decision is closer to its border than fp32 resolves"""
        g = self.g
        o, d = r[:, None, :3], r[:, None, 3:]
        cols, frag = [], np.zeros(len(r), dtype=bool)
        on = np.linalg.norm(r[:, :3], axis=1)[:, None]
        with np.errstate(all="ignore"):
            if len(g.v0):
                e1, e2, v0 = g.e1[None], g.e2[None], g.v0[None]
                det = lambda a, b, c: (np.cross(a, b) * c).sum(axis=-1)
                den = det(e1, e2, -d)
                inv = 1.0 / den
                q = o - v0
                u = det(q, e2, -d) * inv
                v = det(e1, q, -d) * inv
                t = det(e1, e2, q) * inv
                ok = (den != 0.0) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t >= 0.0)
                cols.append(np.where(ok, t, np.inf))
                # fp32 places the hit point to about eps x (|o| + |o - v0| + |e1| + |e2| + t); in barycentric units that is divided by the
                # triangle's smallest altitude.  A ray within 32 such steps (or 2e-3) of an edge, or of t = 0, is fragile.
                l1, l2, l3 = np.linalg.norm(g.e1, axis=1), np.linalg.norm(g.e2, axis=1), np.linalg.norm(g.e2 - g.e1, axis=1)
                area2 = np.linalg.norm(np.cross(g.e1, g.e2), axis=1)
                alt = area2 / np.maximum(np.maximum(l1, l2), l3)
                sc = on + np.linalg.norm(q, axis=-1) + (l1 + l2)[None] + np.abs(t)
                tol = np.maximum(2e-3, 32.0 * EPS32 * sc / alt[None])
                margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
                near = (den != 0.0) & np.isfinite(t) & (t > -32.0 * EPS32 * sc) & (np.abs(margin) < tol)
                near |= ok & (t < 32.0 * EPS32 * sc)
                frag |= (near & (area2 > 0.0)[None]).any(axis=1)
            if len(g.sp):
                c, rad = g.sp[None, :, :3], g.sp[None, :, 3]
                a = o - c
                b = (a * d).sum(axis=-1)
                aa = (a * a).sum(axis=-1)
                disc = b * b - (aa - rad * rad)
                t = -b - np.sqrt(disc)
                ok = (disc > 0.0) & (t > 0.0)
                cols.append(np.where(ok, t, np.inf))
                res = 64.0 * EPS32 * (b * b + aa + rad * rad)          # what fp32 resolves of the discriminant
                near = (np.abs(disc) < res) | ((disc > 0.0) & (np.abs(t) < 64.0 * EPS32 * (np.abs(b) + np.sqrt(np.abs(disc)) + on)))
                frag |= near.any(axis=1)
            if len(g.cb):
                mn, mx = g.cb[None, :, :3], g.cb[None, :, 3:]
                inv = 1.0 / d
                ta, tb = (mn - o) * inv, (mx - o) * inv
                tmin, tmax = np.minimum(ta, tb).max(axis=-1), np.maximum(ta, tb).min(axis=-1)
                ok = (tmin <= tmax) & (tmax >= 0.0)
                cols.append(np.where(ok, np.where(tmin >= 0.0, tmin, tmax), np.inf))
                res = 64.0 * EPS32 * (np.abs(o).max(axis=-1) + np.maximum(np.abs(mn), np.abs(mx)).max(axis=-1)) * np.abs(inv).max(axis=-1)
                near = (np.abs(tmax - tmin) < res) | (np.abs(tmax) < res) | ((tmin <= tmax) & (np.abs(tmin) < res))
                frag |= near.any(axis=1)
        return np.concatenate(cols, axis=1), frag

    def elements_at(self, i, t, tol):
        """elements of every primitive that ray i hits within tol of t (equal-t ties: any of them is a right answer)"""
        tt, _ = self.all_hits(self.rays[i:i + 1])
        return set(self.g.elem[np.abs(tt[0] - t) <= tol].tolist())


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _aim_points(g, rng, first):
    """a jittered point inside each of the first `first` primitives"""
    nt, ns, nc = g.counts
    pts = []
    for k in range(min(first, nt)):
        u, v = rng.uniform(0.2, 0.4, 2)
        pts.append(g.v0[k] + u * g.e1[k] + v * g.e2[k])
    for k in range(min(max(first - nt, 0), ns)):
        pts.append(g.sp[k, :3] + rng.uniform(-0.3, 0.3, 3) * g.sp[k, 3])
    for k in range(min(max(first - nt - ns, 0), nc)):
        c, h = 0.5 * (g.cb[k, :3] + g.cb[k, 3:]), 0.5 * (g.cb[k, 3:] - g.cb[k, :3])
        pts.append(c + rng.uniform(-0.3, 0.3, 3) * h)
    return np.array(pts).reshape(-1, 3)


def _size_of(g, k):
    nt, ns, nc = g.counts
    if k < nt:
        return max(np.linalg.norm(g.e1[k]), np.linalg.norm(g.e2[k]))
    if k < nt + ns:
        return g.sp[k - nt, 3]
    return np.linalg.norm(g.cb[k - nt - ns, 3:] - g.cb[k - nt - ns, :3])


class Case:
    """name, geometry, rays (fp32, n x 6) and their brute-force hits"""

    def __init__(self, name, g, eyes, seed, random_rays=600, ties=False, cover=False, extra_origins=()):
        self.name, self.g, self.ties, self.cover = name, g, ties, cover
        rng = np.random.default_rng(seed)
        lo, hi = g.bounds()
        n = sum(g.counts)
        pts = _aim_points(g, rng, PER_PRIM_CAP)
        eyes = np.asarray(eyes, dtype=np.float64).reshape(-1, 3)
        cand = [np.concatenate([np.broadcast_to(eyes[0], pts.shape), _unit(pts - eyes[0])], axis=1)]     # the fixed eye, one ray per primitive
        tgt = rng.uniform(lo, hi, size=(random_rays, 3))
        org = np.concatenate([eyes, np.asarray(extra_origins, dtype=np.float64).reshape(-1, 3)])[rng.integers(0, len(eyes) + len(extra_origins), random_rays)]
        org = org + rng.normal(size=(random_rays, 3)) * 0.02 * np.linalg.norm(hi - lo)
        cand.append(np.concatenate([org, _unit(tgt - org)], axis=1))
        b = Brute(g, np.concatenate(cand).astype(np.float32))
        b = b.take(np.where(self._usable(b))[0])
        # primitives the eye does not see first get rays from close by, a few attempts each
        if cover:
            for attempt in range(10):
                seen = np.zeros(n, dtype=bool)
                seen[b.prim[b.hit]] = True
                todo = [k for k in range(min(n, PER_PRIM_CAP)) if not seen[k] and not g.degenerate[k]]
                if not todo:
                    break
                more = []
                for k in todo:
                    p = pts[k]
                    d = _unit(rng.normal(size=3))
                    back = _size_of(g, k) * (3.0 + attempt)
                    if k < g.counts[0]:                         # another interior point, from ever closer (a big triangle in a crowd)
                        u, v = rng.uniform(0.1, 0.45, 2)
                        p = g.v0[k] + u * g.e1[k] + v * g.e2[k]
                        nrm = _unit(np.cross(g.e1[k], g.e2[k]))
                        d = _unit(nrm * rng.choice([-1.0, 1.0]) + 0.4 * d)
                        back = _size_of(g, k) * 0.6 * 0.4 ** attempt
                    elif k < g.counts[0] + g.counts[1]:
                        p = g.sp[k - g.counts[0], :3]           # towards the centre, from outside
                    more.append(np.concatenate([p - d * back, d]))
                b2 = Brute(g, np.array(more, dtype=np.float32))
                b = b.plus(b2.take(np.where(self._usable(b2))[0]))
        # all the hits, and misses up to 5 % of them
        hits, misses = np.where(b.hit)[0], np.where(~b.hit)[0]
        self.ref = b.take(np.sort(np.concatenate([hits, misses[:len(hits) // 20]])))
        self.rays = np.ascontiguousarray(self.ref.rays.astype(np.float32))
        self.check()

    def scene_holder(self, ha):
        """the case's scene description, made once"""
        if getattr(self, "_holder", None) is None:
            self._holder = self.g.scene(ha)
        return self._holder

    def _usable(self, b):
        d = b.rays[:, 3:]
        ok = (np.abs(d).min(axis=1) > 1e-3) & ~b.fragile
        if not self.ties:
            with np.errstate(invalid="ignore"):
                ok &= ~(b.hit & (b.t2 - b.t < 1e-5 * (np.linalg.norm(b.rays[:, :3], axis=1) + b.t)))
        return ok

    def check(self):
        """the conditions that keep the tests honest, from the brute force alone"""
        b, g = self.ref, self.g
        assert len(self.rays) >= min(100, sum(g.counts)), (self.name, len(self.rays))
        assert b.hit.mean() >= 0.9, (self.name, b.hit.mean())
        assert not b.fragile.any() and np.abs(self.rays[:, 3:]).min() > 1e-3
        if not self.ties:
            assert (b.t2[b.hit] - b.t[b.hit] >= 1e-5 * b.t[b.hit]).all(), self.name
        if self.cover:
            n = min(sum(g.counts), PER_PRIM_CAP)
            seen = np.zeros(sum(g.counts), dtype=bool)
            seen[b.prim[b.hit]] = True
            missing = [k for k in range(n) if not seen[k] and not g.degenerate[k]]
            assert not missing, (self.name, "primitives no ray hits first", missing[:10], len(missing))


# ------------------------------------------------------------------------------------------ the cases

def _small_tri(rng, c, size):
    e1 = _unit(rng.normal(size=3)) * size
    e2 = rng.normal(size=3)
    e2 -= e1 * (e2 @ e1) / (e1 @ e1)
    e2 = _unit(e2) * size * rng.uniform(0.6, 1.0)
    v0 = c - (e1 + e2) / 3.0
    return [v0, v0 + e1, v0 + e2]


def _facing_tri(rng, c, size, eye):
    """a triangle around c that faces the eye within about 45 degrees"""
    n = _unit(_unit(eye - c) + 0.5 * rng.normal(size=3))
    a = _unit(np.cross(n, rng.normal(size=3)))
    b = np.cross(n, a)
    e1, e2 = a * size, (0.3 * a + b) * size * rng.uniform(0.6, 1.0)
    v0 = c - (e1 + e2) / 3.0
    return [v0, v0 + e1, v0 + e2]


def _mixed(rng, centres, sizes, kinds, eye):
    tris, sph, cub, order = [], [], [], []
    for c, s, k in zip(centres, sizes, kinds):
        if k == TRI:
            tris.append(_facing_tri(rng, c, s, eye))
        elif k == SPHERE:
            sph.append([c[0], c[1], c[2], 0.5 * s]); order.append(SPHERE)
        else:
            h = 0.5 * s * rng.uniform(0.5, 1.0, 3)
            cub.append(list(c - h) + list(c + h)); order.append(CUBOID)
    return Geometry(tris, sph, cub, order)


def case_counts(n, kinds=None):
    """A: n primitives on a jittered lattice facing the eye, the three kinds interleaved in space (or `kinds` of each)."""
    rng = np.random.default_rng(1000 + n + (sum(kinds) * 7 if kinds else 0))
    eye = np.array([0.3, 0.2, 9.0])
    side = int(np.ceil(np.sqrt(n)))
    ij = np.array([(i, j) for i in range(side) for j in range(side)][:n], dtype=np.float64)
    pitch = 4.0 / side
    centres = np.concatenate([(ij - 0.5 * (side - 1)) * pitch + rng.uniform(-0.15, 0.15, (n, 2)) * pitch, rng.uniform(-0.3, 0.3, (n, 1))], axis=1)
    if kinds is None:
        kk = np.arange(n) % 3
        name = "A_n%d" % n
    else:
        kk = rng.permutation(np.concatenate([np.full(c, k) for k, c in enumerate(kinds)]))
        name = "A_runs_%d_%d_%d" % tuple(kinds)
    g = _mixed(rng, centres, np.full(n, 0.45 * pitch), kk, eye)
    return Case(name, g, [eye], 11, random_rays=1500, cover=True)


def case_coincident(copies=300):
    """B: copies of one triangle next to copies of one sphere: every pair of the merge window has the same union area."""
    tri = [[-1.0, -0.5, 0.0], [0.25, -0.5, 0.125], [-0.5, 0.75, 0.0]]
    g = Geometry([tri] * copies, [[1.0, 0.0, 0.0, 0.5]] * copies)
    return Case("B_coincident_%d" % copies, g, [[0.2, 0.3, 5.0], [-0.4, 0.1, -5.0]], 12, random_rays=1500, ties=True)


def case_coincident_triangles(copies=5000):
    """B, for the merge loop: copies of one triangle — with ploc_top = 1 the loop makes ONE merge per iteration until it is stopped."""
    tri = [[-1.0, -0.5, 0.0], [1.0, -0.5, 0.125], [-0.5, 1.0, 0.0]]
    return Case("B_copies_%d" % copies, Geometry([tri] * copies), [[0.2, 0.3, 5.0], [-0.4, 0.1, -5.0]], 13, random_rays=400, ties=True)


def case_nested(kind, shells=64, r0=0.5, r1=1.5):
    """C: one centroid, different boxes.  Rays start outside and between the shells (a ray inside a sphere misses it; inside a cuboid it
    hits the exit face).  Boxes nested in Morton order are the merge loop's other worst case: one merge per iteration."""
    rad = np.linspace(r0, r1, shells)
    c = np.array([0.1, -0.2, 0.3])
    rng = np.random.default_rng(14)
    between = [c + _unit(rng.normal(size=3)) * 0.5 * (rad[k] + rad[k + 1]) * (1.0 if kind == SPHERE else 0.55) for k in range(0, shells - 1, max(1, shells // 16))]
    if kind == SPHERE:
        g = Geometry(spheres=[[c[0], c[1], c[2], r] for r in rad])
    else:
        g = Geometry(cuboids=[list(c - r * np.array([1.0, 0.8, 0.6])) + list(c + r * np.array([1.0, 0.8, 0.6])) for r in rad])
    return Case("C_nested_%s_%d" % ("spheres" if kind == SPHERE else "cuboids", shells), g, [[0.5, 0.4, 6.0]], 15, random_rays=1200, extra_origins=between)


def case_flat_plane(n=2000):
    """D: random triangles in the plane z = 0.25 (the scene has no extent in z)"""
    rng = np.random.default_rng(16)
    side = int(np.ceil(np.sqrt(n)))
    tris = []
    for k in range(n):
        c = np.array([(k % side + rng.uniform(0.3, 0.7)) / side * 4.0 - 2.0, (k // side + rng.uniform(0.3, 0.7)) / side * 4.0 - 2.0])
        a = rng.uniform(0, 2 * np.pi)
        s = 4.0 / side * rng.uniform(0.08, 0.28)          # inside its own cell: coplanar triangles that overlap would tie
        p = [c + s * np.array([np.cos(a + w), np.sin(a + w)]) for w in (0.0, 2.1 + rng.uniform(-0.4, 0.4), 4.2 + rng.uniform(-0.4, 0.4))]
        tris.append([[q[0], q[1], 0.25] for q in p])
    return Case("D_flat_plane_%d" % n, Geometry(tris), [[0.1, 0.2, 7.0]], 17, cover=True)


def case_flat_line(n=500):
    """D: thin triangles whose centroids lie on a line parallel to x (fp32-exact: no extent of the centroids in y and z)"""
    rng = np.random.default_rng(18)
    tris = []
    for k in range(n):
        x = -2.0 + 4.0 * k / n
        h, w = 0.5 * rng.choice([1.0, 0.5, 0.25]), 2.0 ** -10
        # centroid (x, 0.5, -0.25) to the bit: vertices at +-w in x, and y offsets that sum to zero
        tris.append([[x - w, 0.5 - h, -0.25], [x + w, 0.5 - h, -0.25], [x, 0.5 + 2 * h, -0.25]])
    for t in tris:   # x is a multiple of 2^-7 (4 k / 500 is not): snap it so that the centroid's x is exact too
        xs = np.round(np.array(t)[:, 0] * 2.0 ** 12) / 2.0 ** 12
        for v, x in zip(t, xs):
            v[0] = float(x)
    return Case("D_flat_line_%d" % n, Geometry(tris), [[0.1, 0.4, 6.0]], 19, cover=True)


def case_tiny_cube(n=500):
    """D: all primitives inside a cube of edge 1e-4"""
    rng = np.random.default_rng(20)
    c0 = np.array([2e-4, 1e-4, -1e-4])
    eye = c0 + np.array([1e-5, 2e-5, 4e-4])
    side = int(np.ceil(np.sqrt(n)))
    ij = np.array([(i, j) for i in range(side) for j in range(side)][:n], dtype=np.float64)
    pitch = 9e-5 / side
    centres = c0 + np.concatenate([(ij - 0.5 * (side - 1)) * pitch + rng.uniform(-0.1, 0.1, (n, 2)) * pitch, rng.uniform(-3e-5, 3e-5, (n, 1))], axis=1)
    g = _mixed(rng, centres, np.full(n, 0.5 * pitch), np.arange(n) % 3, eye)
    return Case("D_tiny_cube_%d" % n, g, [eye], 21, random_rays=300, cover=True)


def case_outlier(n=2000):
    """E: n triangles of edge 1e-3 in a unit cube, one triangle of edge 1e4, one sphere of radius 0.01 at distance 3e3: the Morton grid
    and the 16-bit quantised frame put every small primitive into a handful of cells."""
    rng = np.random.default_rng(22)
    eye = np.array([0.45, 0.55, 4.0])
    side = int(np.ceil(np.sqrt(n)))
    tris = []
    for k in range(n):
        c = np.array([(k % side + rng.uniform(0.3, 0.7)) / side, (k // side + rng.uniform(0.3, 0.7)) / side, rng.uniform(0.0, 1.0)])
        tris.append(_facing_tri(rng, c, 1e-3, eye))
    big = np.array([[-5000.0, -3000.0, -2.0], [5000.0, -3000.0, -2.5], [0.0, 5660.0, -3.0]])
    far = [2000.0, 1500.0, -1658.0, 0.01]          # |c| = 3e3
    g = Geometry(tris + [big], [far])
    near_far = np.array(far[:3]) + np.array([0.03, 0.02, 0.05])
    inside = [[0.5, 0.5, 0.5], [0.2, 0.7, 0.4]]
    c = Case("E_outlier_%d" % n, g, [eye], 23, random_rays=600, extra_origins=inside)
    # the far sphere from close by (from the cluster, 3e3 away, fp32 cannot resolve a radius of 0.01), and the big triangle from far off
    extra = [np.concatenate([near_far, _unit(np.array(far[:3]) + d - near_far)]) for d in ([0, 0, 0], [0.003, 0.001, 0.0], [-0.002, 0.004, 0.001])]
    extra += [np.concatenate([o, _unit(np.array(tg) - o)]) for o, tg in ((np.array([300.0, 200.0, 900.0]), [1000.0, 500.0, -2.5]), (np.array([-40.0, 30.0, 60.0]), [-2000.0, -1000.0, -2.3]))]
    c.ref = c.ref.plus(Brute(g, np.array(extra, dtype=np.float32)))
    c.rays = np.ascontiguousarray(c.ref.rays.astype(np.float32))
    c.check()
    assert c.ref.hit[-5:].all() and (c.ref.kind[-5:-2] == SPHERE).all() and (c.ref.prim[-2:] == n).all()
    return c


def case_slivers():
    """F: 200 triangles of aspect 1:1000 diagonal to all three axes, three triangles with collinear or equal vertices, 50 spheres and 50
    cuboids in the same volume"""
    rng = np.random.default_rng(24)
    eye = np.array([0.2, 0.1, 8.0])
    tris = []
    for k in range(200):
        c = np.array([(k % 20) * 0.2 - 1.9 + rng.uniform(-0.03, 0.03), (k // 20) * 0.4 - 1.8 + rng.uniform(-0.03, 0.03), rng.uniform(-1.0, 1.0)])
        long = _unit(np.array([1.0, rng.choice([-1.0, 1.0]), rng.choice([-1.0, 1.0])]) + 0.2 * rng.normal(size=3)) * 0.3
        across = _unit(np.cross(long, _unit(eye - c))) * 3e-4
        tris.append([c - 0.5 * long, c + 0.5 * long, c + across])
    tris += [[[0.5, 0.5, 1.5], [1.0, 1.0, 1.75], [1.5, 1.5, 2.0]],                 # collinear, diagonal
             [[-1.0, 1.0, 1.5], [-1.0, 1.0, 1.5], [-1.0, 1.0, 1.5]],               # three equal vertices
             [[-0.5, -1.0, 1.5], [-0.5, -1.0, 1.5], [0.25, -0.25, 1.75]]]          # two equal vertices
    centres = np.stack([rng.uniform(-1.9, 1.9, 100), rng.uniform(-1.9, 1.9, 100), rng.uniform(-3.0, -1.5, 100)], axis=1)
    centres[:, 0] = (np.arange(100) % 10) * 0.4 - 1.8 + rng.uniform(-0.05, 0.05, 100)
    centres[:, 1] = (np.arange(100) // 10) * 0.4 - 1.8 + rng.uniform(-0.05, 0.05, 100)
    m = _mixed(rng, centres, np.full(100, 0.2), 1 + np.arange(100) % 2, eye)
    g = Geometry(tris, m.sp, m.cb, m.order)
    return Case("F_slivers", g, [eye], 25, random_rays=800, cover=True)


def case_soup(n=20000):
    """G: primitives of all three kinds, log-uniform sizes 1e-3 .. 1, clustered positions"""
    rng = np.random.default_rng(26)
    eye = np.array([0.5, 0.3, 30.0])
    clusters = rng.uniform(-8.0, 8.0, (40, 3))
    spread = 10.0 ** rng.uniform(-1.0, 0.3, 40)
    which = rng.integers(0, 40, n)
    centres = clusters[which] + rng.normal(size=(n, 3)) * spread[which, None]
    sizes = 10.0 ** rng.uniform(-3.0, 0.0, n)
    kinds = rng.integers(0, 3, n)
    # the triangles that get an aimed ray (the first PER_PRIM_CAP primitives in Geometry's order: triangles come first) stand in front of
    # the rest, where the eye sees most of them; the random rays and the rays from inside the clusters reach spheres and cuboids
    front = np.where(kinds == TRI)[0][:PER_PRIM_CAP]
    centres[front, 2] = 12.0 + rng.uniform(0.0, 4.0, len(front))
    g = _mixed(rng, centres, sizes, kinds, eye)
    return Case("G_soup_%d" % n, g, [eye], 27, random_rays=1500, extra_origins=clusters[:8], cover=True)


COUNTS = (1, 2, 3, 63, 64, 65, 255, 256, 257)
RUNS = ((1, 1, 2), (1, 4, 5), (1, 15, 16))          # type runs of 1, max_leaf and max_leaf + 1 for max_leaf = 1, 4, 15

CASES = {}
for _n in COUNTS:
    CASES["A_n%d" % _n] = (lambda n=_n: case_counts(n))
for _r in RUNS:
    CASES["A_runs_%d_%d_%d" % _r] = (lambda r=_r: case_counts(sum(r), r))
CASES.update({
    "B_coincident": case_coincident,
    "C_nested_spheres": lambda: case_nested(SPHERE),
    "C_nested_cuboids": lambda: case_nested(CUBOID),
    "D_flat_plane": case_flat_plane,
    "D_flat_line": case_flat_line,
    "D_tiny_cube": case_tiny_cube,
    "E_outlier": case_outlier,
    "F_slivers": case_slivers,
    "G_soup": case_soup,
})
# the merge loop's two worst cases at a size where one merge per iteration overruns the old bound of 4,096 iterations (ploc_top = 1)
LOOP_CASES = {
    "B_copies_5000": case_coincident_triangles,
    "C_nested_spheres_4200": lambda: case_nested(SPHERE, shells=4200, r0=0.5, r1=1.5),
}

_made = {}


def get(name):
    """the case, made once per process and not changed afterwards"""
    if name not in _made:
        _made[name] = (CASES.get(name) or LOOP_CASES[name])()
    return _made[name]


def in_group(name, letters):
    return name[0] in letters


# ------------------------------------------------------------------------------------------ what both tiers assert

# (kernel `t` against the brute force's.)  Triangles: the bounds of test_triangle_test_across_scales(_on_the_gpu), |dt| over
# |o| + |o - v0| + |e1| + |e2| + t.  Spheres and cuboids: the file-header tolerance of tests/test_gpu_parity.py, |dt| over max(1, t).
TRI_MAX, TRI_P90 = 2e-6, 1e-7
ROUND_P99, ROUND_MAX = 2e-5, 1e-3


def check_against_brute(case, got, gel, what):
    """hit flag on every ray; t within the bounds; the element the brute force's (on an equal-t tie: one it finds at that t)"""
    b = case.ref
    hit = got[:, 0] == 1
    assert np.array_equal(hit, b.hit), (case.name, what, "hit flags differ on rays", np.where(hit != b.hit)[0][:10])
    out = {}
    tri, rnd = b.hit & (b.kind == TRI), b.hit & (b.kind != TRI)
    if tri.any():
        err = np.abs(got[tri, 1].astype(np.float64) - b.t[tri]) / b.scale[tri]
        out["tri_max"], out["tri_p90"] = float(err.max()), float(np.quantile(err, 0.9))
    if rnd.any():
        err = np.abs(got[rnd, 1].astype(np.float64) - b.t[rnd]) / np.maximum(1.0, b.t[rnd])
        out["round_max"], out["round_p99"] = float(err.max()), float(np.quantile(err, 0.99))
    print("%s %s vs brute force: %s" % (case.name, what, ", ".join("%s %.3g" % kv for kv in sorted(out.items()))))
    assert out.get("tri_max", 0.0) < TRI_MAX and out.get("tri_p90", 0.0) < TRI_P90, (case.name, what, out)
    assert out.get("round_max", 0.0) < ROUND_MAX and out.get("round_p99", 0.0) < ROUND_P99, (case.name, what, out)
    for i in np.where(b.hit & (gel != b.elem))[0]:
        t = float(got[i, 1])
        tol = 4.0 * max(TRI_MAX * b.scale[i], EPS32 * max(1.0, t))
        assert int(gel[i]) in b.elements_at(i, b.t[i], tol), (case.name, what, "ray", int(i), "element", int(gel[i]), "brute force", int(b.elem[i]))
    return out


def check_same_hits(case, got, gel, base, base_el, what):
    """two trees over the same primitives: hit flag and t bit for bit; the element too, except on equal-t ties, where it is one the
    brute force finds at that t"""
    assert np.array_equal(got[:, 0], base[:, 0]), (case.name, what, "hit flags differ")
    assert np.array_equal(got[:, 1].view(np.uint32), base[:, 1].view(np.uint32)), (case.name, what, "t differs on rays", np.where(got[:, 1] != base[:, 1])[0][:10])
    b = case.ref
    for i in np.where(gel != base_el)[0]:
        tol = 4.0 * max(TRI_MAX * b.scale[i], EPS32 * max(1.0, b.t[i]))
        at = b.elements_at(i, b.t[i], tol)
        assert len(at) > 1 and int(gel[i]) in at, (case.name, what, "ray", int(i), "elements", int(gel[i]), int(base_el[i]), "tie", sorted(at)[:8])
