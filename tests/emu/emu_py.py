"""ctypes loader for tests/emu/libhr_emu.so (host emulation of the kernels' per-lane code; tests only)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhr_emu.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(LIB_PATH)
        L.emu_scene_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.emu_scene_destroy.argtypes = [C.c_void_p]
        L.emu_set_build_options.argtypes = [C.c_int, C.c_double, C.c_uint32]
        L.emu_last_ploc_loop.argtypes = [C.c_void_p]
        L.emu_set_builder.argtypes = [C.c_int]
        L.emu_set_walk_mode.argtypes = [C.c_int]
        L.emu_scene_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.emu_path_draws.argtypes = [C.c_uint32] * 6 + [C.c_int, C.c_void_p]
        L.emu_raw_draws.argtypes = [C.c_uint32] * 6 + [C.c_int, C.c_void_p]
        L.emu_raw_draws_split.argtypes = [C.c_uint32] * 6 + [C.c_int, C.c_void_p]
        L.emu_raw_draws_pc.argtypes = [C.c_uint32] * 6 + [C.c_int, C.c_int, C.c_void_p]
        L.emu_raw_draws_seg.argtypes = [C.c_uint32] * 6 + [C.c_int, C.c_void_p]
        L.emu_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        L.emu_render_wf.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        L.emu_path_log_wf.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        L.emu_set_wf_precise.argtypes = [C.c_int]
        L.emu_path_log.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        L.emu_render_debug.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        L.emu_intersect.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_trace.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_set_walk_mutant.argtypes = [C.c_int]
        L.emu_break_octant_planes.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.emu_shrink_qboxes.argtypes = [C.c_void_p, C.c_int]
        L.emu_surface.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_sky.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_texture.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.emu_resolve.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        _lib = L
    return _lib


class EmuScene:
    def __init__(self, desc_ptr):
        h = C.c_void_p()
        rc = lib().emu_scene_create(C.cast(desc_ptr, C.c_void_p), C.byref(h))
        if rc != 0:
            raise RuntimeError("emu_scene_create failed: %d" % rc)
        self._h = h

    def __del__(self):
        try:
            if self._h:
                lib().emu_scene_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def stats(self):
        out = (C.c_uint64 * 7)()
        lib().emu_scene_stats(self._h, out)
        return dict(zip(["nodes", "leaves", "max_depth", "tris", "spheres", "cuboids", "emitters"], list(out)))

    def render(self, w, h, s_begin, s_end, stride=1, threads=0, acc=None):
        if acc is None:
            acc = np.zeros((h, w, 3), dtype=np.float32)
        cn = (C.c_uint64 * 7)()
        lib().emu_render(self._h, w, h, s_begin, s_end, stride, threads, acc.ctypes.data, cn)
        return acc, dict(zip(["paths", "rays", "node_tests", "tri_tests", "sphere_tests", "cuboid_tests", "shadow_culled"], list(cn)))

    def render_wf(self, w, h, s_begin, s_end, stride=1, threads=0):
        """the split pipeline's per-lane functions (csrc/wf_core.h), path by path"""
        acc = np.zeros((h, w, 3), dtype=np.float32)
        lib().emu_render_wf(self._h, w, h, s_begin, s_end, stride, threads, acc.ctypes.data)
        return acc

    def path_log_wf(self, w, h, sampling, threads=0):
        """path_log's layout from the split pipeline with PRECISE shading (wf_surface_f64)"""
        raw = np.zeros((h, w, 4, 8), dtype=np.uint32)
        lib().emu_path_log_wf(self._h, w, h, sampling, threads, raw.ctypes.data)
        rad = raw[..., 0:3].copy().view(np.float32)
        ev = np.ascontiguousarray(raw[..., 4:7]).view(np.uint8).reshape(h, w, 4, 12)[..., :12]
        return rad, raw[..., 3].copy(), ev.copy(), raw[..., 7].copy()

    def path_log(self, w, h, sampling, threads=0):
        """(radiance [h, w, 4, 3] float32, rays, events [h, w, 4, 12] uint8 (nine event bytes, the count of sphere hits, the 16-bit texel-quad sum), element hash) — the layout of Renderer.debug_path_log"""
        raw = np.zeros((h, w, 4, 8), dtype=np.uint32)
        lib().emu_path_log(self._h, w, h, sampling, threads, raw.ctypes.data)
        rad = raw[..., 0:3].copy().view(np.float32)
        ev = np.ascontiguousarray(raw[..., 4:7]).view(np.uint8).reshape(h, w, 4, 12)[..., :12]
        return rad, raw[..., 3].copy(), ev.copy(), raw[..., 7].copy()

    def one_path(self, w, h, x, y, sub, sampling):
        """radiance of ONE path (fp32 or precise shading as set_precise says)"""
        out = np.zeros(3, dtype=np.float32)
        lib().emu_one_path.argtypes = [C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p]
        lib().emu_one_path(self._h, w, h, x, y, sub, sampling, out.ctypes.data)
        return out

    def render_debug(self, w, h, mode):
        acc = np.zeros((h, w, 3), dtype=np.float32)
        lib().emu_render_debug(self._h, w, h, mode, acc.ctypes.data)
        return acc

    def intersect(self, rays):
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        out = np.empty((r.shape[0], 8), dtype=np.float32)
        el = np.empty((r.shape[0],), dtype=np.int32)
        lib().emu_intersect(self._h, r.shape[0], r.ctypes.data, out.ctypes.data, el.ctypes.data)
        return out, el

    def trace(self, rays, shadow_len=None):
        """Renderer.debug_trace's twin (emu_trace): shadow_len > 0 marks shadow queries (limit shadow_len + 0.03f, shadow_early_out after every
        leaf), on the walk set_walk_mode chose"""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        sl = None if shadow_len is None else np.ascontiguousarray(shadow_len, dtype=np.float32).reshape(r.shape[0])
        out = np.empty((r.shape[0], 8), dtype=np.float32)
        el = np.empty((r.shape[0],), dtype=np.int32)
        rc = lib().emu_trace(self._h, r.shape[0], r.ctypes.data, None if sl is None else sl.ctypes.data, out.ctypes.data, el.ctypes.data)
        assert rc == 0
        return out, el

    def break_octant_planes(self, octant, axis):
        """a deliberately wrong tree: one octant's copy with the near and far planes of one axis exchanged, in both record formats"""
        assert lib().emu_break_octant_planes(self._h, octant, axis) == 0

    def shrink_qboxes(self, steps=2):
        """a deliberately wrong tree: every quantised box `steps` grid steps smaller on each side"""
        assert lib().emu_shrink_qboxes(self._h, steps) == 0

    # the twins of Renderer.debug_surface / debug_sky / debug_texture (csrc/query_core.h on the host): same arguments, same results
    def debug_surface(self, rays, fix=None, draws=None, precise=False):
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = r.shape[0]
        f = None if fix is None else np.ascontiguousarray(fix, dtype=np.float32).reshape(n, 6)
        d = None if draws is None else np.ascontiguousarray(draws, dtype=np.float64).reshape(n, 2)
        out, out64, el = np.empty((n, 24), dtype=np.float32), np.empty((n, 6), dtype=np.float64), np.empty((n,), dtype=np.int32)
        lib().emu_surface(self._h, n, r.ctypes.data, None if f is None else f.ctypes.data, None if d is None else d.ctypes.data, 1 if precise else 0,
                          out.ctypes.data, out64.ctypes.data, el.ctypes.data)
        return out, out64, el

    def sky_form(self):
        """1: the sky lookup goes through the footprint table (six faces of one size); 0: the per-face form"""
        lib().emu_sky_form.argtypes = [C.c_void_p]
        return int(lib().emu_sky_form(self._h))

    def break_sky_quads(self):
        """a deliberately wrong footprint table: its last corner column takes the texels of column w - 2 (the sweeps must notice)"""
        lib().emu_break_sky_quads.argtypes = [C.c_void_p]
        assert lib().emu_break_sky_quads(self._h) == 0

    def debug_sky(self, dirs):
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        rgb, where = np.empty((d.shape[0], 3), dtype=np.float32), np.empty((d.shape[0], 3), dtype=np.uint32)
        lib().emu_sky(self._h, d.shape[0], d.ctypes.data, rgb.ctypes.data, where.ctypes.data)
        return rgb, where

    def debug_texture(self, image, uv):
        im = np.ascontiguousarray(image, dtype=np.int32).reshape(-1)
        c = np.ascontiguousarray(uv, dtype=np.float64).reshape(im.shape[0], 2)
        rgb, rough, quad = np.empty((im.shape[0], 3), dtype=np.float32), np.empty((im.shape[0],), dtype=np.float32), np.empty((im.shape[0], 4), dtype=np.uint32)
        rc = lib().emu_texture(self._h, im.shape[0], im.ctypes.data, c.ctypes.data, rgb.ctypes.data, rough.ctypes.data, quad.ctypes.data)
        assert rc == 0
        return rgb, rough, quad


PLOC_TOP_DEFAULT = 8192   # lbvh_core.h PLOC_TOP_CLUSTERS


def set_build_options(max_leaf=4, split_ratio=-1.0, builder=0, ploc_top=PLOC_TOP_DEFAULT):
    """builder: 0 = host SAH, 1 = LBVH, 2 = PLOC (the device builders' per-thread code, run sequentially); ploc_top: the library's
    debug option of that name (builder 2: the merges stop at <= ploc_top clusters, 1 = merge to the root)."""
    lib().emu_set_build_options(max_leaf, split_ratio, ploc_top)
    lib().emu_set_builder(builder)


def last_ploc_loop():
    """(merge iterations, clusters handed to the top-down build) of the last PLOC build"""
    out = (C.c_uint32 * 2)()
    lib().emu_last_ploc_loop(out)
    return int(out[0]), int(out[1])


def set_walk_mode(mode):
    """0 = node + leaf per visit, 1 = the trace kernel's postponed-leaf schedule, 2 = that schedule on the 16-byte quantised
    nodes (EmuScene.intersect)."""
    lib().emu_set_walk_mode(mode)


WALK_MUTANT_DROP_SECOND_LEAF, WALK_MUTANT_BARE_SHADOW_LIMIT = 1, 2


def set_walk_mutant(bits):
    """a deliberately wrong walk for EmuScene.trace / intersect (0 = the walk as it is): bit 0 drops the newer of two parked leaves, bit 1 takes
    a shadow query's search limit as shadow_len instead of shadow_len + 0.03f"""
    lib().emu_set_walk_mutant(bits)


def set_draw_residuals(on):
    """precise shading with (default, as the library renders) or without the records' twin of draw residuals (isaac_core.h draw_lo_f32)"""
    lib().emu_set_draw_residuals.argtypes = [C.c_int]
    lib().emu_set_draw_residuals(1 if on else 0)


def set_precise(on):
    """option precise_shading for render / path_log (the megakernel's per-lane code, path_advance<.., PREC>)"""
    lib().emu_set_precise.argtypes = [C.c_int]
    lib().emu_set_precise(1 if on else 0)


def set_nee_cull(on):
    """nee_setup's shortcuts (pt_core.h): shadow rays known to add nothing are not traced (default on)."""
    lib().emu_set_nee_cull.argtypes = [C.c_int]
    lib().emu_set_nee_cull(7 if on is True else int(on))


def last_node_tests():
    lib().emu_last_node_tests.restype = C.c_uint64
    return int(lib().emu_last_node_tests())


def path_draws(w, h, x, y, sub, sampling, lens_shape=1):
    out = np.empty(20, dtype=np.float32)
    rc = lib().emu_path_draws(w, h, x, y, sub, sampling, lens_shape, out.ctypes.data)
    return out, rc == 0


def path_draw_residuals(w, h, x, y, sub, sampling, lens_shape=1):
    """the record's twin (precise shading): f64 draw k of the path = float(draw k) + residual k to 2^-49; [0], [1] belong to the raw lens draws"""
    out = np.empty(20, dtype=np.float32)
    lib().emu_path_draw_residuals.argtypes = [C.c_uint32] * 6 + [C.c_int, C.c_void_p]
    rc = lib().emu_path_draw_residuals(w, h, x, y, sub, sampling, lens_shape, out.ctypes.data)
    return out, rc == 0


def raw_draws(w, h, x, y, sub, sampling, window=64):
    out = np.empty(window, dtype=np.uint64)
    lib().emu_raw_draws(w, h, x, y, sub, sampling, window, out.ctypes.data)
    return out


def raw_draws_split(w, h, x, y, sub, sampling, window=64):
    out = np.empty(window, dtype=np.uint64)
    lib().emu_raw_draws_split(w, h, x, y, sub, sampling, window, out.ctypes.data)
    return out


def raw_draws_seg(w, h, x, y, sub, sampling, window=64):
    out = np.empty(window, dtype=np.uint64)
    rc = lib().emu_raw_draws_seg(w, h, x, y, sub, sampling, window, out.ctypes.data)
    assert rc == 0
    return out


def raw_draws_pc(w, h, x, y, sub, sampling, head, window=64):
    out = np.empty(window, dtype=np.uint64)
    rc = lib().emu_raw_draws_pc(w, h, x, y, sub, sampling, window, head, out.ctypes.data)
    assert rc == 0
    return out


def resolve(acc, samplings):
    a = np.ascontiguousarray(acc, dtype=np.float32)
    h, w, _ = a.shape
    out = np.empty((h, w, 3), dtype=np.uint8)
    lib().emu_resolve(a.ctypes.data, w, h, samplings, out.ctypes.data)
    return out
