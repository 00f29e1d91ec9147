"""ctypes plumbing over the two C-ABI libraries of the MI355X hanamaru back end.

  libhanamaru_host.so  — scene authoring / asset IO (include/hanamaru_host.h)
  libhanamaru_hip.so   — the HIP render path      (include/hanamaru_hip.h)

This module holds no algorithm: it mirrors the C structs and forwards calls.  The HIP library is
required for anything that renders — there is no CPU fallback (`Renderer` raises if it cannot load).
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.normpath(os.path.join(_HERE, "..", ".."))
REPO_ROOT = os.path.normpath(os.path.join(PKG_ROOT, ".."))
ASSET_ROOT = os.path.join(REPO_ROOT, "assets")
HOST_LIB = os.path.join(PKG_ROOT, "libhanamaru_host.so")
HIP_LIB = os.path.join(PKG_ROOT, "libhanamaru_hip.so")

HR_OK = 0
HR_ERR_RNG_WINDOW = -5
DIFFUSE, SPECULAR, REFRACTION, GGX, GGX_REFRACTION = range(5)
SPHERE, CUBOID, MESH = range(3)


class Vec3(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]

    def tuple(self):
        return (self.x, self.y, self.z)


class Texture(C.Structure):
    _fields_ = [("color", Vec3), ("image", C.c_int32), ("_pad", C.c_int32)]


class Material(C.Structure):
    _fields_ = [("surface", C.c_int32), ("_pad", C.c_int32), ("param", C.c_double),
                ("albedo", Texture), ("emission", Texture), ("roughness", Texture)]


class Image(C.Structure):
    _fields_ = [("rgba", C.POINTER(C.c_uint8)), ("width", C.c_uint32), ("height", C.c_uint32)]


class Element(C.Structure):
    _fields_ = [("kind", C.c_int32), ("_pad", C.c_int32), ("material", Material),
                ("center", Vec3), ("radius", C.c_double),
                ("aabb_min", Vec3), ("aabb_max", Vec3),
                ("vertexes", C.POINTER(Vec3)), ("num_vertexes", C.c_uint64),
                ("faces", C.POINTER(C.c_uint64)), ("num_faces", C.c_uint64)]


class Camera(C.Structure):
    _fields_ = [("eye", Vec3), ("right", Vec3), ("up", Vec3), ("forward", Vec3),
                ("plane_half_right", Vec3), ("plane_half_up", Vec3),
                ("lens_radius", C.c_double), ("focus_distance", C.c_double),
                ("lens_shape", C.c_int32), ("_pad", C.c_int32)]


class Skybox(C.Structure):
    _fields_ = [("face_image", C.c_int32 * 6), ("intensity", Vec3)]


class SceneDesc(C.Structure):
    _fields_ = [("elements", C.POINTER(Element)), ("num_elements", C.c_uint32),
                ("images", C.POINTER(Image)), ("num_images", C.c_uint32),
                ("skybox", Skybox), ("camera", Camera)]


class CommInfo(C.Structure):
    _fields_ = [("path", C.c_int32), ("nranks", C.c_int32), ("rank", C.c_int32), ("device", C.c_int32),
                ("rccl_version", C.c_int32), ("_pad", C.c_int32), ("allreduces", C.c_uint64)]


class Noise(C.Structure):
    _fields_ = [("samplings", C.c_uint64), ("pixels", C.c_uint64), ("pixels_above", C.c_uint64),
                ("mean_error", C.c_double), ("max_error", C.c_double)]


class DenoiseParams(C.Structure):
    _fields_ = [("levels", C.c_uint32), ("demodulate", C.c_uint32),
                ("sigma_color", C.c_double), ("sigma_normal", C.c_double), ("sigma_albedo", C.c_double), ("sigma_depth", C.c_double)]


class RestoreParams(C.Structure):
    _fields_ = [("levels", C.c_uint32), ("base", C.c_uint32), ("sigma_n", C.c_double), ("sigma_a", C.c_double), ("sigma_z", C.c_double)]


class SelectParams(C.Structure):
    _fields_ = [("smooth", C.c_uint32), ("reserved", C.c_uint32)]


class ReprojectParams(C.Structure):
    _fields_ = [("max_history", C.c_uint32), ("_pad", C.c_uint32), ("min_roughness", C.c_double), ("depth_tolerance", C.c_double)]


COMM_PATHS = {0: "none", 1: "rccl-rank", 2: "rccl-group", 3: "same-device-fallback"}


class Stats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("rays", C.c_uint64), ("node_tests", C.c_uint64),
                ("tri_tests", C.c_uint64), ("sphere_tests", C.c_uint64), ("cuboid_tests", C.c_uint64),
                ("rng_overflow", C.c_uint64),
                ("seed_kernel_ms", C.c_double), ("trace_kernel_ms", C.c_double), ("post_kernel_ms", C.c_double),
                ("seed_launches", C.c_uint64), ("trace_launches", C.c_uint64),
                ("bvh_nodes", C.c_uint64), ("triangles", C.c_uint64), ("spheres", C.c_uint64), ("cuboids", C.c_uint64),
                ("shade_calls", C.c_uint64), ("shade_lanes", C.c_uint64), ("box_passes", C.c_uint64), ("box_lanes", C.c_uint64),
                ("leaf_calls", C.c_uint64), ("leaf_lanes", C.c_uint64), ("outer_iters", C.c_uint64), ("phase_cycles", C.c_uint64 * 4),
                ("bvh_build_ms", C.c_double), ("seed_phase_cycles", C.c_uint64 * 8),
                ("debug_kernel_ms", C.c_double), ("debug_launches", C.c_uint64),
                ("governor_level", C.c_uint64), ("governor_decisions", C.c_uint64), ("governor_moves", C.c_uint64), ("shadow_culled", C.c_uint64), ("governor_budget", C.c_uint64), ("governor_budget_moves", C.c_uint64), ("bvh_builder_used", C.c_uint64), ("shading_in_force", C.c_uint64)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if hasattr(getattr(self, k), "__len__") else getattr(self, k)) for k, _ in self._fields_}


_host = None
_hip = None


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise RuntimeError("libhanamaru_host.so not built — run __graft_entry__.build() / make -C hanamaru-renderer_amd")
        L = C.CDLL(HOST_LIB)
        L.hh_last_error.restype = C.c_char_p
        L.hh_scene_create.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
        L.hh_scene_desc.argtypes = [C.c_void_p]
        L.hh_scene_desc.restype = C.POINTER(SceneDesc)
        L.hh_scene_destroy.argtypes = [C.c_void_p]
        L.hh_decode_image.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.hh_write_png_rgb8.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.hh_load_obj.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.POINTER(Vec3)), C.POINTER(C.c_uint64),
                                  C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64)]
        L.hh_free.argtypes = [C.c_void_p]
        L.hh_debug_isaac64.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.c_int]
        L.hh_camera_new.argtypes = [Vec3, Vec3, Vec3, C.c_double, C.c_int32, C.c_double, C.c_double, C.POINTER(Camera)]
        _host = L
    return _host


def hip_lib():
    """Load the HIP back end.  Fails loudly: there is no fallback path."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB):
            raise RuntimeError("libhanamaru_hip.so not built — run __graft_entry__.build() / make -C hanamaru-renderer_amd")
        # One HIP runtime per process: PyTorch ships its own libamdhip64.  Loaded after this library's (the system's, through DT_NEEDED)
        # it becomes a second runtime that finds no GPU ("No HIP GPUs are available"); loaded first, its SONAME satisfies this
        # library's dependency and both share it.  A process that will use torch next to this wrapper (bench.py binds torch tensors and
        # torch.distributed; some tests do) must therefore have torch loaded before the first CDLL below — do it here, once.
        if "torch" not in sys.modules:
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(HIP_LIB)
        L.hr_last_error.restype = C.c_char_p
        L.hr_abi_version.restype = C.c_int
        L.hr_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.hr_destroy.argtypes = [C.c_void_p]
        L.hr_upload_scene.argtypes = [C.c_void_p, C.POINTER(SceneDesc)]
        L.hr_set_resolution.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.hr_bind_accumulator.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_set_region.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        L.hr_get_region.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.hr_accumulator_device_ptr.argtypes = [C.c_void_p]
        L.hr_accumulator_device_ptr.restype = C.c_void_p
        L.hr_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_clear.argtypes = [C.c_void_p]
        L.hr_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        L.hr_synchronize.argtypes = [C.c_void_p]
        L.hr_mark.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.hr_wait.argtypes = [C.c_void_p, C.c_uint64]
        L.hr_render_debug.argtypes = [C.c_void_p, C.c_int]
        L.hr_read_accumulator.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_write_accumulator.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_resolve.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.hr_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
        L.hr_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        L.hr_set_debug_option.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        L.hr_debug_trace.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hr_debug_draws.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.hr_debug_intersect.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hr_debug_surface.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hr_debug_sky.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hr_debug_texture.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hr_debug_path_log.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.hr_debug_path_draws.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.hr_debug_path_draw_residuals.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.hr_debug_wf_profile.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.hr_comm_get_unique_id.argtypes = [C.c_void_p]
        L.hr_comm_init_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.hr_comm_init_local.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.hr_comm_destroy.argtypes = [C.c_void_p]
        L.hr_allreduce_accumulator.argtypes = [C.c_void_p]
        L.hr_allreduce_accumulators.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.hr_total_device_ptr.argtypes = [C.c_void_p]
        L.hr_total_device_ptr.restype = C.c_void_p
        L.hr_comm_info.argtypes = [C.c_void_p, C.POINTER(CommInfo)]
        L.hr_accumulator_sum.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
        L.hr_read_moments.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.hr_write_moments.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.hr_noise_estimate.argtypes = [C.c_void_p, C.c_double, C.c_double, C.POINTER(Noise)]
        L.hr_read_noise_image.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        L.hr_read_sample_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_write_sample_counts.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_resolve_counted.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_set_tile_mask.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_get_tile_mask.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        L.hr_select_tiles.argtypes = [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_uint32)]
        L.hr_denoise_default_params.argtypes = [C.POINTER(DenoiseParams)]
        L.hr_render_guides.argtypes = [C.c_void_p]
        L.hr_render_guides_lens.argtypes = [C.c_void_p, C.c_uint32]
        L.hr_guide_lens_points.argtypes = [C.c_int, C.c_uint32, C.c_void_p]
        L.hr_read_guides.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_write_guides.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_denoise.argtypes = [C.c_void_p, C.POINTER(DenoiseParams)]
        L.hr_read_denoised.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_resolve_denoised.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_read_buckets.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.hr_write_buckets.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.hr_robust.argtypes = [C.c_void_p]
        L.hr_read_robust.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_read_robust_trim.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_resolve_robust.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_robust_noise_estimate.argtypes = [C.c_void_p, C.c_double, C.c_double, C.POINTER(Noise)]
        L.hr_read_robust_noise_image.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        L.hr_read_robust_noise_trim.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        L.hr_select_tiles_robust.argtypes = [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_uint32)]
        L.hr_denoise_robust.argtypes = [C.c_void_p, C.POINTER(DenoiseParams)]
        L.hr_restore_default_params.argtypes = [C.POINTER(RestoreParams)]
        L.hr_robust_restore.argtypes = [C.c_void_p, C.POINTER(RestoreParams)]
        L.hr_read_restored.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_resolve_restored.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_select_default_params.argtypes = [C.POINTER(SelectParams)]
        L.hr_denoise_select.argtypes = [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(SelectParams)]
        L.hr_read_selected.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_read_selected_levels.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_resolve_selected.argtypes = [C.c_void_p, C.c_void_p]
        _sel = [C.c_void_p, C.POINTER(DenoiseParams), C.POINTER(SelectParams)]
        L.hr_selected_noise_estimate.argtypes = _sel + [C.c_double, C.c_double, C.POINTER(Noise)]
        L.hr_read_selected_noise_image.argtypes = _sel + [C.c_double, C.c_void_p]
        L.hr_read_selected_mse.argtypes = _sel + [C.c_void_p]
        L.hr_select_tiles_selected.argtypes = _sel + [C.c_double, C.c_double, C.POINTER(C.c_uint32)]
        L.hr_fold_statistics.argtypes = [C.c_void_p]
        L.hr_fold_statistics_group.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        L.hr_set_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
        L.hr_get_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
        L.hr_render_motion.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(ReprojectParams)]
        L.hr_read_motion.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_write_motion.argtypes = [C.c_void_p, C.c_void_p]
        L.hr_reproject_default_params.argtypes = [C.POINTER(ReprojectParams)]
        L.hr_reproject.argtypes = [C.c_void_p, C.POINTER(ReprojectParams)]
        _hip = L
    return _hip


def _ok(L, rc):
    if rc != 0:
        raise HipError(rc, L.hr_last_error().decode())


def _with(defaults_fn, struct, who, params):
    """defaults_fn()'s `struct` with the keywords `params` replaced; a keyword that is no field of it is who()'s TypeError"""
    p = defaults_fn()
    for k, v in params.items():
        if k not in dict(struct._fields_):
            raise TypeError("%s() has no parameter %r" % (who, k))
        setattr(p, k, v)
    return p


def _noise_dict(n):
    return {k: getattr(n, k) for k, _ in n._fields_}


def denoise_default_params():
    """hr_denoise_default_params: the documented defaults as a DenoiseParams (needs no device)."""
    L = hip_lib()
    p = DenoiseParams()
    _ok(L, L.hr_denoise_default_params(C.byref(p)))
    return p


COMM_ID_BYTES = 128


def comm_unique_id():
    """ncclGetUniqueId through the library: bytes to hand to every rank's Renderer.comm_init_rank."""
    L = hip_lib()
    buf = (C.c_char * COMM_ID_BYTES)()
    _ok(L, L.hr_comm_get_unique_id(buf))
    return bytes(buf)


def comm_library():
    """hr_comm_library: (path of the RCCL shared object the library's collective runs on, True when it reused one already mapped into the process)."""
    L = hip_lib()
    L.hr_comm_library.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]
    buf = C.create_string_buffer(4096)
    reused = C.c_int(0)
    _ok(L, L.hr_comm_library(buf, 4096, C.byref(reused)))
    return buf.value.decode(), bool(reused.value)


def comm_init_local(renderers):
    """One process driving several GPUs: ncclCommInitAll over the renderers' devices."""
    L = hip_lib()
    arr = (C.c_void_p * len(renderers))(*[r._h for r in renderers])
    _ok(L, L.hr_comm_init_local(arr, len(renderers)))


def allreduce_accumulators(renderers):
    L = hip_lib()
    arr = (C.c_void_p * len(renderers))(*[r._h for r in renderers])
    _ok(L, L.hr_allreduce_accumulators(arr, len(renderers)))


def fold_statistics(renderers):
    """hr_fold_statistics_group: the renderers of one comm_init_local group, in its order — accumulator, moments, sample counts and buckets
    (option bucket_by_sampling 1) of every renderer move to renderers[0], the others hold zeros; every renderer goes on rendering."""
    L = hip_lib()
    arr = (C.c_void_p * len(renderers))(*[r._h for r in renderers])
    rc = L.hr_fold_statistics_group(arr, len(renderers))
    if rc != 0:
        raise HipError(rc, L.hr_last_error().decode())


class HostError(RuntimeError):
    pass


def guide_lens_points(lens_shape, lens_points):
    """hr_guide_lens_points: the (lens_points, 2) float32 table of lens coordinates (u, v) that hr_render_guides_lens averages over, in the order
    it sums them; lens_shape 0 Square, 1 Circle; lens_points 4 or 16 (needs no device)."""
    L = hip_lib()
    uv = np.zeros((max(int(lens_points), 1), 2), dtype=np.float32)
    _ok(L, L.hr_guide_lens_points(int(lens_shape), int(lens_points), uv.ctypes.data))
    return uv


def select_default_params():
    """hr_select_default_params: the documented defaults as a SelectParams (needs no device)."""
    L = hip_lib()
    p = SelectParams()
    _ok(L, L.hr_select_default_params(C.byref(p)))
    return p


def reproject_default_params():
    """hr_reproject_default_params: the documented defaults as a ReprojectParams (needs no device)."""
    L = hip_lib()
    p = ReprojectParams()
    _ok(L, L.hr_reproject_default_params(C.byref(p)))
    return p


def restore_default_params():
    """hr_restore_default_params: the documented defaults as a RestoreParams (needs no device)."""
    L = hip_lib()
    p = RestoreParams()
    _ok(L, L.hr_restore_default_params(C.byref(p)))
    return p


class HipError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("hr error %d: %s" % (code, text))
        self.code = code


class Scene:
    """Owns an hh_scene (host memory) and exposes its hr_scene_desc."""

    def __init__(self, name, asset_root=ASSET_ROOT):
        L = host_lib()
        h = C.c_void_p()
        rc = L.hh_scene_create(name.encode(), asset_root.encode(), C.byref(h))
        if rc != 0:
            raise HostError("hh_scene_create(%s): %s" % (name, L.hh_last_error().decode()))
        self._h = h
        self.name = name
        self.desc_ptr = L.hh_scene_desc(h)
        self.desc = self.desc_ptr.contents

    def close(self):
        if self._h:
            host_lib().hh_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def image(self, i):
        im = self.desc.images[i]
        return np.ctypeslib.as_array(im.rgba, shape=(im.height, im.width, 4))


def decode_image(path):
    L = host_lib()
    p = C.POINTER(C.c_uint8)()
    w, h = C.c_uint32(), C.c_uint32()
    if L.hh_decode_image(path.encode(), C.byref(p), C.byref(w), C.byref(h)) != 0:
        raise HostError(L.hh_last_error().decode())
    arr = np.ctypeslib.as_array(p, shape=(h.value, w.value, 4)).copy()
    L.hh_free(p)
    return arr


def write_png(path, rgb8):
    a = np.ascontiguousarray(rgb8, dtype=np.uint8)
    if host_lib().hh_write_png_rgb8(path.encode(), a.ctypes.data, a.shape[1], a.shape[0]) != 0:
        raise HostError(host_lib().hh_last_error().decode())


def load_obj(path, matrix=None):
    L = host_lib()
    v, f = C.POINTER(Vec3)(), C.POINTER(C.c_uint64)()
    nv, nf = C.c_uint64(), C.c_uint64()
    m = None
    if matrix is not None:
        m = (C.c_double * 16)(*np.asarray(matrix, dtype=np.float64).reshape(16))
    if L.hh_load_obj(path.encode(), m, C.byref(v), C.byref(nv), C.byref(f), C.byref(nf)) != 0:
        raise HostError(L.hh_last_error().decode())
    verts = np.ctypeslib.as_array(C.cast(v, C.POINTER(C.c_double)), shape=(nv.value, 3)).copy()
    faces = np.ctypeslib.as_array(f, shape=(nf.value, 3)).copy()
    L.hh_free(v)
    L.hh_free(f)
    return verts, faces


# The planes a context hands out or takes in, per pixel of the region (hr_api.hip: PLANES): name -> (trailing shape, dtype).  "rgb8" is what
# every hr_resolve* writes; the buckets' trailing shape starts with the K in force and is passed by the caller.
_PLANES = {
    "accumulator": ((3,), np.float32), "rgb8": ((3,), np.uint8), "moments": ((6,), np.float64), "noise": ((), np.float64),
    "sample_counts": ((), np.uint32), "guides": ((8,), np.float32), "denoised": ((3,), np.float32), "buckets": ((3,), np.float64),
    "robust": ((3,), np.float32), "robust_trim": ((), np.uint8), "restored": ((3,), np.float32),
    "selected": ((3,), np.float32), "selected_levels": ((), np.uint8), "motion": ((4, 3), np.float32),
}


class Renderer:
    """Thin wrapper over hr_ctx — mirrors the reference's Renderer trait usage (renderer.rs:20-99):
    render() accumulates samplings, resolve() is update_imgbuf."""

    def __init__(self, device=0):
        self.L = hip_lib()
        h = C.c_void_p()
        self._check(self.L.hr_create(device, C.byref(h)))
        self._h = h
        self.width = self.height = 0
        self._region = None   # (x0, y0, w, h) set by set_region; None = the whole frame
        self._robust_k = 0    # option "robust_buckets" as last accepted

    def _check(self, rc):
        _ok(self.L, rc)

    def close(self):
        if getattr(self, "_h", None):
            self.L.hr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def upload_scene(self, scene):
        self._scene = scene  # keep host memory alive during the call
        self._check(self.L.hr_upload_scene(self._h, scene.desc_ptr))

    def set_resolution(self, w, h):
        self._check(self.L.hr_set_resolution(self._h, w, h))
        self.width, self.height = w, h
        self._region = None

    def set_region(self, x0, y0, w, h):
        """Render only the window [x0, x0+w) x [y0, y0+h) of the frame (include/hanamaru_hip.h: hr_set_region).  The accumulator becomes the
        window's, zeroed; read_accumulator / write_accumulator / resolve then take (h, w, 3) arrays.  (0, 0, width, height) is the whole frame."""
        self._check(self.L.hr_set_region(self._h, x0, y0, w, h))
        self._region = None if (w, h) == (self.width, self.height) else (x0, y0, w, h)

    def region(self):
        """The window in force as (x0, y0, w, h) — (0, 0, width, height) without a region."""
        out = (C.c_uint32 * 4)()
        self._check(self.L.hr_get_region(self._h, out))
        return tuple(out)

    def _acc_hw(self):
        return (self._region[3], self._region[2]) if self._region else (self.height, self.width)

    def _read_plane(self, fn, plane, *args, samplings=False, tail=None):
        """fn(ctx, *args, out[, &samplings]) into a fresh array of the plane's shape; with `samplings` the pair (array, samplings word)."""
        shape, dtype = _PLANES[plane]
        out = np.empty(self._acc_hw() + (shape if tail is None else tail), dtype=dtype)
        if not samplings:
            self._check(fn(self._h, *args, out.ctypes.data))
            return out
        n = C.c_uint64()
        self._check(fn(self._h, *args, out.ctypes.data, C.byref(n)))
        return out, int(n.value)

    def _write_plane(self, fn, plane, array, *args, tail=None):
        """fn(ctx, array, *args) of an array that must have the plane's shape."""
        shape, dtype = _PLANES[plane]
        a = np.ascontiguousarray(array, dtype=dtype)
        assert a.shape == self._acc_hw() + (shape if tail is None else tail)
        self._check(fn(self._h, a.ctypes.data, *args))

    def bind_accumulator(self, device_ptr):
        self._check(self.L.hr_bind_accumulator(self._h, device_ptr))

    def set_stream(self, stream_ptr):
        self._check(self.L.hr_set_stream(self._h, stream_ptr))

    def set_option(self, key, value):
        self._check(self.L.hr_set_option(self._h, key.encode(), float(value)))
        if key == "robust_buckets":   # the K the library accepted sizes read_buckets / write_buckets
            self._robust_k = int(value)

    def set_debug_option(self, key, value):
        """Measurement knobs (include/hanamaru_hip.h: hr_set_debug_option) — not for product code."""
        self._check(self.L.hr_set_debug_option(self._h, key.encode(), float(value)))

    def clear(self):
        self._check(self.L.hr_clear(self._h))

    def render(self, begin, end, stride=1):
        self._check(self.L.hr_render(self._h, begin, end, stride))

    def render_debug(self, mode):
        self._check(self.L.hr_render_debug(self._h, mode))

    def mark(self):
        t = C.c_uint64()
        self._check(self.L.hr_mark(self._h, C.byref(t)))
        return t.value

    def wait(self, ticket):
        self._check(self.L.hr_wait(self._h, C.c_uint64(ticket)))

    def synchronize(self):
        self._check(self.L.hr_synchronize(self._h))

    def read_accumulator(self):
        return self._read_plane(self.L.hr_read_accumulator, "accumulator")

    def write_accumulator(self, acc):
        self._write_plane(self.L.hr_write_accumulator, "accumulator", acc)

    def resolve(self, samplings_done):
        return self._read_plane(self.L.hr_resolve, "rgb8", samplings_done)

    def stats(self):
        s = Stats()
        self._check(self.L.hr_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    # ---- multi-GPU: one all-reduce of the accumulators over RCCL (include/hanamaru_hip.h)
    def comm_init_rank(self, unique_id, world_size, rank):
        buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._check(self.L.hr_comm_init_rank(self._h, buf, world_size, rank))

    def comm_destroy(self):
        self._check(self.L.hr_comm_destroy(self._h))

    def allreduce_accumulator(self):
        self._check(self.L.hr_allreduce_accumulator(self._h))

    def fold_statistics(self):
        """hr_fold_statistics: this rank's part of the fold into rank 0 (comm_init_rank: every rank calls it)."""
        self._check(self.L.hr_fold_statistics(self._h))

    def total_device_ptr(self):
        return self.L.hr_total_device_ptr(self._h)

    def comm_info(self):
        """hr_comm_info: what the communicator reports about itself (ncclCommCount, ncclCommUserRank, ncclCommCuDevice, ncclGetVersion)."""
        ci = CommInfo()
        self._check(self.L.hr_comm_info(self._h, C.byref(ci)))
        return {"path": COMM_PATHS.get(ci.path, "?"), "nranks": int(ci.nranks), "rank": int(ci.rank), "device": int(ci.device),
                "rccl_version": int(ci.rccl_version), "allreduces": int(ci.allreduces)}

    def accumulator_sum(self, total=False):
        """hr_accumulator_sum: per-channel f64 sums (device reduction) of this context's own accumulator, or of the all-reduced total."""
        out = (C.c_double * 3)()
        self._check(self.L.hr_accumulator_sum(self._h, 1 if total else 0, out))
        return [float(out[0]), float(out[1]), float(out[2])]

    # ---- option "moments": per-pixel sample moments and the noise estimate (include/hanamaru_hip.h)
    def read_moments(self):
        """hr_read_moments: ((h, w, 6) float64 array {S1r, S1g, S1b, S2r, S2g, S2b}, samplings behind them)."""
        return self._read_plane(self.L.hr_read_moments, "moments", samplings=True)

    def write_moments(self, moments, samplings):
        self._write_plane(self.L.hr_write_moments, "moments", moments, C.c_uint64(samplings))

    def noise_estimate(self, floor=0.01, threshold=0.05):
        """hr_noise_estimate: {samplings, pixels, pixels_above, mean_error, max_error} of the per-pixel relative standard error e."""
        n = Noise()
        self._check(self.L.hr_noise_estimate(self._h, float(floor), float(threshold), C.byref(n)))
        return _noise_dict(n)

    def noise_image(self, floor=0.01):
        """hr_read_noise_image: e of every pixel, (h, w) float64."""
        return self._read_plane(self.L.hr_read_noise_image, "noise", float(floor))

    # ---- adaptive sampling: option "sample_counts", the tile mask, the selection of tiles (include/hanamaru_hip.h)
    def _tiles_hw(self):
        h, w = self._acc_hw()
        return ((h + 3) // 4, (w + 3) // 4)

    def read_sample_counts(self):
        """hr_read_sample_counts: (h, w) uint32, the samplings every pixel has received."""
        return self._read_plane(self.L.hr_read_sample_counts, "sample_counts")

    def write_sample_counts(self, counts):
        self._write_plane(self.L.hr_write_sample_counts, "sample_counts", counts)

    def resolve_counted(self):
        """hr_resolve_counted: resolve() with every pixel's own count."""
        return self._read_plane(self.L.hr_resolve_counted, "rgb8")

    def set_tile_mask(self, mask):
        """hr_set_tile_mask: (tiles_y, tiles_x) array over the region's 4x4 tiles, nonzero = render; None removes the mask."""
        if mask is None:
            self._check(self.L.hr_set_tile_mask(self._h, None))
            return
        a = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        assert a.shape == self._tiles_hw()
        self._check(self.L.hr_set_tile_mask(self._h, a.ctypes.data))

    def tile_mask(self):
        """hr_get_tile_mask: ((tiles_y, tiles_x) uint8 mask in force — all ones without one —, active tiles)."""
        out = np.empty(self._tiles_hw(), dtype=np.uint8)
        n = C.c_uint32()
        self._check(self.L.hr_get_tile_mask(self._h, out.ctypes.data, C.byref(n)))
        return out, int(n.value)

    def select_tiles(self, floor=0.01, threshold=0.05):
        """hr_select_tiles: keep the tiles with a pixel whose e > threshold (ANDed with the mask in force); returns the active tiles left."""
        n = C.c_uint32()
        self._check(self.L.hr_select_tiles(self._h, float(floor), float(threshold), C.byref(n)))
        return int(n.value)

    # ---- guide planes and the denoiser (include/hanamaru_hip.h)
    def render_guides(self):
        """hr_render_guides: one pinhole pass into the guide planes (set_option("guide_bounces", K), K in 0 .. 8: through up to K mirrors and
        glass surfaces to the first rough hit; default 0, the first hit)."""
        self._check(self.L.hr_render_guides(self._h))

    def render_guides_lens(self, lens_points):
        """hr_render_guides_lens: render_guides with the planes averaged over lens_points (4 or 16) fixed points of the thin lens per sub-sample
        (guide_lens_points has the table); a camera without an aperture gets render_guides' planes."""
        self._check(self.L.hr_render_guides_lens(self._h, int(lens_points)))

    def read_guides(self):
        """hr_read_guides: (h, w, 8) float32 {albedo rgb, normal xyz, depth, coverage}."""
        return self._read_plane(self.L.hr_read_guides, "guides")

    def write_guides(self, guides):
        self._write_plane(self.L.hr_write_guides, "guides", guides)

    def denoise(self, **params):
        """hr_denoise: the defaults, with any of levels, demodulate, sigma_color, sigma_normal, sigma_albedo, sigma_depth replaced."""
        p = _with(denoise_default_params, DenoiseParams, "denoise", params)
        self._check(self.L.hr_denoise(self._h, C.byref(p)))

    def denoise_robust(self, **params):
        """hr_denoise_robust: denoise()'s filter on the robust radiance and its bucket-spread variance (option robust_buckets; no moments
        needed); D is read with read_denoised / resolve_denoised."""
        p = _with(denoise_default_params, DenoiseParams, "denoise_robust", params)
        self._check(self.L.hr_denoise_robust(self._h, C.byref(p)))

    def read_denoised(self):
        """hr_read_denoised: (h, w, 3) float32 radiance."""
        return self._read_plane(self.L.hr_read_denoised, "denoised")

    def resolve_denoised(self):
        """hr_resolve_denoised: resolve() of the denoised radiance."""
        return self._read_plane(self.L.hr_resolve_denoised, "rgb8")

    # ---- camera moves that keep their history (include/hanamaru_hip.h)
    def set_camera(self, camera):
        """hr_set_camera: replace the camera of the scene in place (a Camera); the tree, the textures and what is accumulated stay."""
        self._check(self.L.hr_set_camera(self._h, C.byref(camera)))

    def camera(self):
        """hr_get_camera: the f64 camera in place, as a Camera."""
        out = Camera()
        self._check(self.L.hr_get_camera(self._h, C.byref(out)))
        return out

    def render_motion(self, from_camera, **params):
        """hr_render_motion: the motion plane of the camera in place against the earlier camera `from_camera` (a Camera); the defaults, with any
        of min_roughness, depth_tolerance replaced."""
        p = _with(reproject_default_params, ReprojectParams, "render_motion", params)
        self._check(self.L.hr_render_motion(self._h, C.byref(from_camera), C.byref(p)))

    def read_motion(self):
        """hr_read_motion: (h, w, 4, 3) float32 {mx, my, code} per sub-sample."""
        return self._read_plane(self.L.hr_read_motion, "motion")

    def write_motion(self, motion):
        self._write_plane(self.L.hr_write_motion, "motion", motion)

    def reproject(self, **params):
        """hr_reproject: the defaults, with any of max_history, min_roughness, depth_tolerance replaced."""
        p = _with(reproject_default_params, ReprojectParams, "reproject", params)
        self._check(self.L.hr_reproject(self._h, C.byref(p)))

    # ---- option "robust_buckets": the sample buckets and the firefly-robust resolve (include/hanamaru_hip.h)
    def read_buckets(self):
        """hr_read_buckets: ((h, w, K, 3) float64 bucket sums — K from the size the library reports for the option —, samplings behind them)."""
        return self._read_plane(self.L.hr_read_buckets, "buckets", samplings=True, tail=(max(self._robust_k, 1), 3))

    def write_buckets(self, buckets, samplings):
        self._write_plane(self.L.hr_write_buckets, "buckets", buckets, C.c_uint64(samplings), tail=(self._robust_k, 3))

    def robust(self):
        """hr_robust: the robust radiance R and its trim plane from the buckets."""
        self._check(self.L.hr_robust(self._h))

    def read_robust(self):
        """hr_read_robust: (h, w, 3) float32 radiance."""
        return self._read_plane(self.L.hr_read_robust, "robust")

    def read_robust_trim(self):
        """hr_read_robust_trim: (h, w) uint8, the buckets dropped at either end."""
        return self._read_plane(self.L.hr_read_robust_trim, "robust_trim")

    def resolve_robust(self):
        """hr_resolve_robust: resolve() of the robust radiance."""
        return self._read_plane(self.L.hr_resolve_robust, "rgb8")

    # ---- the restored robust resolve (include/hanamaru_hip.h)
    def robust_restore(self, **params):
        """hr_robust_restore: R' = base + the trimmed buckets' excess spread along the guide planes; the defaults, with any of levels, base,
        sigma_n, sigma_a, sigma_z replaced (base 1: on top of the D of denoise_robust())."""
        p = _with(restore_default_params, RestoreParams, "robust_restore", params)
        self._check(self.L.hr_robust_restore(self._h, C.byref(p)))

    def read_restored(self):
        """hr_read_restored: (h, w, 3) float32 radiance."""
        return self._read_plane(self.L.hr_read_restored, "restored")

    def resolve_restored(self):
        """hr_resolve_restored: resolve() of the restored robust radiance."""
        return self._read_plane(self.L.hr_resolve_restored, "rgb8")

    # ---- the denoiser that picks its level per pixel (include/hanamaru_hip.h)
    def denoise_select(self, smooth=None, **params):
        """hr_denoise_select: S and its level plane L — hr_denoise's filter with the level picked per pixel from the held-out sample halves;
        the denoiser's defaults with any of levels, demodulate, sigma_* replaced, and `smooth` passes over the error planes (None: the default)."""
        self._check(self.L.hr_denoise_select(self._h, *self._select_args("denoise_select", smooth, params)))

    # ---- the error estimate of the selected radiance, and the selection of tiles by it (include/hanamaru_hip.h)
    @staticmethod
    def _select_args(who, smooth, params):
        """(DenoiseParams, SelectParams) by reference from denoise_select()'s keywords"""
        p = _with(denoise_default_params, DenoiseParams, who, params)
        s = select_default_params()
        if smooth is not None:
            s.smooth = smooth
        return C.byref(p), C.byref(s)

    def selected_noise_estimate(self, floor=0.01, threshold=0.05, smooth=None, **params):
        """hr_selected_noise_estimate: {samplings, pixels, pixels_above, mean_error, max_error} of e_S, the estimated relative error of the image
        denoise_select(smooth, **params) makes."""
        n = Noise()
        self._check(self.L.hr_selected_noise_estimate(self._h, *self._select_args("selected_noise_estimate", smooth, params), float(floor), float(threshold), C.byref(n)))
        return _noise_dict(n)

    def selected_noise_image(self, floor=0.01, smooth=None, **params):
        """hr_read_selected_noise_image: e_S of every pixel, (h, w) float64."""
        p, s = self._select_args("selected_noise_image", smooth, params)
        return self._read_plane(self.L.hr_read_selected_noise_image, "noise", p, s, float(floor))

    def selected_mse(self, smooth=None, **params):
        """hr_read_selected_mse: M of every pixel, (h, w) float64 — the estimated mean squared error of the selected radiance."""
        p, s = self._select_args("selected_mse", smooth, params)
        return self._read_plane(self.L.hr_read_selected_mse, "noise", p, s)

    def select_tiles_selected(self, floor=0.01, threshold=0.05, smooth=None, **params):
        """hr_select_tiles_selected: select_tiles() with e_S in place of e; returns the active tiles left."""
        n = C.c_uint32()
        self._check(self.L.hr_select_tiles_selected(self._h, *self._select_args("select_tiles_selected", smooth, params), float(floor), float(threshold), C.byref(n)))
        return int(n.value)

    def read_selected(self):
        """hr_read_selected: (h, w, 3) float32 radiance."""
        return self._read_plane(self.L.hr_read_selected, "selected")

    def read_selected_levels(self):
        """hr_read_selected_levels: (h, w) uint8, the level each pixel took."""
        return self._read_plane(self.L.hr_read_selected_levels, "selected_levels")

    def resolve_selected(self):
        """hr_resolve_selected: resolve() of the selected radiance."""
        return self._read_plane(self.L.hr_resolve_selected, "rgb8")

    # ---- the robust noise estimate of the buckets, and the selection of tiles by it (include/hanamaru_hip.h)
    def robust_noise_estimate(self, floor=0.01, threshold=0.05):
        """hr_robust_noise_estimate: {samplings, pixels, pixels_above, mean_error, max_error} of e_R, the winsorized relative error of R's channel sum."""
        n = Noise()
        self._check(self.L.hr_robust_noise_estimate(self._h, float(floor), float(threshold), C.byref(n)))
        return _noise_dict(n)

    def robust_noise_image(self, floor=0.01):
        """hr_read_robust_noise_image: e_R of every pixel, (h, w) float64."""
        return self._read_plane(self.L.hr_read_robust_noise_image, "noise", float(floor))

    def robust_noise_trim(self, floor=0.01):
        """hr_read_robust_noise_trim: (h, w) uint8, the trim the estimate took (read_robust_trim()'s values without a robust())."""
        return self._read_plane(self.L.hr_read_robust_noise_trim, "robust_trim", float(floor))

    def select_tiles_robust(self, floor=0.01, threshold=0.05):
        """hr_select_tiles_robust: select_tiles() with e_R in place of e; returns the active tiles left."""
        n = C.c_uint32()
        self._check(self.L.hr_select_tiles_robust(self._h, float(floor), float(threshold), C.byref(n)))
        return int(n.value)

    def debug_draws(self, sampling, first_path, num_paths, window):
        out = np.empty((num_paths, window), dtype=np.uint64)
        self._check(self.L.hr_debug_draws(self._h, sampling, first_path, num_paths, window, out.ctypes.data))
        return out

    def debug_path_log(self, sampling):
        """hr_debug_path_log: (radiance [H, W, 4, 3] float32, rays [H, W, 4] uint32, events [H, W, 4, 12] uint8 — nine event bytes, the count of sphere hits, the 16-bit texel-quad sum —, hash [H, W, 4] uint32) of every
        path of one sampling, from the render kernel's logging instantiation."""
        raw = np.zeros((self.height, self.width, 4, 8), dtype=np.uint32)
        self._check(self.L.hr_debug_path_log(self._h, sampling, raw.ctypes.data))
        rad = raw[..., 0:3].copy().view(np.float32)
        ev = np.ascontiguousarray(raw[..., 4:7]).view(np.uint8).reshape(self.height, self.width, 4, 12)[..., :12]
        return rad, raw[..., 3].copy(), ev.copy(), raw[..., 7].copy()

    def debug_wf_profile(self, sampling=1, num_k=4):
        """hr_debug_wf_profile: (ms[21], counts[11, 2]) of one launch of the split pipeline, kernel by kernel (ms[0] camera rays, ms[2s-1] / ms[2s]
        traversal / shading of step s; counts[s] = rays, live paths of step s)."""
        ms = np.zeros(21, dtype=np.float64)
        cn = np.zeros(22, dtype=np.uint32)
        self._check(self.L.hr_debug_wf_profile(self._h, sampling, num_k, ms.ctypes.data, cn.ctypes.data))
        return ms, cn.reshape(11, 2)

    def debug_intersect(self, rays):
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        out = np.empty((r.shape[0], 8), dtype=np.float32)
        el = np.empty((r.shape[0],), dtype=np.int32)
        self._check(self.L.hr_debug_intersect(self._h, r.shape[0], r.ctypes.data, out.ctypes.data, el.ctypes.data))
        return out, el

    def debug_trace(self, rays, shadow_len=None):
        """hr_debug_trace: the same queries through the render kernel's traversal; shadow_len > 0 marks shadow rays."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        out = np.empty((r.shape[0], 8), dtype=np.float32)
        el = np.empty((r.shape[0],), dtype=np.int32)
        sl = None
        if shadow_len is not None:
            sl = np.ascontiguousarray(shadow_len, dtype=np.float32).reshape(-1)
            assert sl.shape[0] == r.shape[0]
        self._check(self.L.hr_debug_trace(self._h, r.shape[0], r.ctypes.data, sl.ctypes.data if sl is not None else None, out.ctypes.data, el.ctypes.data))
        return out, el

    def debug_surface(self, rays, fix=None, draws=None, precise=False):
        """hr_debug_surface: (out [n, 24] float32, out64 [n, 6] float64, element [n] int32) — hanamaru_hip_debug.h has the record's layout."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = r.shape[0]
        f = None if fix is None else np.ascontiguousarray(fix, dtype=np.float32).reshape(n, 6)
        d = None if draws is None else np.ascontiguousarray(draws, dtype=np.float64).reshape(n, 2)
        out, out64, el = np.empty((n, 24), dtype=np.float32), np.empty((n, 6), dtype=np.float64), np.empty((n,), dtype=np.int32)
        self._check(self.L.hr_debug_surface(self._h, n, r.ctypes.data, None if f is None else f.ctypes.data, None if d is None else d.ctypes.data,
                                            1 if precise else 0, out.ctypes.data, out64.ctypes.data, el.ctypes.data))
        return out, out64, el

    def debug_sky(self, dirs):
        """hr_debug_sky: (rgb [n, 3] float32, where [n, 3] uint32 = {face + 8 on the footprint table's form, x1, y1})."""
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        rgb, where = np.empty((d.shape[0], 3), dtype=np.float32), np.empty((d.shape[0], 3), dtype=np.uint32)
        self._check(self.L.hr_debug_sky(self._h, d.shape[0], d.ctypes.data, rgb.ctypes.data, where.ctypes.data))
        return rgb, where

    def debug_texture(self, image, uv):
        """hr_debug_texture: (rgb [n, 3] float32, rough64 [n] float32, quad [n, 4] uint32 = the fp32 lookup's corner, the f64 read's corner)."""
        im = np.ascontiguousarray(image, dtype=np.int32).reshape(-1)
        c = np.ascontiguousarray(uv, dtype=np.float64).reshape(im.shape[0], 2)
        rgb, rough, quad = np.empty((im.shape[0], 3), dtype=np.float32), np.empty((im.shape[0],), dtype=np.float32), np.empty((im.shape[0], 4), dtype=np.uint32)
        self._check(self.L.hr_debug_texture(self._h, im.shape[0], im.ctypes.data, c.ctypes.data, rgb.ctypes.data, rough.ctypes.data, quad.ctypes.data))
        return rgb, rough, quad
