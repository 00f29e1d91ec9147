"""The post-processing core headers compiled for the host: tests/post_harness.cpp built once per process with g++, its entries bound from one
table, and the wrappers that run them over numpy arrays.  The CPU tests hold these against tests/post_numpy.py, the GPU tests and the quality
tools hold the device against these.

No GPU in this module."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from post_numpy import DENOISE_DEFAULTS, RESTORE_DEFAULTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared"]

_P, _U32, _U64, _I, _D = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_double
_BUCKET_IMAGE = [_P, _P, _U64, _U32, _U64, _P, _P]                   # buckets, counts, n_all, K, pixels, two outputs
SIGNATURES = {
    "noise_batch": [_P, _P, _P, _I, _P],
    "lane_pixels": [_P, _P, _U32, _P],
    "tile_rule": [_P, _P, _P, _D, _D, _P],
    "pixel_errors": [_P, _P, _D, _I, _P],
    "default_params_mean_no_list": [],
    "denoise_run": [_P, _P, _P, _U32, _P, _U32, _U32, _U32, _I, _P, _P, _P],
    "denoise_one_level": [_P, _P, _U32, _U32, _U32, _P, _P],
    "robust_run": _BUCKET_IMAGE,
    "robust_k_ok": [_D],
    "robust_k_run": _BUCKET_IMAGE,
    "robust_error_run": [_P, _P, _U64, _U32, _D, _U64, _P, _P],
    "robust_cv_run": _BUCKET_IMAGE,
    "robust_denoise_run": [_P, _P, _U64, _U32, _P, _U32, _U32, _U32, _I, _P, _P, _P],
    "excess_run": _BUCKET_IMAGE,
    "restore_run": [_P, _P, _U64, _U32, _P, _U32, _U32, _U32, _P, _P, _P, _P],
    "spread_run": [_P, _P, _U32, _U32, _U32, _P, _P],
    "select_run": [_P, _U32, _P, _U32, _P, _P, _P, _U32, _U32, _U32, _I, _P, _U32, _P, _P, _P],
}
RETURNS_U32 = ("lane_pixels", "default_params_mean_no_list")         # every other entry returns int or nothing


@functools.lru_cache(maxsize=None)
def lib():
    """The harness as a ctypes.CDLL: one compile per process, whoever asks."""
    directory = tempfile.mkdtemp(prefix="post_harness_")
    atexit.register(shutil.rmtree, directory, ignore_errors=True)
    so = os.path.join(directory, "libpost_harness.so")
    subprocess.run(["g++"] + FLAGS + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "hanamaru-renderer_amd", "csrc"),
                    "-o", so, os.path.join(ROOT, "tests", "post_harness.cpp")], check=True)
    cdll = C.CDLL(so)
    for name, argtypes in SIGNATURES.items():
        getattr(cdll, name).argtypes = argtypes
    for name in RETURNS_U32:
        getattr(cdll, name).restype = C.c_uint32
    return cdll


@pytest.fixture(scope="module")
def core():
    return lib()


def sigmas(params, keys):
    return np.array([params[k] for k in keys], dtype=np.float64)


DENOISE_SIGMAS = ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth")
RESTORE_SIGMAS = ("sigma_n", "sigma_a", "sigma_z")


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _counts(n):
    """n: one count for every pixel, or an array of per-pixel counts -> (counts or None, its pointer, n_all)"""
    counts = None if np.isscalar(n) else np.ascontiguousarray(n, dtype=np.uint32)
    return counts, _ptr(counts), (int(n) if counts is None else 0)


def _image_args(buckets, n):
    b = np.ascontiguousarray(buckets, dtype=np.float64)
    K, shape = b.shape[-2], b.shape[:-2]
    assert b.shape[-1] == 3
    counts, cp, n_all = _counts(n)
    assert counts is None or counts.shape == shape
    return b, K, shape, int(np.prod(shape, dtype=np.int64)), cp, n_all


# ---- noise_core.h ----
def core_noise(lib, mom, n, floor):
    """noise_pixel_error over moments (.., 6) with one count and one floor, or one of each per pixel."""
    mom = np.ascontiguousarray(mom, dtype=np.float64).reshape(-1, 6)
    n = np.ascontiguousarray(np.broadcast_to(n, (mom.shape[0],)), dtype=np.uint64)
    floor = np.ascontiguousarray(np.broadcast_to(floor, (mom.shape[0],)), dtype=np.float64)
    out = np.empty(mom.shape[0], dtype=np.float64)
    lib.noise_batch(mom.ctypes.data, n.ctypes.data, floor.ctypes.data, mom.shape[0], out.ctypes.data)
    return out


# (adapt_core.h's entries lane_pixels, tile_rule, pixel_errors and default_params_mean_no_list take plain pointers: tests/test_adaptive_cpu.py
# calls them on the CDLL as they are)


# ---- denoise_core.h ----
def core_denoise(lib, acc, mom, n, guides, want_state=False, **over):
    """The host-compiled core over a whole image.  n: one count for every pixel, or an (h, w) array of counts."""
    params = dict(DENOISE_DEFAULTS, **over)
    acc = np.ascontiguousarray(acc, dtype=np.float32)
    mom = np.ascontiguousarray(mom, dtype=np.float64)
    guides = np.ascontiguousarray(guides, dtype=np.float32)
    h, w = acc.shape[:2]
    assert mom.shape == (h, w, 6) and guides.shape == (h, w, 8)
    counts, cp, n_all = _counts(n)
    d = np.zeros((h, w, 3), dtype=np.float32)
    state = np.zeros((h, w, 6), dtype=np.float64) if want_state else None
    sig = sigmas(params, DENOISE_SIGMAS)
    lib.denoise_run(acc.ctypes.data, mom.ctypes.data, cp, n_all, guides.ctypes.data, w, h, int(params["levels"]), int(params["demodulate"]), sig.ctypes.data,
                    d.ctypes.data, _ptr(state))
    return (d, state) if want_state else d


def core_one_level(lib, state, guides, step, **over):
    """denoise_level with the given step over an image of states (h, w, 6)"""
    h, w = state.shape[:2]
    sig = sigmas(dict(DENOISE_DEFAULTS, **over), DENOISE_SIGMAS)
    out = np.zeros_like(state)
    lib.denoise_one_level(state.ctypes.data, guides.ctypes.data, w, h, step, sig.ctypes.data, out.ctypes.data)
    return out


# ---- robust_core.h ----
def core_r(lib, buckets, n, templated=False):
    """robust_pixel (the run-time K definition) or robust_pixel_k<K> over buckets (.., K, 3).  n: one count for every pixel, or an array of per-pixel
    counts.  Returns (R float32 (.., 3), trim uint8 (..))."""
    b, K, shape, pixels, cp, n_all = _image_args(buckets, n)
    R, trim = np.zeros(shape + (3,), dtype=np.float32), np.zeros(shape, dtype=np.uint8)
    if templated:
        assert lib.robust_k_run(b.ctypes.data, cp, n_all, K, pixels, R.ctypes.data, trim.ctypes.data) == 0
    else:
        lib.robust_run(b.ctypes.data, cp, n_all, K, pixels, R.ctypes.data, trim.ctypes.data)
    return R, trim


def core_robust(lib, buckets, n):
    return core_r(lib, buckets, n, templated=False)


def core_error(lib, buckets, n, floor=0.01):
    """robust_error_image over buckets (.., K, 3); every count >= K.  Returns (e float64 (..), trim uint8 (..))."""
    b, K, shape, pixels, cp, n_all = _image_args(buckets, n)
    e, trim = np.zeros(shape), np.zeros(shape, dtype=np.uint8)
    lib.robust_error_run(b.ctypes.data, cp, n_all, K, float(floor), pixels, e.ctypes.data, trim.ctypes.data)
    return e, trim


core_e = core_error


def core_cv(lib, buckets, n):
    """robust_pixel_cv over buckets (.., K, 3); every count >= K.  Returns (cv float64 (.., 6), trim uint8 (..))."""
    b, K, shape, pixels, cp, n_all = _image_args(buckets, n)
    cv, trim = np.zeros(shape + (6,)), np.zeros(shape, dtype=np.uint8)
    lib.robust_cv_run(b.ctypes.data, cp, n_all, K, pixels, cv.ctypes.data, trim.ctypes.data)
    return cv, trim


def core_filter(lib, buckets, n, guides, want_state=False, **over):
    """robust_denoise_image over an (h, w, K, 3) image of buckets with the rule of hr_denoise_robust: demodulate only with levels > 0."""
    params = dict(DENOISE_DEFAULTS, **over)
    b, K, (h, w), _, cp, n_all = _image_args(buckets, n)
    guides = np.ascontiguousarray(guides, dtype=np.float32)
    assert guides.shape == (h, w, 8)
    d = np.zeros((h, w, 3), dtype=np.float32)
    state = np.zeros((h, w, 6)) if want_state else None
    sig = sigmas(params, DENOISE_SIGMAS)
    lib.robust_denoise_run(b.ctypes.data, cp, n_all, K, guides.ctypes.data, w, h, int(params["levels"]), int(params["demodulate"]), sig.ctypes.data,
                           d.ctypes.data, _ptr(state))
    return (d, state) if want_state else d


# ---- restore_core.h ----
def core_excess(lib, buckets, n):
    """robust_pixel_excess over buckets (.., K, 3).  Returns (cx float64 (.., 6), trim uint8 (..))."""
    b, K, shape, pixels, cp, n_all = _image_args(buckets, n)
    cx, trim = np.zeros(shape + (6,)), np.zeros(shape, dtype=np.uint8)
    lib.excess_run(b.ctypes.data, cp, n_all, K, pixels, cx.ctypes.data, trim.ctypes.data)
    return cx, trim


def core_restore(lib, buckets, n, guides, D=None, want_x=False, **over):
    """restore_image over an (h, w, K, 3) image of buckets; D: the base of base 1 (h, w, 3) float32."""
    params = dict(RESTORE_DEFAULTS, **over)
    b, K, (h, w), _, cp, n_all = _image_args(buckets, n)
    guides = np.ascontiguousarray(guides, dtype=np.float32)
    assert guides.shape == (h, w, 8) and (D is not None) == bool(params["base"])
    if D is not None:
        D = np.ascontiguousarray(D, dtype=np.float32)
        assert D.shape == (h, w, 3)
    r = np.zeros((h, w, 3), dtype=np.float32)
    x = np.zeros((h, w, 3)) if want_x else None
    sig = sigmas(params, RESTORE_SIGMAS)
    lib.restore_run(b.ctypes.data, cp, n_all, K, guides.ctypes.data, w, h, int(params["levels"]), sig.ctypes.data, _ptr(D), r.ctypes.data, _ptr(x))
    return (r, x) if want_x else r


def core_spread(lib, X, guides, **over):
    params = dict(RESTORE_DEFAULTS, **over)
    X = np.ascontiguousarray(X, dtype=np.float64)
    h, w = X.shape[:2]
    guides = np.ascontiguousarray(guides, dtype=np.float32)
    assert guides.shape == (h, w, 8) and X.shape == (h, w, 3)
    out = np.zeros((h, w, 3))
    sig = sigmas(params, RESTORE_SIGMAS)
    lib.spread_run(X.ctypes.data, guides.ctypes.data, w, h, int(params["levels"]), sig.ctypes.data, out.ctypes.data)
    return out


# ---- select_core.h ----
def core_select(lib, buckets, acc, mom, n, guides, smooth=0, want_states=False, **over):
    """select_image over an (h, w, K, 3) image of buckets.  n: one count for every pixel, or an (h, w) array.  Returns (S, L[, states (3, h, w, 6)])."""
    params = dict(DENOISE_DEFAULTS, **over)
    b = np.ascontiguousarray(buckets, dtype=np.float64)
    h, w, K = b.shape[:3]
    acc = np.ascontiguousarray(acc, dtype=np.float32)
    mom = np.ascontiguousarray(mom, dtype=np.float64)
    guides = np.ascontiguousarray(guides, dtype=np.float32)
    assert acc.shape == (h, w, 3) and mom.shape == (h, w, 6) and guides.shape == (h, w, 8) and b.shape[3] == 3
    counts, cp, n_all = _counts(n)
    S, L = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w), dtype=np.uint8)
    states = np.zeros((3, h, w, 6)) if want_states else None
    sig = sigmas(params, DENOISE_SIGMAS)
    lib.select_run(b.ctypes.data, K, cp, n_all, acc.ctypes.data, mom.ctypes.data, guides.ctypes.data, w, h, int(params["levels"]), int(params["demodulate"]),
                   sig.ctypes.data, int(smooth), S.ctypes.data, L.ctypes.data, _ptr(states))
    return (S, L, states) if want_states else (S, L)
