"""csrc/select_noise_core.h compiled for the host: tests/select_noise_harness.cpp built once per process with g++, the way post_cores.lib() builds
tests/post_harness.cpp, and the wrappers that run its entries over numpy arrays.  The CPU tests hold these against tests/select_noise_numpy.py, the
GPU tests and tools/select_noise_quality.py hold the device against these.

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

from post_cores import DENOISE_SIGMAS, FLAGS, ROOT, _counts, sigmas
from post_numpy import DENOISE_DEFAULTS

_P, _U32, _U64, _I, _D = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_double
SIGNATURES = {
    "select_noise_run": [_P, _U32, _P, _U32, _P, _P, _P, _U32, _U32, _U32, _I, _P, _U32, _P, _P, _P],
    "select_noise_errors": [_P, _P, _D, _U64, _P],
    "select_noise_tile_rule": [_P, _U32, _U32, _D, _P],
}


@functools.lru_cache(maxsize=None)
def lib():
    """The harness as a ctypes.CDLL: one compile per process, whoever asks."""
    directory = tempfile.mkdtemp(prefix="select_noise_harness_")
    atexit.register(shutil.rmtree, directory, ignore_errors=True)
    so = os.path.join(directory, "libselect_noise_harness.so")
    subprocess.run(["g++"] + FLAGS + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "hanamaru-renderer_amd", "csrc"),
                    "-o", so, os.path.join(ROOT, "tests", "select_noise_harness.cpp")], check=True)
    cdll = C.CDLL(so)
    for name, argtypes in SIGNATURES.items():
        getattr(cdll, name).argtypes = argtypes
        getattr(cdll, name).restype = None
    return cdll


@pytest.fixture(scope="module")
def noise_core():
    return lib()


def core_select_noise(lib, buckets, acc, mom, n, guides, smooth=0, **over):
    """select_noise_image over an (h, w, K, 3) image of buckets.  n: one count for every pixel, or an (h, w) array.  Returns (S, L, M)."""
    params = dict(DENOISE_DEFAULTS, **over)
    b = np.ascontiguousarray(buckets, dtype=np.float64)
    h, w, K = b.shape[:3]
    acc = np.ascontiguousarray(acc, dtype=np.float32)
    mom = np.ascontiguousarray(mom, dtype=np.float64)
    guides = np.ascontiguousarray(guides, dtype=np.float32)
    assert acc.shape == (h, w, 3) and mom.shape == (h, w, 6) and guides.shape == (h, w, 8) and b.shape[3] == 3
    counts, cp, n_all = _counts(n)
    S, L, M = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w), dtype=np.uint8), np.zeros((h, w))
    sig = sigmas(params, DENOISE_SIGMAS)
    lib.select_noise_run(b.ctypes.data, K, cp, n_all, acc.ctypes.data, mom.ctypes.data, guides.ctypes.data, w, h, int(params["levels"]), int(params["demodulate"]),
                         sig.ctypes.data, int(smooth), S.ctypes.data, L.ctypes.data, M.ctypes.data)
    return S, L, M


def core_errors(lib, M, S, floor=0.01):
    """select_noise_error of every pixel: M (h, w) f64, S (h, w, 3) f32 -> e_S (h, w)"""
    M = np.ascontiguousarray(M, dtype=np.float64)
    S = np.ascontiguousarray(S, dtype=np.float32)
    assert S.shape == M.shape + (3,)
    out = np.zeros(M.shape)
    lib.select_noise_errors(M.ctypes.data, S.ctypes.data, float(floor), M.size, out.ctypes.data)
    return out


def core_tile_rule(lib, e_img, threshold):
    """The tile rule of the device (adapt_pixel_above over a tile's 16 lanes) on an error image (h, w) -> (tiles_y, tiles_x) uint8"""
    e = np.ascontiguousarray(e_img, dtype=np.float64)
    h, w = e.shape
    out = np.zeros(((h + 3) // 4, (w + 3) // 4), dtype=np.uint8)
    lib.select_noise_tile_rule(e.ctypes.data, w, h, float(threshold), out.ctypes.data)
    return out
