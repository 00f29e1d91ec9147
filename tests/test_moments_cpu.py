"""Per-pixel sample moments and the noise estimate (option "moments") on the CPU tier: the entry points are declared,
exported and bound by every host layer; csrc/noise_core.h, compiled for the host here, agrees with a numpy restatement of the definition;
the CLI documents its four flags and refuses bad values before any device is opened."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cli import run_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def noise_reference(moments, n, floor):
    """The definition (include/hanamaru_hip.h), every step one IEEE f64 operation, in the order noise_core.h takes them."""
    mom = np.asarray(moments, dtype=np.float64)
    n = np.float64(n)
    s1, s2 = mom[..., 0:3], mom[..., 3:6]
    m = s1 / n
    var = np.maximum(0.0, (s2 - s1 * m) / (n - 1.0))
    se = np.sqrt(var / n) / 4.0
    mu = m / 4.0
    return ((se[..., 0] + se[..., 1]) + se[..., 2]) / (((mu[..., 0] + mu[..., 1]) + mu[..., 2]) + 3.0 * np.float64(floor))


def ulp_distance(a, b):
    """Distance in units of the last place between two arrays of finite, non-negative doubles (their bit patterns are ordered like integers)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    assert np.isfinite(a).all() and np.isfinite(b).all() and (a >= 0).all() and (b >= 0).all()
    return np.abs((a + 0.0).view(np.int64) - (b + 0.0).view(np.int64))


def _product_header():
    text = open(os.path.join(ROOT, "include", "hanamaru_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_moments_entry_points_declared_and_exported(ha):
    text = _product_header()
    c = r"hr_ctx\s*\*\s*\w*"
    assert re.search(r"int\s+hr_read_moments\s*\(\s*%s\s*,\s*double\s*\*\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)\s*;" % c, text)
    assert re.search(r"int\s+hr_write_moments\s*\(\s*%s\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*\)\s*;" % c, text)
    assert re.search(r"int\s+hr_noise_estimate\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*,\s*hr_noise\s*\*\s*\w+\s*\)\s*;" % c, text)
    assert re.search(r"int\s+hr_read_noise_image\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;" % c, text)
    assert re.search(r"typedef\s+struct\s+hr_noise\s*\{\s*uint64_t\s+samplings\s*,\s*pixels\s*,\s*pixels_above\s*;\s*double\s+mean_error\s*,\s*max_error\s*;\s*\}\s*hr_noise\s*;", text)
    assert int(re.search(r"#define\s+HR_ABI_VERSION\s+(\d+)", text).group(1)) == 7   # functions and one struct were added, no struct changed
    assert '"moments"' in open(os.path.join(ROOT, "include", "hanamaru_hip.h")).read()
    lib = C.CDLL(ha.HIP_LIB)
    for name in ("hr_read_moments", "hr_write_moments", "hr_noise_estimate", "hr_read_noise_image"):
        assert hasattr(lib, name), name
    assert C.sizeof(ha.Stats) == 46 * 8 and C.sizeof(ha.Noise) == 40


def test_python_and_rust_mirrors_bind_the_moments(ha):
    for m in ("read_moments", "write_moments", "noise_estimate", "noise_image"):
        assert callable(getattr(ha.Renderer, m, None)), m
    L = ha.hip_lib()
    assert len(L.hr_read_moments.argtypes) == 3 and len(L.hr_write_moments.argtypes) == 3
    assert len(L.hr_noise_estimate.argtypes) == 4 and len(L.hr_read_noise_image.argtypes) == 3
    assert [f for f, _ in ha.Noise._fields_] == ["samplings", "pixels", "pixels_above", "mean_error", "max_error"]
    ffi = open(os.path.join(ROOT, "rust", "hip_ffi.rs")).read()
    assert re.search(r"pub fn hr_read_moments\(ctx: \*mut HrCtx, host: \*mut f64, samplings: \*mut u64\) -> c_int;", ffi)
    assert re.search(r"pub fn hr_write_moments\(ctx: \*mut HrCtx, host: \*const f64, samplings: u64\) -> c_int;", ffi)
    assert re.search(r"pub fn hr_noise_estimate\(ctx: \*mut HrCtx, floor: f64, threshold: f64, out: \*mut HrNoise\) -> c_int;", ffi)
    assert re.search(r"pub fn hr_read_noise_image\(ctx: \*mut HrCtx, floor: f64, host: \*mut f64", ffi)
    assert "pub struct HrNoise" in ffi and "size_of::<HrNoise>() == 40" in ffi
    ren = open(os.path.join(ROOT, "rust", "hip_renderer.rs")).read()
    assert "hr_noise_estimate(self.ctx" in ren and "pub noise_target: Option<(f64, f64)>" in ren


def _noise_core(tmp_path):
    src = tmp_path / "noise_harness.cpp"
    src.write_text('#include "noise_core.h"\n'
                   'extern "C" void noise_batch(const double *mom, const unsigned long long *n, const double *floor, int count, double *out) {\n'
                   '    for (int i = 0; i < count; i++) out[i] = hr::noise_pixel_error(mom + 6 * i, n[i], floor[i]);\n'
                   '}\n')
    so = tmp_path / "libnoise_harness.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-I", os.path.join(ROOT, "hanamaru-renderer_amd", "csrc"),
                    "-o", str(so), str(src)], check=True)
    lib = C.CDLL(str(so))
    lib.noise_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]

    def run(mom, n, floor):
        mom = np.ascontiguousarray(mom, dtype=np.float64).reshape(-1, 6)
        n = np.ascontiguousarray(np.broadcast_to(n, (mom.shape[0],)), dtype=np.uint64)
        floor = np.ascontiguousarray(np.broadcast_to(floor, (mom.shape[0],)), dtype=np.float64)
        out = np.empty(mom.shape[0], dtype=np.float64)
        lib.noise_batch(mom.ctypes.data, n.ctypes.data, floor.ctypes.data, mom.shape[0], out.ctypes.data)
        return out
    return run


def _synthetic_moments(rng, pixels, n, scale):
    """Moments of `n` fp32 values per pixel and channel, summed the way the kernel sums them (one at a time, in f64)."""
    x = (rng.gamma(0.7, scale, size=(n, pixels, 3))).astype(np.float32).astype(np.float64)
    return np.concatenate([np.cumsum(x, axis=0)[-1], np.cumsum(x * x, axis=0)[-1]], axis=-1)


def test_noise_core_matches_the_definition(tmp_path):
    """noise_core.h against the numpy restatement on synthetic moments: within 4 ulp of f64 (one sqrt per channel and three further roundings
    may differ between libm and numpy; everything else is a correctly rounded IEEE operation on identical inputs)."""
    run = _noise_core(tmp_path)
    rng = np.random.default_rng(20261016)
    for n, scale, floor in [(2, 1.0, 0.01), (3, 0.02, 0.01), (24, 4.0, 0.01), (1000, 1.0, 0.5), (100000, 300.0, 1e-6)]:
        mom = _synthetic_moments(rng, 4096, min(n, 64), scale)
        got, ref = run(mom, n, floor), np.array([noise_reference(m, n, floor) for m in mom])
        assert np.isfinite(got).all() and (got >= 0).all()
        d = ulp_distance(got, ref)
        print("n = %d: worst %d ulp" % (n, int(d.max())))
        assert d.max() <= 4, (n, int(d.max()))
    # n = 2 with both values known: x = (1, 3) per channel -> m = 2, var = 2, se = sqrt(2 / 2) / 4 = 0.25, mu = 0.5, e = 0.75 / (1.5 + 0.03)
    two = run([4.0, 4.0, 4.0, 10.0, 10.0, 10.0], 2, 0.01)[0]
    assert ulp_distance([two], [0.75 / (1.5 + 3.0 * 0.01)])[0] <= 4
    # a black pixel: zero moments -> e = 0 / (3 floor) = 0, not NaN
    assert run(np.zeros(6), 24, 0.01)[0] == 0.0
    # a constant pixel whose S2 fell below S1^2 / n by rounding: the variance is clamped at 0, e = 0 (not NaN from a negative sqrt)
    s1 = 24 * 0.1
    below = np.nextafter(s1 * (s1 / 24), 0.0)
    assert (np.float64(below) - np.float64(s1) * (np.float64(s1) / 24)) / 23.0 < 0
    assert run([s1, s1, s1, below, below, below], 24, 0.01)[0] == 0.0 and noise_reference([s1, s1, s1, below, below, below], 24, 0.01) == 0.0
    # one noisy channel next to two clamped ones
    mixed = np.array([s1, 24 * 0.5, s1, below, 24 * 0.5 * 0.5 * 3.0, below])
    assert ulp_distance(run(mixed, 24, 0.01), [noise_reference(mixed, 24, 0.01)])[0] <= 4 and run(mixed, 24, 0.01)[0] > 0


def test_cli_help_lists_the_noise_flags(tmp_path):
    r = run_cli(["--help"], tmp_path, missing="skip")
    assert r.returncode == 0
    for flag in ("--noise-target E", "--noise-floor F", "--noise-check N", "--noise-image FILE.png"):
        assert flag in r.stdout, flag
    assert "default 0.01" in r.stdout and "default 64" in r.stdout


@pytest.mark.parametrize("args,flag", [(["--noise-target", "-0.1"], "--noise-target"), (["--noise-target", "nan"], "--noise-target"),
                                       (["--noise-target", "soon"], "--noise-target"), (["--noise-target", "0.1x"], "--noise-target"),
                                       (["--noise-floor", "0"], "--noise-floor"), (["--noise-floor", "-1"], "--noise-floor"),
                                       (["--noise-floor", "nan"], "--noise-floor"), (["--noise-floor", "dark"], "--noise-floor"),
                                       (["--noise-check", "0"], "--noise-check"), (["--noise-check", "-3"], "--noise-check"),
                                       (["--noise-check", "1.5"], "--noise-check")])
def test_cli_rejects_bad_noise_values_before_any_device(tmp_path, args, flag):
    """Argument errors: exit status 1 and a message naming the flag, before the log file is opened or a device is touched."""
    r = run_cli(["-w", "96", "-h", "54", "-s", "4"] + args, tmp_path, missing="skip")
    assert r.returncode == 1, r.stdout
    assert flag in r.stdout
    assert not (tmp_path / "result.txt").exists()
