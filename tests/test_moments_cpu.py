"""Per-pixel sample moments and the noise estimate (option "moments") on the CPU tier: the entry points are declared,
exported and bound by every host layer; csrc/noise_core.h, compiled for the host here, agrees with a numpy restatement of the definition;
the CLI documents its four flags and refuses bad values before any device is opened."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import interface_checks as ic
from cli import run_cli
from post_cores import core, core_noise  # noqa: F401  (core: the g++-built harness, a fixture)
from post_numpy import noise_reference, ulp_distance


def test_moments_entry_points_declared_and_exported(ha):
    text = ic.header_text()
    assert ic.declared(text, r"int\s+hr_read_moments\s*\(\s*%s\s*,\s*double\s*\*\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_write_moments\s*\(\s*%s\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*uint64_t\s+\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_noise_estimate\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*,\s*hr_noise\s*\*\s*\w+\s*\)\s*;")
    assert ic.declared(text, r"int\s+hr_read_noise_image\s*\(\s*%s\s*,\s*double\s+\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;")
    assert re.search(r"typedef\s+struct\s+hr_noise\s*\{\s*uint64_t\s+samplings\s*,\s*pixels\s*,\s*pixels_above\s*;\s*double\s+mean_error\s*,\s*max_error\s*;\s*\}\s*hr_noise\s*;", text)
    assert ic.abi_version(text) == 7   # functions and one struct were added, no struct changed
    assert '"moments"' in ic.header_text(raw=True)
    assert not ic.exported_and_bound(ha, ("hr_read_moments", "hr_write_moments", "hr_noise_estimate", "hr_read_noise_image"))
    assert C.sizeof(ha.Stats) == 46 * 8 and C.sizeof(ha.Noise) == 40


def test_python_and_rust_mirrors_bind_the_moments(ha):
    for m in ("read_moments", "write_moments", "noise_estimate", "noise_image"):
        assert callable(getattr(ha.Renderer, m, None)), m
    L = ha.hip_lib()
    assert len(L.hr_read_moments.argtypes) == 3 and len(L.hr_write_moments.argtypes) == 3
    assert len(L.hr_noise_estimate.argtypes) == 4 and len(L.hr_read_noise_image.argtypes) == 3
    assert [f for f, _ in ha.Noise._fields_] == ["samplings", "pixels", "pixels_above", "mean_error", "max_error"]
    ffi = ic.rust_ffi()
    assert re.search(r"pub fn hr_read_moments\(ctx: \*mut HrCtx, host: \*mut f64, samplings: \*mut u64\) -> c_int;", ffi)
    assert re.search(r"pub fn hr_write_moments\(ctx: \*mut HrCtx, host: \*const f64, samplings: u64\) -> c_int;", ffi)
    assert re.search(r"pub fn hr_noise_estimate\(ctx: \*mut HrCtx, floor: f64, threshold: f64, out: \*mut HrNoise\) -> c_int;", ffi)
    assert re.search(r"pub fn hr_read_noise_image\(ctx: \*mut HrCtx, floor: f64, host: \*mut f64", ffi)
    assert "pub struct HrNoise" in ffi and "size_of::<HrNoise>() == 40" in ffi
    ren = ic.read("rust", "hip_renderer.rs")
    assert "hr_noise_estimate(self.ctx" in ren and "pub noise_target: Option<(f64, f64)>" in ren


def _synthetic_moments(rng, pixels, n, scale):
    """Moments of `n` fp32 values per pixel and channel, summed the way the kernel sums them (one at a time, in f64)."""
    x = (rng.gamma(0.7, scale, size=(n, pixels, 3))).astype(np.float32).astype(np.float64)
    return np.concatenate([np.cumsum(x, axis=0)[-1], np.cumsum(x * x, axis=0)[-1]], axis=-1)


def test_noise_core_matches_the_definition(core):
    """noise_core.h against the numpy restatement on synthetic moments: within 4 ulp of f64 (one sqrt per channel and three further roundings
    may differ between libm and numpy; everything else is a correctly rounded IEEE operation on identical inputs)."""
    run = functools.partial(core_noise, core)
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
    r, left_a_result = ic.cli_refused(tmp_path, args, size=("-w", "96", "-h", "54", "-s", "4"), missing="skip")
    assert r.returncode == 1, r.stdout
    assert flag in r.stdout
    assert not left_a_result
