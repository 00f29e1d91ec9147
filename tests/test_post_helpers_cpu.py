"""The helpers the post-processing tests share (tests/post_cores.py, tests/post_numpy.py, gpu_helpers.bits), checked on their own: the harness
exports what the table binds and is built once, the tap slices and the bucket prologue agree with per-pixel loops written from the headers'
comments, and the bit-pattern comparison of the *_against_numpy tests fails on a single flipped bit."""
import numpy as np
import pytest

from post_cores import SIGNATURES, core_cv, core_denoise, core_error, core_robust, lib
from post_numpy import (bits, bucket_means_sorted, fill_buckets, gini_trim, heavy_tailed, numpy_cv, numpy_denoise, numpy_error, numpy_robust,
                        synthetic_inputs, taps, tie_pixel)


def test_the_harness_exports_every_bound_entry_and_is_built_once():
    assert lib() is lib()
    for name, argtypes in SIGNATURES.items():
        assert hasattr(lib(), name), name
        assert list(getattr(lib(), name).argtypes or []) == argtypes, name


@pytest.mark.parametrize("s", [1, 2, 4, 8])
@pytest.mark.parametrize("h,w", [(3, 5), (1, 1), (4, 9)])
def test_taps_against_a_loop_over_the_pixels(h, w, s):
    """Every (pixel p, neighbour q, i, j) with q inside the image, the taps in row order and the pixels of a tap in row order; a tap without a pair
    is not yielded at all (from s = max(h, w) on that is every tap but the centre; 4 x 9 at s = 8 keeps the centre row's two nearest)."""
    want = []
    for j in range(-2, 3):
        for i in range(-2, 3):
            for y in range(h):
                for x in range(w):
                    if 0 <= y + s * j < h and 0 <= x + s * i < w:
                        want.append(((y, x), (y + s * j, x + s * i), i, j))
    got, yielded = [], 0
    for i, j, P, Q in taps(h, w, s):
        yielded += 1
        ps = [(y, x) for y in range(*P[0].indices(h)) for x in range(*P[1].indices(w))]
        qs = [(y, x) for y in range(*Q[0].indices(h)) for x in range(*Q[1].indices(w))]
        assert ps and len(ps) == len(qs), (i, j)
        got += [(p, q, i, j) for p, q in zip(ps, qs)]
    assert got == want
    assert yielded == len({(i, j) for _, _, i, j in want})
    if s >= max(h, w):
        assert yielded == 1


def _prologue_of_one_pixel(B, n):
    """robust_core.h's comment for n >= K, one operation at a time on Python floats (IEEE f64): (m, y, order, trim)"""
    K = len(B)
    m = [[float(B[b][c]) / float((n - b + K - 1) // K) / 4.0 for c in range(3)] for b in range(K)]
    y = [(m[b][0] + m[b][1]) + m[b][2] for b in range(K)]
    order = []
    for b in range(K):                                                               # a stable insertion sort, ties by bucket index
        at = len(order)
        while at > 0 and y[order[at - 1]] > y[b]:
            at -= 1
        order.insert(at, b)
    T, Gn = y[order[0]], float(2 - K - 1) * y[order[0]]
    for i in range(2, K + 1):
        T = T + y[order[i - 1]]
        Gn = Gn + float(2 * i - K - 1) * y[order[i - 1]]
    trim = 0
    if T > 0.0:
        G = Gn / (float(K) * T)
        trim = min((K - 1) // 2, int(G * float(K) / 2.0)) if G > 0.0 else 0
    return m, y, order, trim


def _prologue_cases():
    for K in (3, 9, 15):
        rng = np.random.default_rng(40 + K)
        counts = rng.integers(K, 3 * K + 3, size=64).astype(np.uint64)
        x = heavy_tailed(rng, int(counts.max()), (64,))
        yield fill_buckets(x * (np.arange(x.shape[0])[:, None, None] < counts[None, :, None]), K), counts
        hot = np.zeros((K, K, 3))
        hot[np.arange(K), np.arange(K)] = [1.0, 2.0, 0.5]
        yield np.concatenate([np.zeros((1, K, 3)), hot]), np.full(K + 1, 2 * K, dtype=np.uint64)
    yield np.stack([tie_pixel(), tie_pixel(True)]), np.full(2, 9, dtype=np.uint64)


def test_the_bucket_prologue_against_a_scalar_loop():
    pixels = 0
    for B, n in _prologue_cases():
        K = B.shape[1]
        with np.errstate(divide="ignore", invalid="ignore"):
            m, y, order, ys, ms = bucket_means_sorted(B, n)
            trim = gini_trim(ys, K)
        for p in range(B.shape[0]):
            wm, wy, worder, wtrim = _prologue_of_one_pixel(B[p], int(n[p]))
            assert np.array_equal(bits(m[p]), bits(np.float64(wm))) and np.array_equal(bits(y[p]), bits(np.float64(wy))), (K, p)
            assert order[p].tolist() == worder, (K, p)
            assert np.array_equal(bits(ys[p]), bits(np.float64(wy)[worder])) and np.array_equal(bits(ms[p]), bits(np.float64(wm)[worder])), (K, p)
            assert int(trim[p]) == wtrim, (K, p)
        pixels += B.shape[0]
    assert pixels == 3 * 64 + (4 + 10 + 16) + 2


def test_bits_of_one_four_and_eight_byte_elements():
    assert bits(np.uint8([0, 255])).dtype == np.uint8 and bits(np.uint8([0, 255])).tolist() == [0, 255]
    assert bits(np.array([True, False])).tolist() == [1, 0]
    assert bits(np.float32([1.0, -0.0])).dtype == np.uint32 and bits(np.float32([1.0, -0.0])).tolist() == [0x3F800000, 0x80000000]
    assert bits(np.float64([1.0, -0.0])).dtype == np.uint64 and bits(np.float64([1.0, -0.0])).tolist() == [0x3FF0000000000000, 0x8000000000000000]
    assert not np.array_equal(bits(np.float64([0.0])), bits(np.float64([-0.0])))        # equal values, other bits
    with pytest.raises(KeyError):
        bits(np.float16([1.0]))


def _flipped(a, index):
    """a with the lowest bit of one element flipped"""
    out = np.array(a, copy=True)
    view = out.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[out.dtype.itemsize]).reshape(-1)
    view[index] ^= 1
    return out


def test_one_flipped_bit_fails_the_comparison_with_the_restatement():
    """SENSITIVE: the comparison of the *_against_numpy tests, np.array_equal(bits(core), bits(numpy)), holds for the restatement and fails
    when the lowest bit of one of its values is flipped — in an f32 radiance, an f64 state, an f64 error and a uint8 trim."""
    K, n = 9, 20
    B = fill_buckets(heavy_tailed(np.random.default_rng(6), n, (5, 7)), K)
    acc, mom, cnt, g = synthetic_inputs(8, 7, 5)
    pairs = [(core_robust(lib(), B, n)[0], numpy_robust(B, n)[0]), (core_robust(lib(), B, n)[1], numpy_robust(B, n)[1]),
             (core_error(lib(), B, n)[0], numpy_error(B, n)[0]), (core_cv(lib(), B, n)[0], numpy_cv(B, n)[0]),
             (core_denoise(lib(), acc, mom, cnt, g, want_state=True, levels=2)[1], numpy_denoise(acc, mom, cnt, g, want_state=True, levels=2)[1]),
             (core_denoise(lib(), acc, mom, cnt, g, levels=2), numpy_denoise(acc, mom, cnt, g, levels=2))]
    for got, ref in pairs:
        assert np.array_equal(bits(got), bits(ref))
        for index in (0, ref.size // 2, ref.size - 1):
            assert not np.array_equal(bits(got), bits(_flipped(ref, index))), (ref.dtype, index)
