"""The error estimate of hr_denoise_select's image restated in numpy — written from the comment of include/hanamaru_hip.h and of
csrc/select_noise_core.h with the pieces of tests/post_numpy.py, every line one IEEE f64 operation per element, every sum in the order written.
The host build of the header (tests/select_noise_cores.py) and the device are held against this bit for bit, so this module reads no file under
csrc/ and does not import select_noise_cores.

No GPU in this module."""
import numpy as np

from post_numpy import (DENOISE_DEFAULTS, EPS, _counts, _sigmas2, atrous_level, demodulate, fill_buckets, initial_state, remodulate, sums_of, synthetic_inputs,
                        smooth as smooth_plane)


def synthetic(seed, w, h, K, n, firefly=0.03):
    """Consistent inputs of one render: per-sampling values whose mean follows synthetic_inputs' guides, with rare bright outliers, summed into
    the fp32 accumulator, the f64 moments and the K buckets (sampling j of a pixel into bucket j mod K).  n: one count, or per-pixel counts (a pixel
    holds its own prefix).  Returns (buckets, acc, mom, n, guides)."""
    rng = np.random.default_rng(seed)
    g = synthetic_inputs(seed, w, h, n=2)[3]
    cnt = _counts(n, h, w)
    mean = 4.0 * (g[..., 0:3].astype(np.float64) + 0.05)
    N = int(cnt.max())
    x = rng.gamma(2.0, 0.5, size=(N, h, w, 3)) * mean
    x = np.where(rng.random((N, h, w, 1)) < firefly, x * 200.0, x).astype(np.float32)
    x = x * (np.arange(N)[:, None, None, None] < cnt[None, ..., None])
    acc, mom = sums_of(x)
    return fill_buckets(x, K), acc, mom, n, g


def _sum3(v):
    return (v[..., 0] + v[..., 1]) + v[..., 2]


def numpy_select_noise(buckets, acc, mom, n, guides, smooth=0, **over):
    """Returns (S, L, M, per-level mse (levels + 1, h, w)).  S and L are numpy_select's, restated here beside M."""
    p = dict(DENOISE_DEFAULTS, **over)
    B = np.asarray(buckets, dtype=np.float64)
    h, w, K = B.shape[:3]
    acc = np.asarray(acc, dtype=np.float32)
    mom = np.asarray(mom, dtype=np.float64)
    g = np.asarray(guides, dtype=np.float32).astype(np.float64)
    cnt = _counts(n, h, w)
    assert (cnt >= 2).all()
    levels = int(p["levels"])
    dem = bool(p["demodulate"]) and levels > 0
    with np.errstate(under="ignore", invalid="ignore", over="ignore", divide="ignore"):
        nb = (cnt.astype(np.int64)[..., None] - np.arange(K)[None, None, :] + (K - 1)) // K
        nA, nB = nb[..., 0::2].sum(axis=-1).astype(np.float64)[..., None], nb[..., 1::2].sum(axis=-1).astype(np.float64)[..., None]
        sa, sb = B[..., 0, :].copy(), B[..., 1, :].copy()
        for b in range(2, K):
            if b & 1:
                sb = sb + B[..., b, :]
            else:
                sa = sa + B[..., b, :]
        A0, B0 = sa / nA / 4.0, sb / nB / 4.0
        FW, nd = initial_state(acc, mom, cnt)
        V0 = FW[..., 3:6]
        FA, FB = np.concatenate([A0, V0 * nd / nA], axis=-1), np.concatenate([B0, V0 * nd / nB], axis=-1)
        a = g[..., 0:3] + EPS
        k = a * a
        if dem:
            FA, FB, FW = demodulate(FA, a), demodulate(FB, a), demodulate(FW, a)
            A0, B0 = FA[..., 0:3], FB[..., 0:3]
        vA0, vB0 = FA[..., 3:6].copy(), FB[..., 3:6].copy()
        best = S = L = M = None
        per_level = []
        for lev in range(levels + 1):
            dA, dB = FA[..., 0:3] - B0, FB[..., 0:3] - A0
            e = ((dA[..., 0] * dA[..., 0] + dB[..., 0] * dB[..., 0]) + (dA[..., 1] * dA[..., 1] + dB[..., 1] * dB[..., 1])) + (dA[..., 2] * dA[..., 2] + dB[..., 2] * dB[..., 2])
            hc = ((dA * dA + dB * dB) - (vA0 + vB0)) / 2.0
            vh = (FA[..., 3:6] + FB[..., 3:6]) / 2.0
            vw = FW[..., 3:6]
            if dem:
                hc, vh, vw = hc * k, vh * k, vw * k
            m = _sum3(hc)
            for t in range(int(smooth)):
                e = smooth_plane(e, 1 << t)
                m = smooth_plane(m, 1 << t)
            x = m - _sum3(vh)
            mse = _sum3(vw) + np.where(x > 0.0, x, 0.0)
            per_level.append(mse)
            final = (remodulate(FW[..., 0:3], a) if dem else FW[..., 0:3]).astype(np.float32)
            if lev == 0:
                best, L, S, M = e, np.zeros((h, w), dtype=np.uint8), final, mse
            else:
                take = e < best
                best, L, S, M = np.where(take, e, best), np.where(take, np.uint8(lev), L), np.where(take[..., None], final, S), np.where(take, mse, M)
            if lev < levels:
                FA, FB, FW = (atrous_level(F, g, 1 << lev, _sigmas2(p)) for F in (FA, FB, FW))
    return S, L.astype(np.uint8), M, np.stack(per_level)


def numpy_error(M, S, floor=0.01):
    """e_S = sqrt(M) / (S_r + S_g + S_b + 3 floor), 0 where the denominator is not positive"""
    S = np.asarray(S, dtype=np.float32).astype(np.float64)
    den = ((S[..., 0] + S[..., 1]) + S[..., 2]) + 3.0 * np.float64(floor)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0.0, np.sqrt(M) / den, 0.0)


def numpy_tile_rule(e_img, threshold, prev=None):
    """(tiles_y, tiles_x) uint8: a 4x4 tile is active iff one of its in-image pixels has e > threshold (a NaN never has), ANDed with prev"""
    h, w = e_img.shape
    ty, tx = (h + 3) // 4, (w + 3) // 4
    hot = np.zeros((ty * 4, tx * 4), dtype=bool)
    hot[:h, :w] = e_img > threshold
    out = hot.reshape(ty, 4, tx, 4).any(axis=(1, 3))
    if prev is not None:
        out = out & (np.asarray(prev) != 0)
    return out.astype(np.uint8)
