"""The post-processing chain restated in numpy: the noise estimate, the robust resolve and its error, variance and excess, one à-trous level and
what is built from it (hr_denoise, hr_denoise_robust, hr_robust_restore, hr_denoise_select) — written from the comments of include/hanamaru_hip.h
and of the core headers, every line one IEEE f64 operation per element, every sum sequential from its first term, the taps in row order.  The host
build of the headers (tests/post_cores.py) and the device are held against these bit for bit, so this module reads no file under csrc/ and does not
import post_cores.  Also here: the synthetic inputs and the two metrics the tests and tools share.

No GPU in this module."""
import numpy as np

from gpu_helpers import bits  # noqa: F401  (the one bit-pattern view; re-exported for the tests of this family)

ALL_K = (3, 5, 7, 9, 11, 13, 15)
DENOISE_DEFAULTS = {"levels": 4, "demodulate": 1, "sigma_color": 3.0, "sigma_normal": 0.5, "sigma_albedo": 0.25, "sigma_depth": 0.1}
RESTORE_DEFAULTS = {"levels": 4, "base": 0, "sigma_n": 0.5, "sigma_a": 0.25, "sigma_z": 0.1}
EPS, TINY = 1e-3, 1e-30
TAP_KERNEL = (0.375, 0.25, 0.0625)


# ---- metrics ----
def ulp_distance(a, b):
    """Distance in units of the last place between two arrays of finite, non-negative doubles (their bit patterns are ordered like integers)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    assert np.isfinite(a).all() and np.isfinite(b).all() and (a >= 0).all() and (b >= 0).all()
    return np.abs((a + 0.0).view(np.int64) - (b + 0.0).view(np.int64))


def rel_sq_error(x, t):
    return float(np.mean((x.astype(np.float64) - t) ** 2 / (t ** 2 + 0.01 ** 2)))


# ---- the noise estimate from the moments ----
def noise_reference(moments, n, floor):
    """The definition (include/hanamaru_hip.h), every step one IEEE f64 operation, in the order noise_core.h takes them.  n: one count, or a count
    per pixel."""
    mom = np.asarray(moments, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)[..., None]
    s1, s2 = mom[..., 0:3], mom[..., 3:6]
    m = s1 / n
    var = np.maximum(0.0, (s2 - s1 * m) / (n - 1.0))
    se = np.sqrt(var / n) / 4.0
    mu = m / 4.0
    return ((se[..., 0] + se[..., 1]) + se[..., 2]) / (((mu[..., 0] + mu[..., 1]) + mu[..., 2]) + 3.0 * np.float64(floor))


# ---- the buckets: means, order, trim ----
def _pixels(buckets, n):
    """buckets (.., K, 3) as (P, K, 3), n as (P,) uint64, and the leading shape"""
    B = np.asarray(buckets, dtype=np.float64)
    K, shape = B.shape[-2], B.shape[:-2]
    B = B.reshape(-1, K, 3)
    return B, np.broadcast_to(np.asarray(n, dtype=np.uint64).reshape(-1), (B.shape[0],)), K, shape


def bucket_means_sorted(B, n):
    """Of buckets B (P, K, 3) after n (P,) samplings: the bucket means m (bucket b holds n_b = (n - b + K - 1) / K samplings of four sub-samples),
    their keys y, the stable order by (y, b), and keys and means in that order.  (A count below K is taken as K: no caller uses such a pixel.)"""
    K = B.shape[1]
    nn = np.maximum(n, np.uint64(K))
    nb = (nn[:, None] - np.arange(K, dtype=np.uint64)[None, :] + np.uint64(K - 1)) // np.uint64(K)
    m = B / nb.astype(np.float64)[..., None] / 4.0
    y = (m[..., 0] + m[..., 1]) + m[..., 2]
    order = np.argsort(y, axis=1, kind="stable")                                  # ascending by (y, b)
    return m, y, order, np.take_along_axis(y, order, 1), np.take_along_axis(m, order[..., None], 1)


def gini_trim(ys, K):
    """The buckets dropped at either end: the Gini coefficient G of the sorted keys, (int)(G K / 2), at most down to the median."""
    T = ys[:, 0].copy()
    Gn = float(1 - K) * ys[:, 0]
    for i in range(2, K + 1):
        T = T + ys[:, i - 1]
        Gn = Gn + float(2 * i - K - 1) * ys[:, i - 1]
    G = Gn / (float(K) * T)
    want = np.trunc(np.where((T > 0.0) & (G > 0.0), G * float(K) / 2.0, 0.0)).astype(np.int64)
    return np.minimum((K - 1) // 2, want)


def kept_sum(vs, t):
    """The sum of the sorted values vs (P, K[, 3]) without t at either end, from its first term."""
    K = vs.shape[1]
    s = vs[:, t].copy()
    for i in range(t + 1, K - t):
        s = s + vs[:, i]
    return s


def winsorized(vs, t):
    """The K sorted values with the t at either end replaced by the nearest kept one."""
    K = vs.shape[1]
    lo, hi = vs[:, t], vs[:, K - 1 - t]
    return [lo if i < t else (hi if i >= K - t else vs[:, i]) for i in range(K)]


def winsorized_ss(w, K):
    """The sum of squares of the K values of the list w about their mean."""
    ws = w[0].copy()
    for i in range(1, K):
        ws = ws + w[i]
    wbar = ws / float(K)
    ss = (w[0] - wbar) * (w[0] - wbar)
    for i in range(1, K):
        d = w[i] - wbar
        ss = ss + d * d
    return ss


def numpy_robust(buckets, n):
    """hr_robust (include/hanamaru_hip.h).  Returns (R float32 (.., 3), trim uint8 (..))."""
    B, n, K, shape = _pixels(buckets, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = B[:, 0, :].copy()
        for b in range(1, K):
            s = s + B[:, b, :]
        plain = s / n.astype(np.float64)[:, None] / 4.0
        _, _, _, ys, ms = bucket_means_sorted(B, n)                                   # (where n < K the robust branch is not taken)
        trim = gini_trim(ys, K)
        robust = np.zeros((B.shape[0], 3))
        for t in range((K - 1) // 2 + 1):
            robust = np.where((trim == t)[:, None], kept_sum(ms, t) / float(K - 2 * t), robust)
    small = (n < np.uint64(K))[:, None]
    R = np.where((n == 0)[:, None], 0.0, np.where(small, plain, robust)).astype(np.float32)
    trim = np.where(small[:, 0], 0, trim).astype(np.uint8)
    return R.reshape(shape + (3,)), trim.reshape(shape)


def numpy_error(buckets, n, floor=0.01, parts=False):
    """The comment of robust_pixel_error.  Every n >= K.  parts: (e, trim, se, Ry, ss) instead of (e, trim)."""
    B, n, K, shape = _pixels(buckets, n)
    P = B.shape[0]
    assert (n >= K).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        _, _, _, ys, _ = bucket_means_sorted(B, n)
        trim = gini_trim(ys, K)
        e = np.zeros(P)
        se_all, ry_all, ss_all = np.zeros(P), np.zeros(P), np.zeros(P)
        for t in range((K - 1) // 2 + 1):
            kept = float(K - 2 * t)
            Ry = kept_sum(ys, t) / kept
            ss = winsorized_ss(winsorized(ys, t), K)
            se = np.sqrt(ss / float(K - 1) / float(K)) * float(K) / kept
            den = Ry + 3.0 * floor
            e_t = np.where(den > 0.0, se / den, 0.0)
            sel = trim == t
            e = np.where(sel, e_t, e)
            se_all, ry_all, ss_all = np.where(sel, se, se_all), np.where(sel, Ry, ry_all), np.where(sel, ss, ss_all)
    if parts:
        return e.reshape(shape), trim.astype(np.uint8).reshape(shape), se_all.reshape(shape), ry_all.reshape(shape), ss_all.reshape(shape)
    return e.reshape(shape), trim.astype(np.uint8).reshape(shape)


def numpy_cv(buckets, n):
    """The comment of robust_pixel_cv_k.  Every n >= K.  Returns (cv (.., 6), trim)."""
    B, n, K, shape = _pixels(buckets, n)
    assert (n >= K).all()
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        _, _, _, ys, ms = bucket_means_sorted(B, n)
        trim = gini_trim(ys, K)
        cv = np.zeros((B.shape[0], 6))
        for t in range((K - 1) // 2 + 1):
            kept = float(K - 2 * t)
            Cc = kept_sum(ms, t) / kept
            ss = winsorized_ss(winsorized(ms, t), K)
            f = float(K) / kept
            V = ss / float(K - 1) / float(K) * f * f
            cv = np.where((trim == t)[:, None], np.concatenate([Cc, V], axis=1), cv)
    return cv.reshape(shape + (6,)), trim.astype(np.uint8).reshape(shape)


def numpy_excess(buckets, n):
    """The comment of restore_core.h.  Every n >= K.  Returns (cx (.., 6), trim)."""
    B, n, K, shape = _pixels(buckets, n)
    P = B.shape[0]
    assert (n >= K).all()
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        _, _, _, ys, ms = bucket_means_sorted(B, n)
        trim = gini_trim(ys, K)
        cx = np.zeros((P, 6))
        for t in range((K - 1) // 2 + 1):
            Cc = kept_sum(ms, t) / float(K - 2 * t)
            X = np.zeros((P, 3))
            if t:
                top = ms[:, K - 1 - t, :]
                e = ms[:, K - t, :] - top
                for i in range(K - t + 1, K):
                    e = e + (ms[:, i, :] - top)
                q = e / float(K)
                X = np.where(q > 0.0, q, 0.0)
            cx = np.where((trim == t)[:, None], np.concatenate([Cc, X], axis=1), cx)
    return cx.reshape(shape + (6,)), trim.astype(np.uint8).reshape(shape)


# ---- one à-trous level ----
def taps(h, w, s):
    """The 5 x 5 taps of step s in row order: (i, j, P, Q), Q the slices of P moved by (s i, s j).  A tap that is outside the image for every pixel
    is skipped."""
    for j in range(-2, 3):
        for i in range(-2, 3):
            dx, dy = s * i, s * j
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            if y0 < y1 and x0 < x1:
                yield i, j, (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def kernel_weight(x):
    """K(x) = max(0, 1 - x)^2"""
    t = 1.0 - x
    u = np.where(t > 0.0, t, 0.0)
    return u * u


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def guide_weight(g, P, Q, i, j, sn2, sa2, sz2):
    """h(i) h(j) K(x_n) K(x_a) K(x_z) K(x_h) of tap (i, j) between the pixels P and Q of the guide planes g (h, w, 8) in f64"""
    A, N, Z, H = g[..., 0:3], g[..., 3:6], g[..., 6], g[..., 7]
    xn = _sq3(N[P] - N[Q]) / sn2
    xa = _sq3(A[P] - A[Q]) / sa2
    dz = Z[P] - Z[Q]
    xz = (dz * dz) / (sz2 * (Z[P] * Z[P] + Z[Q] * Z[Q]) + TINY)
    dh = H[P] - H[Q]
    xh = dh * dh
    k = TAP_KERNEL
    return ((((k[abs(i)] * k[abs(j)]) * kernel_weight(xn)) * kernel_weight(xa)) * kernel_weight(xz)) * kernel_weight(xh)


def atrous_level(state, g, s, sigmas2):
    """denoise_core.h's level with step s on a state (h, w, 6) = {C, V}; sigmas2: the squares of sigma_color, _normal, _albedo, _depth"""
    Cc, V = state[..., 0:3], state[..., 3:6]
    h, w = Cc.shape[:2]
    sc2, sn2, sa2, sz2 = sigmas2
    sw, sC, sV = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w, 3))
    sumV = (V[..., 0] + V[..., 1]) + V[..., 2]
    for i, j, P, Q in taps(h, w, s):
        xc = _sq3(Cc[P] - Cc[Q]) / (sc2 * (sumV[P] + sumV[Q]) + TINY)
        wt = guide_weight(g, P, Q, i, j, sn2, sa2, sz2) * kernel_weight(xc)
        w2 = wt * wt
        sw[P] = sw[P] + wt
        sC[P] = sC[P] + wt[..., None] * Cc[Q]
        sV[P] = sV[P] + w2[..., None] * V[Q]
    return np.concatenate([sC / sw[..., None], sV / (sw * sw)[..., None]], axis=-1)


def smooth(e, s):
    """The tap kernel alone, step s, over a plane e (h, w), normalised by the taps inside the image."""
    h, w = e.shape
    k = TAP_KERNEL
    se, sh = np.zeros((h, w)), np.zeros((h, w))
    for i, j, P, Q in taps(h, w, s):
        hw = k[abs(i)] * k[abs(j)]
        se[P] = se[P] + hw * e[Q]
        sh[P] = sh[P] + hw
    return se / sh


_smooth_plane = smooth                                                                # (numpy_select's parameter has the name)


def demodulate(state, a):
    """{C / a, V / a^2}"""
    return np.concatenate([state[..., 0:3] / a, state[..., 3:6] / (a * a)], axis=-1)


def remodulate(C, a):
    return C * a


def _sigmas2(p):
    return tuple(p[k] * p[k] for k in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"))


def _counts(n, h, w):
    return np.full((h, w), n, dtype=np.uint32) if np.isscalar(n) else np.asarray(n, dtype=np.uint32)


def initial_state(acc, mom, cnt):
    """{C, V} of the mean from the fp32 accumulator and the f64 moments with cnt (h, w) samplings, and cnt in f64 (h, w, 1)"""
    scale = (np.float32(1.0) / (cnt * np.uint32(4)).astype(np.float32)).astype(np.float64)     # the resolve's fp32 scale, correctly rounded
    nd = cnt.astype(np.float64)[..., None]
    C0 = acc.astype(np.float64) * scale[..., None]
    s1, s2 = mom[..., 0:3], mom[..., 3:6]
    var = (s2 - s1 * (s1 / nd)) / (nd - 1.0)
    V0 = np.where(var > 0.0, var, 0.0) / nd / 16.0
    return np.concatenate([C0, V0], axis=-1), nd


def numpy_filter(cv, guides, want_state=False, **over):
    """denoise_core.h's demodulation, levels and final pass on an initial state cv (h, w, 6) = {C, V}."""
    p = dict(DENOISE_DEFAULTS, **over)
    g = np.asarray(guides, dtype=np.float32).astype(np.float64)
    levels = int(p["levels"])
    dem = bool(p["demodulate"]) and levels > 0
    a = g[..., 0:3] + EPS
    state = demodulate(cv, a) if dem else cv
    with np.errstate(under="ignore"):
        for lev in range(levels):
            state = atrous_level(state, g, 1 << lev, _sigmas2(p))
    Cc = state[..., 0:3]
    out = (remodulate(Cc, a) if dem else Cc).astype(np.float32)
    return (out, state) if want_state else out


def numpy_denoise(acc, mom, n, guides, want_state=False, **over):
    """hr_denoise (include/hanamaru_hip.h): numpy_filter on the state of the mean."""
    acc = np.asarray(acc, dtype=np.float32)
    h, w = acc.shape[:2]
    state, _ = initial_state(acc, np.asarray(mom, dtype=np.float64), _counts(n, h, w))
    return numpy_filter(state, guides, want_state, **over)


def numpy_spread(X, guides, **over):
    """restore_norm and restore_gather, level by level, on an excess X (h, w, 3)."""
    p = dict(RESTORE_DEFAULTS, **over)
    g = np.asarray(guides, dtype=np.float32).astype(np.float64)
    X = np.asarray(X, dtype=np.float64)
    h, w = X.shape[:2]
    s2 = (p["sigma_n"] * p["sigma_n"], p["sigma_a"] * p["sigma_a"], p["sigma_z"] * p["sigma_z"])
    with np.errstate(under="ignore"):
        for lev in range(int(p["levels"])):
            N = np.zeros((h, w))
            for i, j, P, Q in taps(h, w, 1 << lev):
                N[P] = N[P] + guide_weight(g, P, Q, i, j, *s2)
            S = X / N[..., None]
            out = np.zeros((h, w, 3))
            for i, j, P, Q in taps(h, w, 1 << lev):
                out[P] = out[P] + guide_weight(g, P, Q, i, j, *s2)[..., None] * S[Q]
            X = out
    return X


def numpy_restore(buckets, n, guides, D=None, **over):
    cx, _ = numpy_excess(buckets, n)
    x = numpy_spread(cx[..., 3:6], guides, **over)
    base = cx[..., 0:3] if D is None else np.asarray(D, dtype=np.float32).astype(np.float64)
    return (base + x).astype(np.float32), x


def numpy_select(buckets, acc, mom, n, guides, smooth=0, **over):
    """The comment of select_core.h.  Returns (S, L, states (3, h, w, 6))."""
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
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
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
        if dem:
            FA, FB, FW = demodulate(FA, a), demodulate(FB, a), demodulate(FW, a)
            A0, B0 = FA[..., 0:3], FB[..., 0:3]
        best = S = L = None
        for lev in range(levels + 1):
            dA, dB = FA[..., 0:3] - B0, FB[..., 0:3] - A0
            e = ((dA[..., 0] * dA[..., 0] + dB[..., 0] * dB[..., 0]) + (dA[..., 1] * dA[..., 1] + dB[..., 1] * dB[..., 1])) + (dA[..., 2] * dA[..., 2] + dB[..., 2] * dB[..., 2])
            for t in range(int(smooth)):
                e = _smooth_plane(e, 1 << t)
            final = (remodulate(FW[..., 0:3], a) if dem else FW[..., 0:3]).astype(np.float32)
            if lev == 0:
                best, L, S = e, np.zeros((h, w), dtype=np.uint8), final
            else:
                take = e < best
                best, L, S = np.where(take, e, best), np.where(take, np.uint8(lev), L), np.where(take[..., None], final, S)
            if lev < levels:
                FA, FB, FW = (atrous_level(F, g, 1 << lev, _sigmas2(p)) for F in (FA, FB, FW))
    return S, L.astype(np.uint8), np.stack([FA, FB, FW])


# ---- synthetic inputs ----
def fill_buckets(x, K, start=0):
    """The bucket sums of per-sampling values x (n, .., 3), fp32, one sampling at a time in f64: sampling j into bucket (start + j) mod K."""
    B = np.zeros(x.shape[1:-1] + (K, 3))
    for j in range(x.shape[0]):
        B[..., (start + j) % K, :] += x[j].astype(np.float32).astype(np.float64)
    return B


def sums_of(x):
    """(fp32 accumulator, f64 moments) of the samplings x (n, h, w, 3), one sampling at a time"""
    acc = np.zeros(x.shape[1:], dtype=np.float32)
    for s in range(x.shape[0]):
        acc = acc + x[s]
    xd = x.astype(np.float64)
    return acc, np.concatenate([xd.sum(axis=0), (xd * xd).sum(axis=0)], axis=-1)


def heavy_tailed(rng, n, shape):
    """Per-sampling values with rare very bright outliers: what NEE to a small emitter without MIS produces."""
    x = rng.gamma(2.0, 0.5, size=(n,) + shape + (3,))
    hot = rng.random((n,) + shape + (1,)) < 0.03
    return np.where(hot, x * 400.0, x).astype(np.float32)


def synthetic_inputs(seed, w, h, counts=None, n=12):
    """A small frame with structure in every guide: two albedo regions, a normal that turns, a depth ramp with a step, a band of misses (eight
    zeros) and a column of partly covered pixels; gamma-distributed per-sampling values whose mean follows the albedo.  Returns
    (accumulator f32, moments f64, counts or n, guides f32)."""
    rng = np.random.default_rng(seed)
    cnt = np.full((h, w), n, dtype=np.uint32) if counts is None else np.asarray(counts, dtype=np.uint32)
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.zeros((h, w, 8), dtype=np.float32)
    left = xx < (w + 1) // 2
    g[..., 0:3] = np.where(left[..., None], np.float32([0.8, 0.3, 0.2]), np.float32([0.25, 0.5, 0.75]))
    ang = (0.02 * xx + 0.5 * (yy >= (h + 1) // 2)).astype(np.float32)
    g[..., 3], g[..., 4], g[..., 5] = np.sin(ang), 0.0, np.cos(ang)
    g[..., 6] = (4.0 + 0.01 * xx + 0.02 * yy + 3.0 * (xx >= (2 * w) // 3)).astype(np.float32)
    g[..., 7] = 1.0
    if h > 4:
        g[h - 2:, :, :] = 0.0                                   # misses
    if w > 8:
        g[:, 5, :] *= np.float32(0.5)                           # two of four sub-samples hit
    acc = np.zeros((h, w, 3), dtype=np.float32)
    mom = np.zeros((h, w, 6))
    mean = 4.0 * (g[..., 0:3].astype(np.float64) + 0.05)
    for s in range(int(cnt.max())):
        x = (rng.gamma(2.0, 0.5, size=(h, w, 3)) * mean).astype(np.float32) * (cnt > s)[..., None]
        acc = acc + x                                            # fp32, one sampling at a time
        mom[..., 0:3] += x.astype(np.float64)
        mom[..., 3:6] += x.astype(np.float64) ** 2
    return acc, mom, (n if counts is None else cnt), g


def flat_guides(w, h):
    g = np.zeros((h, w, 8), dtype=np.float32)
    g[..., 0:3] = 0.5
    g[..., 5] = 1.0
    g[..., 6] = 4.0
    g[..., 7] = 1.0
    return g


def tie_pixel(swap=False):
    """K = 9, n = 9: buckets 0 and 1 share the key y = 1 with different colours, two hot buckets make the trim 1 — the two tied buckets straddle
    the low trim boundary.  swap: the two change places."""
    B = np.zeros((9, 3))
    B[0], B[1] = [4.0, 0.0, 0.0], [0.0, 4.0, 0.0]
    B[2:7] = [4.0, 4.0, 4.0]
    B[7:9] = [8.0, 8.0, 8.0]
    if swap:
        B[[0, 1]] = B[[1, 0]]
    return B


def plant(B, n=None):
    """The corner cases into the first pixels of an image of buckets (h, w, K, 3), wherever the image has room for them: equal buckets, one hot
    bucket, all zero, negative sums, tiny values (the squares of their differences are subnormal), and for K = 9 the tie of tie_pixel."""
    B = B.copy()
    K = B.shape[-2]
    flat = B.reshape(-1, K, 3)
    cases = [np.broadcast_to(np.float64([3.0, 10.0, 0.5]), (K, 3)), np.zeros((K, 3)), np.zeros((K, 3)), -np.abs(flat[0]) - 1.0, flat[0] * 1e-160]
    cases[1] = cases[1].copy()
    cases[1][K // 3] = [7.0, 14.0, 3.5]
    if K == 9:
        cases += [tie_pixel(), tie_pixel(True)]
    for i, c in enumerate(cases):
        if 2 * i + 1 < flat.shape[0]:
            flat[2 * i + 1] = c
    return B


def synthetic_buckets(seed, K, shape, n):
    """Heavy-tailed buckets with the planted cases.  n: a count for every pixel, or per-pixel counts (every pixel the buckets of its own prefix)."""
    rng = np.random.default_rng(seed)
    if np.isscalar(n):
        return plant(fill_buckets(heavy_tailed(rng, min(int(n), 96), shape), K))
    x = heavy_tailed(rng, int(n.max()), shape)
    x = x * (np.arange(x.shape[0])[:, None, None, None] < n[None, ..., None])
    return plant(fill_buckets(x, K))
