"""csrc/reproject_core.h restated in f64 numpy — written from the comment of include/hanamaru_hip.h and of the header: every step one
IEEE f64 operation, in the order written (numpy neither fuses nor reorders).  The CPU tests hold the host-compiled core against these lines.

No GPU in this module."""
import numpy as np

SNAP = 2.0 ** -10
MAX_MOTION = 2.0 ** 20
DEFAULTS = dict(max_history=32, min_roughness=0.3, depth_tolerance=1e-3)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cam_array(cam):
    """{eye, forward, plane_half_right, plane_half_up, focus_distance} of a Camera structure (or anything with those fields) as 13 doubles"""
    v = lambda p: [p.x, p.y, p.z]
    return np.array(v(cam.eye) + v(cam.forward) + v(cam.plane_half_right) + v(cam.plane_half_up) + [cam.focus_distance], dtype=np.float64)


def numpy_project(cam, x, at_infinity):
    """reproject_project.  cam: 13 doubles; x (n, 3) float32; at_infinity (n,) bool.  Returns (front bool, v (n, 3), ncx, ncy)."""
    eye, fwd, phr, phu, focus = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12]
    xd = x.astype(np.float64)
    v = np.where(at_infinity[:, None], xd, xd - eye[None, :])
    c = _dot(v, fwd[None, :])
    with np.errstate(all="ignore"):
        front = c > 0.0
        k = c / focus
        dr, du = _dot(phr, phr) * k, _dot(phu, phu) * k
        ncx = np.where(front, _dot(v, phr[None, :]) / dr, 0.0)
        ncy = np.where(front, _dot(v, phu[None, :]) / du, 0.0)
    return front, v, ncx, ncy


def numpy_motion(ncx, ncy, W, H, px, py, sub):
    """reproject_motion.  Returns (inside bool, mx, my)."""
    w, h = float(W), float(H)
    m = w if w < h else h
    ox, oy = (sub & 1).astype(np.float64) * 0.5 - 0.5, (sub >> 1).astype(np.float64) * 0.5 - 0.5
    with np.errstate(all="ignore"):
        fx, fy = (ncx * m + w) / 2.0, (ncy * m + h) / 2.0
        gx, gy = px.astype(np.float64) + ox, (h - py.astype(np.float64)) + oy
        mx, my = fx - gx, gy - fy
        mx = np.where((mx < SNAP) & (mx > -SNAP), 0.0, mx)
        my = np.where((my < SNAP) & (my > -SNAP), 0.0, my)
        inside = (fx >= -1.0) & (fx <= w + 1.0) & (fy >= -1.0) & (fy <= h + 1.0)
    return inside, mx, my


def numpy_reproject(motion, acc, counts, mom, max_history):
    """reproject_pixel over an image.  motion (h, w, 4, 3) float32; acc (h, w, 3) float32; counts (h, w) uint32; mom (h, w, 6) float64 or None.
    Returns (acc', counts', mom' or None)."""
    h, w = counts.shape
    yy, xx = np.mgrid[0:h, 0:w]
    pxd, pyd = xx.astype(np.float64), yy.astype(np.float64)
    wd, hd = float(w), float(h)
    Wp, N = np.zeros((h, w)), np.zeros((h, w))
    A = np.zeros((h, w, 3))
    M = np.zeros((h, w, 6)) if mom is not None else None
    accd = acc.astype(np.float64)
    with np.errstate(all="ignore"):
        for s in range(4):
            mx, my = motion[:, :, s, 0].astype(np.float64), motion[:, :, s, 1].astype(np.float64)
            valid = (motion[:, :, s, 2] == 0.0) & (mx >= -MAX_MOTION) & (mx <= MAX_MOTION) & (my >= -MAX_MOTION) & (my <= MAX_MOTION)
            mx, my = np.where(valid, mx, 0.0), np.where(valid, my, 0.0)
            u, v = pxd + mx, pyd + my
            x0, y0 = np.floor(u), np.floor(v)
            ax, ay = u - x0, v - y0
            for j in range(2):
                ty, wy = y0 + float(j), (ay if j else 1.0 - ay)
                for i in range(2):
                    tx, wx = x0 + float(i), (ax if i else 1.0 - ax)
                    wt = wx * wy
                    ok = valid & (wt != 0.0) & (tx >= 0.0) & (tx < wd) & (ty >= 0.0) & (ty < hd)
                    ix, iy = np.where(ok, tx, 0.0).astype(np.int64), np.where(ok, ty, 0.0).astype(np.int64)
                    nq = counts[iy, ix]
                    ok = ok & (nq != 0)
                    nd = np.where(ok, nq.astype(np.float64), 1.0)
                    Wp = np.where(ok, Wp + wt, Wp)
                    N = np.where(ok, N + wt * nd, N)
                    A = np.where(ok[..., None], A + wt[..., None] * (accd[iy, ix] / nd[..., None]), A)
                    if M is not None:
                        M = np.where(ok[..., None], M + wt[..., None] * (mom[iy, ix] / nd[..., None]), M)
        quarter, cap = np.floor(N / 4.0), float(max_history)
        nn = np.where(quarter < cap, quarter, cap)
        none = ~(Wp > 0.0) | ~(nn >= 1.0)
        safe = np.where(none, 1.0, Wp)
        out_acc = np.where(none[..., None], 0.0, (A / safe[..., None]) * nn[..., None]).astype(np.float32)
        out_counts = np.where(none, 0.0, nn).astype(np.uint32)
        out_mom = np.where(none[..., None], 0.0, (M / safe[..., None]) * nn[..., None]) if M is not None else None
    return out_acc, out_counts, out_mom
