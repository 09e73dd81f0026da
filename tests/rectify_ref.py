"""The contract of vimg_rectify_clamp (include/vimg_rectify.h) restated in numpy float32, written from the header: every
+ - * / and the square root is one float32 operation in the header's order, every choice a comparison (np.where, never
np.maximum / np.minimum, whose NaN rules are not the comparison's).  The library must give these bits;
tests/test_rectify_abi.py pins this file on its own."""
import numpy as np

from atrous_ref import _shifted

F = np.float32
KEPT, CLAMPED, FEW_TAPS, NOT_LIVE = 0, 1, 2, 3


def clamp(slow, fast, albedo=None, *, radius, min_taps, k, cut, sigma_normal, sigma_plane, albedo_floor):
    """``slow`` [>= 3, H, W, 4] and ``fast`` [>= 3, H, W, 4] float32 histories (planes A, G0, G1 first) and the
    [H, W, 3] albedo frame or None in; (the new plane A [H, W, 4], the [H, W, 3] colour of every pixel, the [H, W] uint8
    codes) out.  Nothing is written to the arguments."""
    slow, fast = np.asarray(slow, dtype=F), np.asarray(fast, dtype=F)
    A, n, z, P = slow[0], slow[1][..., :3], slow[1][..., 3], slow[2][..., :3]
    R, min_taps = int(radius), int(min_taps)
    k, cut, sigma_normal, sigma_plane, floor = F(k), F(cut), F(sigma_normal), F(sigma_plane), F(albedo_floor)
    one, zero = F(1), F(0)
    h, w = z.shape
    with np.errstate(all="ignore"):
        if albedo is not None:
            albedo = np.asarray(albedo, dtype=F)
            a = np.where(albedo > floor, albedo, floor).astype(F)
        else:
            a = np.ones((h, w, 3), F)
        Fq_all = (fast[0][..., :3] / a).astype(F)
        Lf = fast[0][..., 3]
        Ls = A[..., 3]
        H = (A[..., :3] / a).astype(F)
        live = (z > zero) & (Ls > zero)
        sz = sigma_plane * z
        plane_den = sz * sz
        m = np.zeros((h, w), np.int64)
        s1, s2 = np.zeros((h, w, 3), F), np.zeros((h, w, 3), F)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                zq, Lfq = _shifted(z, dy, dx, zero), _shifted(Lf, dy, dx, zero)       # outside the image: not accepted
                nq, Pq, Fq = (_shifted(a_, dy, dx, zero) for a_ in (n, P, Fq_all))
                ok = (zq > zero) & (Lfq > zero)
                if dx != 0 or dy != 0:
                    dn = one - ((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
                    s_n = np.where(dn < zero, zero, dn / sigma_normal)
                    e = Pq - P
                    d = (n[..., 0] * e[..., 0] + n[..., 1] * e[..., 1]) + n[..., 2] * e[..., 2]
                    s_p = (d * d) / plane_den
                    ok = ok & ((s_n + s_p) < one)
                m = np.where(ok, m + 1, m)
                s1 = np.where(ok[..., None], s1 + Fq, s1).astype(F)
                s2 = np.where(ok[..., None], s2 + Fq * Fq, s2).astype(F)
        enough = live & (m >= min_taps)
        fm = m.astype(F)[..., None]
        mean = s1 / fm
        v = s2 / fm - mean * mean
        v = np.where(v < zero, zero, v).astype(F)
        wd = k * np.sqrt(v)
        lo, hi = mean - wd, mean + wd
        below, above = H < lo, H > hi
        Hc = np.where(below, lo, np.where(above, hi, H)).astype(F)
        moved = enough & (below | above).any(axis=-1)
        rgb = np.where(moved[..., None], Hc * a, A[..., :3]).astype(F)
        L = np.where(moved & (Lf > zero) & (Ls > Lf), Ls - cut * (Ls - Lf), Ls).astype(F)
        code = np.where(~live, NOT_LIVE, np.where(~enough, FEW_TAPS, np.where(moved, CLAMPED, KEPT))).astype(np.uint8)
    plane = np.concatenate([rgb, L[..., None]], axis=-1).astype(F)
    assert plane.dtype == F and rgb.dtype == F
    return plane, rgb, code


def rel_error(x, ref):
    """DESIGN.md 4.18's relative squared error e = mean((x - ref)^2 / (ref^2 + 0.01)), in float64."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(((x - ref) ** 2 / (ref ** 2 + 0.01)).mean())


def flat_histories(h, w, slow_rgb=0.5, fast_rgb=0.5, Ls=16.0, Lf=4.0, z=8.0):
    """(slow, fast) [3, h, w, 4] of a plane facing the camera: normal (0, 0, 1), positions on z = -8 a unit apart,
    depth 8, constant colours and lengths."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for rgb, L in ((slow_rgb, Ls), (fast_rgb, Lf)):
        t = np.zeros((3, h, w, 4), F)
        t[0, ..., :3] = rgb
        t[0, ..., 3] = L
        t[1, ..., 2] = 1
        t[1, ..., 3] = z
        t[2, ..., 0], t[2, ..., 1], t[2, ..., 2] = xx, yy, -z
        out.append(t)
    return out[0], out[1]


def synthetic_histories(h, w, planes=3, seed=7):
    """(slow [planes, h, w, 4], fast [3, h, w, 4], albedo [h, w, 3]) of one picture: a wall facing the camera that meets,
    at a vertical edge, a wall turned away (1 - n.n = 0.2), both with relief in their positions so that the plane term
    decides near 1; a block of misses; slow pixels of length 0; fast pixels of length 0 and some longer than the slow
    ones; a checkered albedo with components below any floor; a quarter of the picture where the slow colour is stale
    (four times the fast); and - from 48 pixels on - a NaN and an inf fast colour and a NaN slow colour."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    xe = max(1, int(0.55 * w))
    right = xx >= xe
    slow, fast = np.zeros((planes, h, w, 4), F), np.zeros((3, h, w, 4), F)
    relief = rng.uniform(-0.5, 0.5, (h, w))
    slow[1, ..., :3] = np.where(right[..., None], (-0.6, 0.0, 0.8), (0.0, 0.0, 1.0))
    pz = np.where(right, -8.0 + 0.75 * (xx - xe), -8.0) + relief
    slow[2, ..., 0], slow[2, ..., 1], slow[2, ..., 2] = xx, yy, pz
    slow[1, ..., 3] = -pz
    base = 0.2 + 0.6 * rng.random((h, w, 3))
    base = np.where(right[..., None], base * 0.5, base)
    fast[0, ..., :3] = base * rng.uniform(0.7, 1.3, (h, w, 3))
    slow[0, ..., :3] = base * rng.uniform(0.9, 1.1, (h, w, 3))
    slow[0, : (h + 1) // 2, : (w + 1) // 2, :3] *= 4                       # stale
    slow[0, ..., 3] = rng.integers(1, 33, (h, w))
    fast[0, ..., 3] = rng.integers(1, 5, (h, w))
    fast[0, ..., 3][rng.random((h, w)) < 0.08] = 0                        # no fast history
    fast[0, ..., 3][rng.random((h, w)) < 0.05] = 40                       # longer than any slow one
    slow[0, ..., 3][rng.random((h, w)) < 0.05] = 0                        # no slow history
    miss = (yy < h // 4) & (xx >= w - max(1, w // 5))
    slow[1, ..., 3][miss] = 0
    slow[0][miss] = 0
    fast[0][miss] = 0
    fast[1:] = slow[1:3]
    if planes > 3:
        slow[3] = rng.random((h, w, 4))
    albedo = np.where(((xx // 3 + yy // 2) % 2 == 0)[..., None], (0.8, 0.7, 0.6), (0.3, 0.25, 0.35)).astype(F)
    albedo[rng.random((h, w)) < 0.06] = (0.001, 0.5, 0.0)
    if h * w >= 48:
        ys, xs = np.nonzero(~miss)
        spots = [(ys[i], xs[i]) for i in np.linspace(0, len(ys) - 1, 5).astype(int)[1:4]]
        fast[0][spots[0]][1] = np.nan
        fast[0][spots[1]][:3] = np.inf
        slow[0][spots[2]][0] = np.nan
    return slow.astype(F), fast.astype(F), albedo
