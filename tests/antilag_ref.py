"""The contract of vimg_antilag_rescale (include/vimg_antilag.h) restated in numpy float32: every + - * / is one float32
operation in the header's order, every choice a comparison (np.where, never np.maximum / np.minimum, whose NaN rules
are not the comparison's).  The window sums are written as the header writes them - clipped to the picture, columns
ascending within a row, then rows ascending - not as the kernel computes them (a zero-padded tile).  The library must
give these bits; tests/test_antilag_abi.py pins this file on its own."""
import numpy as np

F = np.float32
DEFAULTS = dict(radius=2, t_low=2.0, t_high=3.0, min_matches=8.0, sigma_normal=0.1, sigma_plane=0.00005)


def lum(c):
    return (c[..., 0] * F(0.212671) + c[..., 1] * F(0.715160)) + c[..., 2] * F(0.072169)


def pairs(color, normal, position, depth, history, matrix, *, sigma_normal, sigma_plane, **_):
    """Pass 1: (d, v) [H, W] float32 of the history [>= 3, H, W, 4] against the current [H, W, 3] frames."""
    C, n, P = (np.asarray(a, dtype=F) for a in (color, normal, position))
    z = np.asarray(depth, dtype=F)[..., 0]
    hist = np.asarray(history, dtype=F)
    h, w = z.shape
    M = np.asarray(matrix, dtype=F).reshape(12)
    sigma_normal, sigma_plane = F(sigma_normal), F(sigma_plane)
    zero, one, half = F(0), F(1), F(0.5)
    A, nq, zq, Pq = hist[0], hist[1, ..., :3], hist[1, ..., 3], hist[2, ..., :3]
    with np.errstate(all="ignore"):
        ok = A[..., 3] > zero
        hx = ((M[0] * Pq[..., 0] + M[1] * Pq[..., 1]) + M[2] * Pq[..., 2]) + M[3]
        hy = ((M[4] * Pq[..., 0] + M[5] * Pq[..., 1]) + M[6] * Pq[..., 2]) + M[7]
        hw = ((M[8] * Pq[..., 0] + M[9] * Pq[..., 1]) + M[10] * Pq[..., 2]) + M[11]
        ok = ok & (hw > zero)
        fx = hx / hw - half
        fy = hy / hw - half
        cx, cy = np.floor(fx + half), np.floor(fy + half)
        ok = ok & (cx >= zero) & (cx < F(w)) & (cy >= zero) & (cy < F(h))
        ix, iy = (np.where(ok, v, zero).astype(np.int64) for v in (cx, cy))
        ok = ok & (z[iy, ix] > zero)
        np_, Pp, Cp = n[iy, ix], P[iy, ix], C[iy, ix]
        dn = one - ((nq[..., 0] * np_[..., 0] + nq[..., 1] * np_[..., 1]) + nq[..., 2] * np_[..., 2])
        e = Pp - Pq
        dd = (nq[..., 0] * e[..., 0] + nq[..., 1] * e[..., 1]) + nq[..., 2] * e[..., 2]
        sz = sigma_plane * zq
        ok = ok & (dn < sigma_normal) & (dd * dd < sz * sz)
        d = lum(Cp) - lum(A[..., :3])
        ok = ok & (d - d == zero)
    d = np.where(ok, d, zero).astype(F)
    return d, np.where(ok, one, zero).astype(F)


def window_sums(d, v, radius):
    """Pass 2's sums: (sd, sq, c) [H, W] float32 over the window of ``radius`` clipped to the picture."""
    h, w = d.shape
    with np.errstate(all="ignore"):
        terms = (d, d * d, v)
    yy, xx = np.mgrid[0:h, 0:w]
    rows = []
    for t in terms:
        s = np.zeros((h, w), F)
        for dx in range(-radius, radius + 1):                # columns ascending
            qx = xx + dx
            inside = (qx >= 0) & (qx < w)
            with np.errstate(all="ignore"):
                s = np.where(inside, s + t[yy, np.where(inside, qx, 0)], s)
        rows.append(s)
    out = []
    for s in rows:
        a = np.zeros((h, w), F)
        for dy in range(-radius, radius + 1):                # rows ascending
            qy = yy + dy
            inside = (qy >= 0) & (qy < h)
            with np.errstate(all="ignore"):
                a = np.where(inside, a + s[np.where(inside, qy, 0), xx], a)
        out.append(a.astype(F))
    return tuple(out)


def scale_of(sd, sq, c, *, t_low, t_high, min_matches, **_):
    t_low, t_high, min_matches = F(t_low), F(t_high), F(min_matches)
    zero, one = F(0), F(1)
    with np.errstate(all="ignore"):
        m = sd / c
        var = (sq - sd * m) / (c - one)
        var = np.where(var > zero, var, zero)
        t2 = (m * m) / (var / c)
        lo, hi = t_low * t_low, t_high * t_high
        ramp = (hi - t2) / (hi - lo)
        s = np.where(~(t2 > lo), one, np.where(~(t2 < hi), zero, ramp))
    return np.where(c >= min_matches, s, one).astype(F)


def rescale(color, normal, position, depth, history, matrix, **params):
    """The frames, the history [PLANES >= 3, H, W, 4] and the CURRENT camera's 12-float matrix in; (the rescaled copy
    of the history, the scale [H, W]) out.  Only [0, :, :, 3] differs from ``history``, and only where it is > 0."""
    params = dict(DEFAULTS, **params)
    hist = np.array(history, dtype=F, copy=True)
    d, v = pairs(color, normal, position, depth, hist, matrix, **params)
    s = scale_of(*window_sums(d, v, int(params["radius"])), **params)
    L = hist[0, ..., 3]
    with np.errstate(all="ignore"):
        hist[0, ..., 3] = np.where(L > F(0), L * s, L)
    assert hist.dtype == F and s.dtype == F
    return hist, s
