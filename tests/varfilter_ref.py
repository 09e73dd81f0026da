"""The contracts of vimg_varfilter_atrous and vimg_varfilter_variance (include/vimg_varfilter.h) restated in numpy
float32: every + - * / is one float32 operation in the header's order, every choice a comparison (np.where, never
np.maximum / np.minimum, whose NaN rules are not the comparison's).  The library must give these bits;
tests/test_varfilter_abi.py pins this file on its own."""
import numpy as np

from atrous_ref import H5, _shifted

F = np.float32
B3 = (F(1 / 4), F(1 / 2), F(1 / 4))
YR, YG, YB = F(0.212671), F(0.715160), F(0.072169)


def lum(v):
    return (v[..., 0] * YR + v[..., 1] * YG) + v[..., 2] * YB


def known(v):
    """Where a variance frame's value is known: v >= 0 && v < +inf, as comparisons (a NaN is neither)."""
    v = np.asarray(v, dtype=F)
    with np.errstate(invalid="ignore"):
        return (v >= F(0)) & (v < F(np.inf))


def _guide_score(n, P, nq, Pq, sigma_normal, plane_den):
    one, zero = F(1), F(0)
    dn = one - ((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
    s_n = np.where(dn < zero, zero, dn / sigma_normal)
    e = Pq - P
    d = (n[..., 0] * e[..., 0] + n[..., 1] * e[..., 1]) + n[..., 2] * e[..., 2]
    return s_n + (d * d) / plane_den


def atrous(color, normal, position, depth, albedo=None, variance=None, *, iterations, sigma_luminance, sigma_normal, sigma_plane,
           albedo_floor, variance_floor, stages=None):
    """[H, W, 3] float32 frames and the [H, W] variance frame (or None) in; (the filtered [H, W, 3] frame, its
    [H, W] variance) out.  ``depth`` is the `depth` feature frame (t t t): its first component is read.
    ``stages``: a dict that receives the demodulated V after the estimate ("estimated") for the pins."""
    color, n, P = (np.asarray(a, dtype=F) for a in (color, normal, position))
    z = np.asarray(depth, dtype=F)[..., 0]
    sigma_luminance, sigma_normal, sigma_plane = F(sigma_luminance), F(sigma_normal), F(sigma_plane)
    floor, vfloor = F(albedo_floor), F(variance_floor)
    one, zero = F(1), F(0)
    with np.errstate(all="ignore"):
        # pack
        if albedo is not None:
            albedo = np.asarray(albedo, dtype=F)
            a = np.where(albedo > floor, albedo, floor).astype(F)
            C = color / a
            ya = lum(a)
        else:
            C = color.copy()
            ya = np.ones(z.shape, F)
        ya2 = ya * ya
        live = z > zero                                     # False for a miss and for a NaN depth
        if variance is not None:
            v = np.asarray(variance, dtype=F)
            V = np.where(known(v), v / ya2, F(-1))
        else:
            V = np.full(z.shape, -1, F)
        V = np.where(live, V, zero).astype(F)
        sz = sigma_plane * z
        plane_den = sz * sz

        # estimate: live pixels with V < 0
        L = lum(C)
        sw, s1, s2 = (np.zeros(z.shape, F) for _ in range(3))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                if dx == 0 and dy == 0:
                    w, Lq = np.ones(z.shape, F), L
                else:
                    zq = _shifted(z, dy, dx, zero)                      # outside the image: not live
                    nq, Pq = (_shifted(a_, dy, dx, zero) for a_ in (n, P))
                    Lq = _shifted(L, dy, dx, zero)
                    S = _guide_score(n, P, nq, Pq, sigma_normal, plane_den)
                    t = one - S
                    w = np.where(S < one, t * t, zero)
                    w = np.where((zq > zero) & ((Lq - Lq) == zero), w, zero).astype(F)
                take = w > zero
                sw = np.where(take, sw + w, sw)
                s1 = np.where(take, s1 + w * Lq, s1)
                s2 = np.where(take, s2 + w * (Lq * Lq), s2)
        m1, m2 = s1 / sw, s2 / sw
        est = m2 - m1 * m1
        est = np.where(est < zero, zero, est)
        V = np.where(live & (V < zero), est, V).astype(F)
        if stages is not None:
            stages["estimated"] = V.copy()

        sl2 = sigma_luminance * sigma_luminance
        for i in range(iterations):
            s = 1 << i
            # the 3 x 3 Gaussian of V over the live taps
            sg, sv = np.zeros(z.shape, F), np.zeros(z.shape, F)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    g = B3[dx + 1] * B3[dy + 1]
                    use = _shifted(z, dy, dx, zero) > zero
                    Vr = _shifted(V, dy, dx, zero)
                    sg = np.where(use, sg + g, sg)
                    sv = np.where(use, sv + g * Vr, sv)
            Vg = sv / sg
            den = sl2 * Vg + vfloor
            Lp = lum(C)
            sumw = np.zeros(z.shape, F)
            sumc = np.zeros(C.shape, F)
            sumv = np.zeros(z.shape, F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    k = H5[dx + 2] * H5[dy + 2]
                    if dx == 0 and dy == 0:
                        w, Cq, Vq = np.full(z.shape, k, F), C, V
                    else:
                        zq = _shifted(z, s * dy, s * dx, zero)
                        nq, Pq, Cq = (_shifted(a_, s * dy, s * dx, zero) for a_ in (n, P, C))
                        Vq = _shifted(V, s * dy, s * dx, zero)
                        dl = Lp - lum(Cq)
                        S = _guide_score(n, P, nq, Pq, sigma_normal, plane_den) + (dl * dl) / den
                        t = one - S
                        w = np.where(S < one, k * (t * t), zero)
                        w = np.where(zq > zero, w, zero).astype(F)
                    take = w > zero
                    sumw = np.where(take, sumw + w, sumw)
                    sumc = np.where(take[..., None], sumc + w[..., None] * Cq, sumc)
                    sumv = np.where(take, sumv + (w * w) * Vq, sumv)
            C = np.where(live[..., None], sumc / sumw[..., None], C).astype(F)
            V = np.where(live, sumv / (sumw * sumw), V).astype(F)
        # unpack
        out = C * a if albedo is not None else C
        out_v = V * ya2
    assert out.dtype == F and out_v.dtype == F
    return out, out_v


def variance(count, batches, m2):
    """vimg_varfilter_variance: V = (K < 2 || N == 0) ? NaN : ((M2 < 0 ? 0 : M2) / float(K - 1)) / float(N)."""
    N, K = np.asarray(count).astype(np.uint32), np.asarray(batches).astype(np.uint32)
    m2 = np.asarray(m2, dtype=F)
    with np.errstate(all="ignore"):
        km1 = np.where(K < 2, 1, K - np.uint32(1)).astype(F)
        v = (np.where(m2 < F(0), F(0), m2) / km1) / N.astype(F)
    return np.where((K < 2) | (N == 0), F(np.nan), v).astype(F)


def shadowed_frame(h=64, w=96):
    """atrous_ref.synthetic_frame with a shadow on the floor right of column 48 at 0.3, which no guide knows about:
    the frame's dict with ``clean`` darkened there (``noisy`` is not used: noisy_mean makes the noisy frames)."""
    from atrous_ref import synthetic_frame
    s = synthetic_frame(h, w)
    floor = s["hit"] & (s["normal"][..., 1] == 1) & (s["normal"][..., 0] == 0)
    shade = np.ones((h, w, 1), F)
    shade[:, 48:][floor[:, 48:]] = F(0.3)
    s["clean"] = (s["clean"] * shade).astype(F)
    return s


def noisy_mean(s, n, K, rng):
    """(colour, variance): ``s['clean']`` as the mean of n samples of gamma(2, 0.5) noise (mean 1) on the hit pixels,
    taken in K batches; the variance of the mean luminance from the K batch means, NaN where K < 2.  n and K may be
    [H, W] arrays (a frame whose pixels stand at different counts)."""
    h, w = s["hit"].shape
    n, K = np.broadcast_to(n, (h, w)), np.broadcast_to(K, (h, w))
    clean = s["clean"].astype(np.float64)
    kmax = int(K.max())
    per = n // K
    # a batch of m samples of gamma(2, 0.5) has the mean gamma(2 m, 0.5 / m)
    means = rng.gamma(2.0 * per[None], 0.5 / per[None], size=(kmax, h, w))
    used = np.arange(kmax)[:, None, None] < K[None]
    mean = np.where(used, means, 0).sum(0) / K
    mean = np.where(s["hit"], mean, 1.0)
    color = (clean * mean[..., None]).astype(F)
    lum64 = clean @ np.array([0.212671, 0.715160, 0.072169])
    dev = np.where(used, means - mean[None], 0)
    with np.errstate(all="ignore"):
        var = (dev ** 2).sum(0) / (K - 1) / K * lum64 ** 2
    var = np.where((K >= 2) & s["hit"], var, np.nan).astype(F)
    return color, var


def rel_error(x, clean, where):
    """e = mean((x - clean)^2 / (clean^2 + 0.01)) over the pixels ``where``."""
    x, clean = np.asarray(x, np.float64), np.asarray(clean, np.float64)
    return float((((x - clean) ** 2) / (clean ** 2 + 0.01))[where].mean())
