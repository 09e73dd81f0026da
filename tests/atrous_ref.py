"""The contract of vimg_filter_atrous (include/vimg_filter.h) restated in numpy float32: every + - * / is one
float32 operation in the header's order, every choice a comparison (np.where, never np.maximum / np.minimum, whose
NaN rules are not the comparison's).  The library must give these bits; tests/test_filter_abi.py pins this file on
its own."""
import numpy as np

F = np.float32
H5 = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))


def _shifted(a, dy, dx, fill):
    """a[y + dy, x + dx] where that is inside the image, `fill` elsewhere."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = slice(max(dy, 0), min(h + dy, h)), slice(max(-dy, 0), min(h - dy, h))
    xs, xd = slice(max(dx, 0), min(w + dx, w)), slice(max(-dx, 0), min(w - dx, w))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[yd, xd] = a[ys, xs]
    return out


def atrous(color, normal, position, depth, albedo=None, *, iterations, sigma_color, sigma_normal, sigma_plane, albedo_floor):
    """[H, W, 3] float32 frames in, the filtered [H, W, 3] frame out.  ``depth`` is the `depth` feature frame
    (t t t): its first component is read."""
    color, n, P = (np.asarray(a, dtype=F) for a in (color, normal, position))
    z = np.asarray(depth, dtype=F)[..., 0]
    sigma_color, sigma_normal, sigma_plane, floor = F(sigma_color), F(sigma_normal), F(sigma_plane), F(albedo_floor)
    one, zero = F(1), F(0)
    with np.errstate(all="ignore"):
        # pack
        if albedo is not None:
            albedo = np.asarray(albedo, dtype=F)
            a = np.where(albedo > floor, albedo, floor).astype(F)
            C = color / a
        else:
            C = color.copy()
        live = z > zero                                     # False for a miss and for a NaN depth
        sz = sigma_plane * z
        plane_den = sz * sz
        scale = F(1)
        for i in range(iterations):
            s = 1 << i
            sc = sigma_color * scale                        # sigma_color 2^-i, a float product
            color_den = sc * sc
            sumw = np.zeros(z.shape, F)
            sumc = np.zeros(C.shape, F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    k = H5[dx + 2] * H5[dy + 2]
                    if dx == 0 and dy == 0:
                        w, Cq = np.full(z.shape, k, F), C
                    else:
                        zq = _shifted(z, s * dy, s * dx, zero)          # outside the image: not live
                        nq, Pq, Cq = (_shifted(a_, s * dy, s * dx, zero) for a_ in (n, P, C))
                        dn = one - ((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
                        s_n = np.where(dn < zero, zero, dn / sigma_normal)
                        e = Pq - P
                        d = (n[..., 0] * e[..., 0] + n[..., 1] * e[..., 1]) + n[..., 2] * e[..., 2]
                        s_p = (d * d) / plane_den
                        dc = C - Cq
                        s_c = ((dc[..., 0] * dc[..., 0] + dc[..., 1] * dc[..., 1]) + dc[..., 2] * dc[..., 2]) / color_den
                        S = (s_n + s_p) + s_c
                        t = one - S
                        w = np.where(S < one, k * (t * t), zero)
                        w = np.where(zq > zero, w, zero).astype(F)
                    take = w > zero
                    sumw = np.where(take, sumw + w, sumw)
                    sumc = np.where(take[..., None], sumc + w[..., None] * Cq, sumc)
            C = np.where(live[..., None], sumc / sumw[..., None], C).astype(F)
            scale = scale * F(0.5)
        # unpack
        out = C * a if albedo is not None else C
    assert out.dtype == F
    return out


def synthetic_frame(h=64, w=96, seed=1):
    """A sphere over a checkered floor under a sky, seen from the origin: a dict with the clean frame, the noisy one
    (gamma(2, 0.5) noise, mean 1, on the shaded pixels) and the guides normal / position / depth / albedo, all
    [h, w, 3] float32; sky pixels are misses (every guide 0, not live) and carry the sky colour in both frames."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    dirs = np.stack([(xx - w / 2) / w, (h / 2 - yy) / w, -np.ones_like(xx)], -1)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    c, r = np.array([0.0, 0.0, -3.0]), 0.8
    b = dirs @ c
    disc = b * b - (c @ c - r * r)
    ts = np.where(disc > 0, b - np.sqrt(np.maximum(disc, 0)), np.inf)
    down = dirs[..., 1] < -1e-3
    tf = np.where(down, -0.8 / np.where(down, dirs[..., 1], -1.0), np.inf)          # the floor y = -0.8
    t = np.minimum(ts, tf)
    hit, ball = np.isfinite(t), ts < tf
    P = np.where(hit[..., None], dirs * np.where(hit, t, 0)[..., None], 0)
    nrm = np.where(hit[..., None], np.where(ball[..., None], (P - c) / r, np.array([0.0, 1.0, 0.0])), 0)
    checker = (np.floor(P[..., 0] * 2) + np.floor(P[..., 2] * 2)) % 2
    alb = np.where(ball[..., None], np.array([0.8, 0.3, 0.2]), np.where(checker[..., None] > 0, 0.9, 0.2) * np.ones(3))
    alb = np.where(hit[..., None], alb, 0)
    irr = np.clip(nrm @ np.array([0.3, 0.8, 0.5]), 0.05, None)[..., None] * np.ones(3)
    clean = np.where(hit[..., None], alb * irr, np.array([0.5, 0.7, 1.0]))
    noisy = clean * np.where(hit[..., None], rng.gamma(2.0, 0.5, size=(h, w, 1)), 1.0)
    depth = np.repeat(np.where(hit, t, 0)[..., None], 3, axis=-1)
    return {k: np.ascontiguousarray(v, dtype=F) for k, v in dict(clean=clean, noisy=noisy, normal=nrm, position=P, depth=depth,
                                                                albedo=alb).items()} | {"hit": hit}
