"""The contract of vimg_despeckle_clamp (include/vimg_despeckle.h) restated in numpy float32: every + - * / is one
float32 operation in the header's order, every choice a comparison (np.where, never np.maximum / np.minimum, whose
NaN rules are not the comparison's).  The library must give these bits; tests/test_despeckle_abi.py pins this file on
its own."""
import numpy as np

from atrous_ref import _shifted

F = np.float32
KEPT, CLAMPED, FEW_TAPS, NOT_LIVE = 0, 1, 2, 3
LUM = (F(0.212671), F(0.715160), F(0.072169))


def clamp(color, normal, position, depth, albedo=None, *, radius, rank, min_taps, gain, sigma_normal, sigma_plane, albedo_floor):
    """[H, W, 3] float32 frames in, (the clamped [H, W, 3] frame, the [H, W] uint8 codes) out.  ``depth`` is the `depth`
    feature frame (t t t): its first component is read."""
    color, n, P = (np.asarray(a, dtype=F) for a in (color, normal, position))
    z = np.asarray(depth, dtype=F)[..., 0]
    R, rank, min_taps = int(radius), int(rank), int(min_taps)
    gain, sigma_normal, sigma_plane, floor = F(gain), F(sigma_normal), F(sigma_plane), F(albedo_floor)
    one, zero, inf = F(1), F(0), F(np.inf)
    with np.errstate(all="ignore"):
        # pack
        live = z > zero                                     # False for a miss and for a NaN depth
        if albedo is not None:
            albedo = np.asarray(albedo, dtype=F)
            a = np.where(albedo > floor, albedo, floor).astype(F)
            C = np.where(live[..., None], color / a, color).astype(F)
        else:
            C = color.copy()
        L = (C[..., 0] * LUM[0] + C[..., 1] * LUM[1]) + C[..., 2] * LUM[2]
        # clamp
        sz = sigma_plane * z
        plane_den = sz * sz
        m = np.zeros(z.shape, np.int64)
        total = np.zeros(z.shape, F)
        top = [np.full(z.shape, -inf, F) for _ in range(rank)]          # t_1 .. t_rank, descending
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                if dx == 0 and dy == 0:
                    continue
                zq = _shifted(z, dy, dx, zero)                          # outside the image: not live
                nq, Pq = (_shifted(a_, dy, dx, zero) for a_ in (n, P))
                Lq = _shifted(L, dy, dx, zero)
                dn = one - ((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
                s_n = np.where(dn < zero, zero, dn / sigma_normal)
                e = Pq - P
                d = (n[..., 0] * e[..., 0] + n[..., 1] * e[..., 1]) + n[..., 2] * e[..., 2]
                s_p = (d * d) / plane_den
                S = s_n + s_p
                ok = (zq > zero) & (S < one) & (Lq >= zero)
                m = np.where(ok, m + 1, m)
                total = np.where(ok, total + Lq, total)
                v = Lq
                for k in range(rank):
                    swap = ok & (v > top[k])
                    top[k], v = np.where(swap, v, top[k]), np.where(swap, top[k], v)
        enough = live & (m >= min_taps)
        mean = total / m.astype(F)
        b = np.where(mean > top[rank - 1], mean, top[rank - 1])
        T = gain * b
        hit = enough & (L > T) & (L < inf)
        f = T / L
        scaled = (C * f[..., None]) * a if albedo is not None else C * f[..., None]
        out = np.where(hit[..., None], scaled, color).astype(F)
        code = np.where(~live, NOT_LIVE, np.where(~enough, FEW_TAPS, np.where(hit, CLAMPED, KEPT))).astype(np.uint8)
    assert out.dtype == F
    return out, code


def luminance(x):
    """Rec. 709 luminance in float64, for the shares and means the tests and tools report."""
    x = np.asarray(x, np.float64)
    return x[..., 0] * 0.212671 + x[..., 1] * 0.715160 + x[..., 2] * 0.072169


def rel_error(x, ref):
    """DESIGN.md 4.18's relative squared error e = mean((x - ref)^2 / (ref^2 + 0.01)), in float64."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(((x - ref) ** 2 / (ref ** 2 + 0.01)).mean())


def speckled(frame, color, live, share=0.01, seed=5):
    """A dict of frames (atrous_ref.synthetic_frame's, infill_ref.creased_frames') with speckles injected into a copy of
    ``color``: ``share`` of the ``live`` pixels (at least one) multiplied by 10..1000, and - from 48 pixels on - a NaN,
    a +inf and a -inf colour, a NaN normal and a NaN depth on live pixels.  Returns a copy of the dict with ``color``
    set."""
    rng = np.random.default_rng(seed)
    color = np.array(color, dtype=F)
    h, w = color.shape[:2]
    ys, xs = np.nonzero(live)
    f = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in frame.items()}
    if len(ys):
        pick = rng.choice(len(ys), max(1, int(share * len(ys))), replace=False)
        color[ys[pick], xs[pick]] *= rng.uniform(10, 1000, (len(pick), 1)).astype(F)
    if h * w >= 48 and len(ys) > 8:
        spots = [(ys[i], xs[i]) for i in np.linspace(0, len(ys) - 1, 7).astype(int)[1:6]]
        color[spots[0]][1] = np.nan
        color[spots[1]] = np.inf
        color[spots[2]][0] = -np.inf
        f["normal"][spots[3]][0] = np.nan
        f["depth"][spots[4]] = np.nan
    f["color"] = color
    return f
