"""The contract of vimg_infill_reconstruct (include/vimg_infill.h) restated in numpy float32: every + - * / is one
float32 operation in the header's order, every choice a comparison (np.where, never np.maximum / np.minimum, whose
NaN rules are not the comparison's).  The library must give these bits; tests/test_infill_abi.py pins this file on
its own."""
import numpy as np

from atrous_ref import _shifted

F = np.float32
SAMPLED, GUIDED, UNGUIDED, HOLE = 0, 1, 2, 3


def reconstruct(color, normal, position, depth, count, albedo=None, *, radius, sigma_normal, sigma_plane, albedo_floor):
    """[H, W, 3] float32 frames and the [H, W] sample counts in, (the filled [H, W, 3] frame, the [H, W] uint8 codes)
    out.  ``depth`` is the `depth` feature frame (t t t): its first component is read."""
    color, n, P = (np.asarray(a, dtype=F) for a in (color, normal, position))
    z = np.asarray(depth, dtype=F)[..., 0]
    sampled = np.asarray(count) > 0
    R = int(radius)
    sigma_normal, sigma_plane, floor = F(sigma_normal), F(sigma_plane), F(albedo_floor)
    one, zero = F(1), F(0)
    with np.errstate(all="ignore"):
        # pack
        live = z > zero                                     # False for a miss and for a NaN depth
        if albedo is not None:
            albedo = np.asarray(albedo, dtype=F)
            a = np.where(albedo > floor, albedo, floor).astype(F)
            C = np.where(live[..., None], color / a, color).astype(F)
        else:
            C = color.copy()
        # fill
        sz = sigma_plane * z
        plane_den = sz * sz
        gw, fw = np.zeros(z.shape, F), np.zeros(z.shape, F)
        gc, fc = np.zeros(C.shape, F), np.zeros(C.shape, F)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                k = F((R + 1 - abs(dx)) * (R + 1 - abs(dy)))
                sq = _shifted(sampled, dy, dx, False)               # outside the image: not sampled
                zq = _shifted(z, dy, dx, zero)
                nq, Pq, Cq = (_shifted(a_, dy, dx, zero) for a_ in (n, P, C))
                # the unguided sums: every sampled tap
                fw = np.where(sq, fw + k, fw)
                fc = np.where(sq[..., None], fc + k * Cq, fc)
                # the guided sums: the sampled taps of p's own kind
                dn = one - ((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
                s_n = np.where(dn < zero, zero, dn / sigma_normal)
                e = Pq - P
                d = (n[..., 0] * e[..., 0] + n[..., 1] * e[..., 1]) + n[..., 2] * e[..., 2]
                s_p = (d * d) / plane_den
                S = s_n + s_p
                t = one - S
                w = np.where(live, np.where(S < one, k * (t * t), zero), k).astype(F)
                take = sq & ((zq > zero) == live) & (w > zero)
                gw = np.where(take, gw + w, gw)
                gc = np.where(take[..., None], gc + w[..., None] * Cq, gc)
        guided, any_tap = gw > zero, fw > zero
        Cp = np.where(guided[..., None], gc / gw[..., None], np.where(any_tap[..., None], fc / fw[..., None], zero)).astype(F)
        code = np.where(sampled, SAMPLED, np.where(guided, GUIDED, np.where(any_tap, UNGUIDED, HOLE))).astype(np.uint8)
        filled = np.where(live[..., None], Cp * a, Cp) if albedo is not None else Cp
        out = np.where(sampled[..., None], color, filled).astype(F)
    assert out.dtype == F
    return out, code


def tent_fill(color, count, radius):
    """The fill without guides, in float64: every unsampled pixel gets the tent-weighted mean of the sampled pixels
    within ``radius`` (0 0 0 when there is none) - what the guided fill is measured against."""
    color = np.asarray(color, dtype=np.float64)
    sampled = np.asarray(count) > 0
    R = int(radius)
    sw, sc = np.zeros(sampled.shape), np.zeros(color.shape)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            k = float((R + 1 - abs(dx)) * (R + 1 - abs(dy)))
            sq = _shifted(sampled, dy, dx, False)
            sw += np.where(sq, k, 0.0)
            sc += np.where(sq[..., None], k * _shifted(color, dy, dx, 0.0), 0.0)
    mean = sc / np.where(sw > 0, sw, 1.0)[..., None]
    return np.where(sampled[..., None], color, mean)


def lattice(h, w, stride, cx=0, cy=0):
    """[h, w] bool: True where (x % stride, y % stride) == (cx, cy)."""
    m = np.zeros((h, w), bool)
    m[cy::stride, cx::stride] = True
    return m


def rel_error(x, ref, where=None):
    """DESIGN.md 4.18's relative squared error e = mean((x - ref)^2 / (ref^2 + 0.01)), in float64."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    e = (x - ref) ** 2 / (ref ** 2 + 0.01)
    return float(e.mean() if where is None else e[where].mean())


def creased_frames(h, w, seed=0):
    """Synthetic frames for the bit-level tests: two planes that meet at a crease (a vertical fold at x = w / 2: the
    normal turns by some 60 degrees), a depth step (the lower third of the right plane stands a unit nearer), a block
    of misses in the upper left corner, and - from 8 x 6 on - a NaN depth, a NaN normal and albedo at and below the
    floor somewhere.  ``color`` is albedo x a smooth irradiance that differs per plane, with noise; a dict of
    [h, w, 3] float32 arrays."""
    rng = np.random.default_rng(1000 * h + w + seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    left = xx < w / 2
    n = np.where(left[..., None], np.array([0.5, 0.0, 0.8660254]), np.array([-0.5, 0.0, 0.8660254])) + 0.01 * rng.normal(size=(h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    z = 5.0 + 0.03 * np.abs(xx - w / 2) + 0.01 * yy
    step = ~left & (yy >= 2 * h / 3)
    z = np.where(step, z - 1.0, z)
    P = np.stack([0.05 * (xx - w / 2), 0.05 * (h / 2 - yy), -z], -1) * (z / 5.0)[..., None]
    albedo = rng.uniform(0.05, 0.9, (h, w, 3))
    irr = np.where(left, 1.5, 0.4) + np.where(step, 0.8, 0.0) + 0.1 * np.sin(yy / 3.0)
    color = albedo * irr[..., None] * rng.gamma(8.0, 1 / 8, (h, w, 3))
    miss = (xx < w / 4) & (yy < h / 3) if h * w >= 48 else np.zeros((h, w), bool)
    color = np.where(miss[..., None], np.array([0.5, 0.7, 1.0]) + 0.05 * rng.normal(size=(h, w, 3)), color)
    f = {k: np.ascontiguousarray(v, dtype=F) for k, v in dict(color=color, normal=n, position=P, albedo=albedo,
                                                             depth=np.repeat(z[..., None], 3, -1)).items()}
    for k in ("normal", "position", "depth", "albedo"):
        f[k][miss] = 0
    if h * w >= 48:
        f["depth"][h - 1, w // 3] = np.nan
        f["normal"][h // 2, w - 2][0] = np.nan
        f["albedo"][h - 2, 1] = (0.0, 0.01, 0.0199)
        f["depth"][h // 2, 2][1:] = (0.0, np.nan)          # only the first component is read: this pixel is live
    return f
