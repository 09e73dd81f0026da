"""The contract of vimg_moments_accumulate (include/vimg_moments.h) restated in numpy float32: every + - * / is one
float32 operation in the header's order, every choice a comparison (np.where, never np.maximum / np.minimum, whose
NaN rules are not the comparison's).  The library must give these bits; tests/test_moments_abi.py pins this file on
its own - planes 0..2 against tests/temporal_ref.py, plane 3 against closed forms and a statistical bound."""
import numpy as np

from temporal_ref import IDENTITY, flat_frames, shift_matrix  # noqa: F401  (the same helpers serve both restatements)

F = np.float32
NAN = np.uint32(0x7FC00000).view(F)          # the quiet NaN the contract writes for "unknown"
YR, YG, YB = F(0.212671), F(0.715160), F(0.072169)


def lum(c):
    c = np.asarray(c, dtype=F)
    return (c[..., 0] * YR + c[..., 1] * YG) + c[..., 2] * YB


def known(v):
    with np.errstate(invalid="ignore"):
        return (v >= F(0)) & (v < F(np.inf))


def accumulate(color, normal, position, depth, variance=None, prev=None, matrix=None, *, max_history, current_weight, sigma_normal,
               sigma_plane, min_history):
    """[H, W, 3] float32 frames, the [H, W] variance frame (or None), the previous history [4, H, W, 4] (or None) and
    its 12-float matrix in, the next history [4, H, W, 4] out: planes A = {rgb, L}, G0 = {n, z}, G1 = {P, 0},
    M = {m1, m2, V, 0}.  The library's rgb output is next[0, :, :, :3], its variance output next[3, :, :, 2]."""
    C, n, P = (np.asarray(a, dtype=F) for a in (color, normal, position))
    z = np.asarray(depth, dtype=F)[..., 0]
    h, w = z.shape
    max_history, cw, sigma_normal, sigma_plane = F(max_history), F(current_weight), F(sigma_normal), F(sigma_plane)
    min_history = F(min_history)
    one, zero, half = F(1), F(0), F(0.5)
    nxt = np.zeros((4, h, w, 4), F)
    nxt[1, ..., :3], nxt[1, ..., 3] = n, z
    nxt[2, ..., :3] = P
    live = z > zero                                            # False for a miss and for a NaN depth
    with np.errstate(all="ignore"):
        Lc = lum(C)
        x2 = Lc * Lc
        if variance is None:
            v, vk = np.zeros((h, w), F), np.zeros((h, w), bool)
        else:
            v = np.asarray(variance, dtype=F)
            vk = known(v)
            x2 = np.where(vk, x2 + v * (cw - one), x2)
    A = np.concatenate([C, np.where(live, one, zero).astype(F)[..., None]], axis=-1)       # no history: {C, 1} or {C, 0}
    V0 = np.where(live, np.where(vk, v, NAN), zero).astype(F)
    M = np.stack([Lc, x2, V0, np.zeros((h, w), F)], axis=-1)
    if prev is not None:
        prev = np.asarray(prev, dtype=F)
        Mx = np.asarray(matrix, dtype=F).reshape(12)
        with np.errstate(all="ignore"):
            hx = ((Mx[0] * P[..., 0] + Mx[1] * P[..., 1]) + Mx[2] * P[..., 2]) + Mx[3]
            hy = ((Mx[4] * P[..., 0] + Mx[5] * P[..., 1]) + Mx[6] * P[..., 2]) + Mx[7]
            hw = ((Mx[8] * P[..., 0] + Mx[9] * P[..., 1]) + Mx[10] * P[..., 2]) + Mx[11]
            fx = hx / hw - half
            fy = hy / hw - half
            seen = live & (hw > zero) & (fx > -one) & (fx < F(w)) & (fy > -one) & (fy < F(h))
            x0, y0 = np.floor(fx), np.floor(fy)
            tx, ty = fx - x0, fy - y0
            ux, uy = one - tx, one - ty
            ix, iy = (np.where(seen, q, zero).astype(np.int64) for q in (x0, y0))
            sz = sigma_plane * z
            plane = sz * sz
            sumb, suml, sumh = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w, 3), F)
            s1, s2 = np.zeros((h, w), F), np.zeros((h, w), F)
            for i, b in enumerate((ux * uy, tx * uy, ux * ty, tx * ty)):
                qx, qy = ix + (i & 1), iy + (i >> 1)
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                gx, gy = np.where(inside, qx, 0), np.where(inside, qy, 0)
                Aq, G0q, G1q, Mq = prev[0, gy, gx], prev[1, gy, gx], prev[2, gy, gx], prev[3, gy, gx]
                dn = one - ((n[..., 0] * G0q[..., 0] + n[..., 1] * G0q[..., 1]) + n[..., 2] * G0q[..., 2])
                e = G1q[..., :3] - P
                d = (n[..., 0] * e[..., 0] + n[..., 1] * e[..., 1]) + n[..., 2] * e[..., 2]
                take = seen & inside & (b > zero) & (Aq[..., 3] > zero) & (dn < sigma_normal) & (d * d < plane)
                sumb = np.where(take, sumb + b, sumb)
                sumh = np.where(take[..., None], sumh + b[..., None] * Aq[..., :3], sumh)
                suml = np.where(take, suml + b * Aq[..., 3], suml)
                s1 = np.where(take, s1 + b * Mq[..., 0], s1)
                s2 = np.where(take, s2 + b * Mq[..., 1], s2)
            found = seen & (sumb > zero)
            H = sumh / sumb[..., None]
            L = suml / sumb
            N = L + cw
            N = np.where(N > max_history, max_history, N)
            a = cw / N
            a = np.where(a > one, one, a)
            blend = np.concatenate([H + (C - H) * a[..., None], N[..., None]], axis=-1)
            m1h, m2h = s1 / sumb, s2 / sumb
            sh = m2h - m1h * m1h
            sh = np.where(sh < zero, zero, sh)
            Vh = sh / L
            m1 = m1h + (Lc - m1h) * a
            m2 = m2h + (x2 - m2h) * a
            sc = m2 - m1 * m1
            sc = np.where(sc < zero, zero, sc)
            Vc = np.where(vk, v, sc / cw)
            u = one - a
            V = (u * u) * Vh + (a * a) * Vc
            V = np.where(N >= min_history, V, NAN)
            moments = np.stack([m1, m2, V, np.zeros((h, w), F)], axis=-1)
        A = np.where(found[..., None], blend, A)
        M = np.where(found[..., None], moments, M)
    nxt[0], nxt[3] = A, M
    assert nxt.dtype == F
    return nxt
