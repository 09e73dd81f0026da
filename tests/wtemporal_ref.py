"""The contract of vimg_wtemporal_accumulate (include/vimg_wtemporal.h) restated in numpy float32: every + - * / is one
float32 operation in the header's order, every choice a comparison (np.where, never np.maximum / np.minimum, whose
NaN rules are not the comparison's).  The library must give these bits; tests/test_wtemporal_abi.py pins this file on
its own - among other things against tests/temporal_ref.py, whose bits it gives when every weight is one value >= 1."""
import numpy as np

F = np.float32
DEAD, STARTED, BLENDED, CARRIED, SHOWN = 0, 1, 2, 3, 4


def accumulate(color, normal, position, depth, weight, prev=None, matrix=None, *, max_history, sigma_normal, sigma_plane):
    """[H, W, 3] float32 frames, the [H, W] float32 weights, the previous history [3, H, W, 4] (or None) and its
    12-float matrix in; (the next history [3, H, W, 4], the [H, W] uint8 codes) out.  Planes A = {rgb, L},
    G0 = {n, z}, G1 = {P, 0}; ``depth`` is the `depth` feature frame (t t t): its first component is read.  The
    library's rgb output is next[0, :, :, :3]."""
    C, n, P = (np.asarray(a, dtype=F) for a in (color, normal, position))
    z = np.asarray(depth, dtype=F)[..., 0]
    wp = np.asarray(weight, dtype=F)
    h, w = z.shape
    assert wp.shape == (h, w)
    max_history, sigma_normal, sigma_plane = F(max_history), F(sigma_normal), F(sigma_plane)
    one, zero, half = F(1), F(0), F(0.5)
    nxt = np.zeros((3, h, w, 4), F)
    nxt[1, ..., :3], nxt[1, ..., 3] = n, z
    nxt[2, ..., :3] = P
    with np.errstate(all="ignore"):
        wt = np.where(wp > zero, wp, zero).astype(F)               # a NaN or negative weight is 0
        live = z > zero                                            # False for a miss and for a NaN depth
        worth = wt > zero
        start = np.where(worth, np.where(wt < one, wt, one), zero).astype(F)
        A = np.concatenate([C, np.where(live, start, zero).astype(F)[..., None]], axis=-1)   # no history: {C, min(wt, 1)} or {C, 0}
        code = np.where(live, np.where(worth, STARTED, SHOWN), DEAD).astype(np.uint8)
        if prev is not None:
            prev = np.asarray(prev, dtype=F)
            M = np.asarray(matrix, dtype=F).reshape(12)
            hx = ((M[0] * P[..., 0] + M[1] * P[..., 1]) + M[2] * P[..., 2]) + M[3]
            hy = ((M[4] * P[..., 0] + M[5] * P[..., 1]) + M[6] * P[..., 2]) + M[7]
            hw = ((M[8] * P[..., 0] + M[9] * P[..., 1]) + M[10] * P[..., 2]) + M[11]
            fx = hx / hw - half
            fy = hy / hw - half
            seen = live & (hw > zero) & (fx > -one) & (fx < F(w)) & (fy > -one) & (fy < F(h))
            x0, y0 = np.floor(fx), np.floor(fy)
            tx, ty = fx - x0, fy - y0
            ux, uy = one - tx, one - ty
            ix, iy = (np.where(seen, v, zero).astype(np.int64) for v in (x0, y0))
            sz = sigma_plane * z
            plane = sz * sz
            sumb, suml, sumh = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w, 3), F)
            for i, b in enumerate((ux * uy, tx * uy, ux * ty, tx * ty)):
                qx, qy = ix + (i & 1), iy + (i >> 1)
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                gx, gy = np.where(inside, qx, 0), np.where(inside, qy, 0)
                Aq, G0q, G1q = prev[0, gy, gx], prev[1, gy, gx], prev[2, gy, gx]
                dn = one - ((n[..., 0] * G0q[..., 0] + n[..., 1] * G0q[..., 1]) + n[..., 2] * G0q[..., 2])
                e = G1q[..., :3] - P
                d = (n[..., 0] * e[..., 0] + n[..., 1] * e[..., 1]) + n[..., 2] * e[..., 2]
                take = seen & inside & (b > zero) & (Aq[..., 3] > zero) & (dn < sigma_normal) & (d * d < plane)
                sumb = np.where(take, sumb + b, sumb)
                sumh = np.where(take[..., None], sumh + b[..., None] * Aq[..., :3], sumh)
                suml = np.where(take, suml + b * Aq[..., 3], suml)
            found = seen & (sumb > zero)
            H = sumh / sumb[..., None]
            L = suml / sumb
            # a pixel whose colour is worth something: the blend
            N = L + wt
            N = np.where(N > max_history, max_history, N)
            a = wt / N
            a = np.where(a > one, one, a)
            blend = np.concatenate([H + (C - H) * a[..., None], N[..., None]], axis=-1)
            # ... and one whose colour is worth nothing: the history alone
            K = np.where(L > max_history, max_history, L)
            carry = np.concatenate([H, K[..., None]], axis=-1)
            A = np.where((found & worth)[..., None], blend, np.where((found & ~worth)[..., None], carry, A))
            code = np.where(found, np.where(worth, BLENDED, CARRIED), code).astype(np.uint8)
    nxt[0] = A
    assert nxt.dtype == F and code.dtype == np.uint8
    return nxt, code
