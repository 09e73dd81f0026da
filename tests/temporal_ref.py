"""The contract of vimg_temporal_accumulate (include/vimg_temporal.h) restated in numpy float32: every + - * / is one
float32 operation in the header's order, every choice a comparison (np.where, never np.maximum / np.minimum, whose
NaN rules are not the comparison's).  The library must give these bits; tests/test_temporal_abi.py pins this file on
its own."""
import numpy as np

F = np.float32
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1], F)      # hx = P.x, hy = P.y, hw = 1


def accumulate(color, normal, position, depth, prev=None, matrix=None, *, max_history, current_weight, sigma_normal, sigma_plane):
    """[H, W, 3] float32 frames, the previous history [3, H, W, 4] (or None) and its 12-float matrix in, the next
    history [3, H, W, 4] out: planes A = {rgb, L}, G0 = {n, z}, G1 = {P, 0}.  ``depth`` is the `depth` feature frame
    (t t t): its first component is read.  The library's rgb output is next[0, :, :, :3]."""
    C, n, P = (np.asarray(a, dtype=F) for a in (color, normal, position))
    z = np.asarray(depth, dtype=F)[..., 0]
    h, w = z.shape
    max_history, cw, sigma_normal, sigma_plane = F(max_history), F(current_weight), F(sigma_normal), F(sigma_plane)
    one, zero, half = F(1), F(0), F(0.5)
    nxt = np.zeros((3, h, w, 4), F)
    nxt[1, ..., :3], nxt[1, ..., 3] = n, z
    nxt[2, ..., :3] = P
    live = z > zero                                            # False for a miss and for a NaN depth
    A = np.concatenate([C, np.where(live, one, zero).astype(F)[..., None]], axis=-1)       # no history: {C, 1} or {C, 0}
    if prev is not None:
        prev = np.asarray(prev, dtype=F)
        M = np.asarray(matrix, dtype=F).reshape(12)
        with np.errstate(all="ignore"):
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
            N = L + cw
            N = np.where(N > max_history, max_history, N)
            a = cw / N
            a = np.where(a > one, one, a)
            blend = np.concatenate([H + (C - H) * a[..., None], N[..., None]], axis=-1)
        A = np.where(found[..., None], blend, A)
    nxt[0] = A
    assert nxt.dtype == F
    return nxt


def flat_frames(h, w, color, depth=8.0):
    """A wall facing the viewer whose position frame lies on pixel centres, P = (x + 0.5, y + 0.5, -depth): under
    IDENTITY every pixel reprojects onto itself with tx = ty = 0."""
    yy, xx = np.mgrid[0:h, 0:w]
    position = np.stack([xx + 0.5, yy + 0.5, np.full((h, w), -depth)], -1).astype(F)
    normal = np.zeros((h, w, 3), F)
    normal[..., 2] = 1
    return dict(color=np.broadcast_to(np.asarray(color, F), (h, w, 3)).copy(), normal=normal, position=position,
                depth=np.full((h, w, 3), depth, F))


def shift_matrix(dx, dy=0.0):
    """IDENTITY moved: a point reprojects dx columns and dy rows from where it is now."""
    m = IDENTITY.copy()
    m[3], m[7] = dx, dy
    return m


def synthetic_sequence(h=16, w=32, frames=4, seed=1, focal=16.0, step=0.5):
    """A wall at z = -8 and a box in front of it at z = -4, both facing a pinhole camera that looks along -z and moves
    along +x by `step` per frame: the wall moves focal step / 8 = 1 pixel per frame to the left, the box 2, so wall
    behind the box comes into view.  The two top rows see past the wall (misses: guides 0).  Every position lies on a
    pixel centre's ray and focal, depths and step are powers of two, so the projections are exact in float32: each
    pixel reprojects onto a pixel centre (tx = ty = 0).  A list of dicts per frame: color (clean times seeded gamma
    noise on the surfaces), clean (a function of the world position), normal, position, depth [h, w, 3] float32,
    matrix (the frame's own world-to-pixel, 12 floats), box and hit (bool masks)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = (xx + 0.5 - w / 2) / focal, (yy + 0.5 - h / 2) / focal
    out = []
    for i in range(frames):
        cx = i * step
        bx, by = cx + 4 * u, 4 * v                                             # where the ray meets z = -4
        box = (bx >= -0.5) & (bx < 1.0) & (by >= -0.75) & (by < 0.75)
        hit = box | (yy >= 2)
        t = np.where(box, 4.0, 8.0)
        P = np.stack([cx + t * u, t * v, -t], -1)
        wall = 0.25 + 0.5 * ((np.floor(P[..., 0] * 2) + np.floor(P[..., 1] * 2)) % 2)
        clean = np.where(box[..., None], np.array([0.8, 0.3, 0.2]), wall[..., None] * np.array([0.5, 0.75, 1.0]))
        clean = np.where(hit[..., None], clean, np.array([0.5, 0.7, 1.0]))
        noisy = clean * np.where(hit[..., None], rng.gamma(2.0, 0.5, size=(h, w, 1)), 1.0)
        normal = np.where(hit[..., None], np.array([0.0, 0.0, 1.0]), 0.0)
        f = {k: np.ascontiguousarray(a, dtype=F) for k, a in dict(
            color=noisy, clean=clean, normal=normal, position=np.where(hit[..., None], P, 0.0),
            depth=np.repeat(np.where(hit, t, 0.0)[..., None], 3, -1)).items()}
        f["matrix"] = np.array([focal, 0, -w / 2, -focal * cx, 0, focal, -h / 2, 0, 0, 0, -1, 0], F)
        f["box"], f["hit"] = box, hit
        out.append(f)
    return out
