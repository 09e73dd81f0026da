"""The contract of vimg_demand_mask (include/vimg_demand.h) restated in numpy float32: every + - * / is one float32
operation in the header's order, every choice a comparison (np.where, never np.maximum / np.minimum, whose NaN rules are
not the comparison's).  The library must give these bits; tests/test_demand_abi.py pins this file on its own - among
other things against tests/wtemporal_ref.py, whose carried lengths it gives."""
import numpy as np

F = np.float32
DEFAULTS = dict(stride=2, phase=0, min_history=1.0, sigma_normal=0.1, sigma_plane=0.00005)
COUNTS = ("masked", "needed", "extra", "live")


def cell(stride, phase):
    """(cx, cy) of the header: integers."""
    return phase % stride, (phase // stride + phase % stride) % stride


def lattice(h, w, stride, phase):
    """lat of the header as an [h, w] bool array; stride 0: nowhere."""
    lat = np.zeros((h, w), bool)
    if stride != 0:
        cx, cy = cell(stride, phase)
        yy, xx = np.mgrid[0:h, 0:w]
        lat = (xx % stride == cx) & (yy % stride == cy)
    return lat


def length(normal, position, depth, prev=None, matrix=None, *, sigma_normal, sigma_plane):
    """L of the header, [H, W] float32: the history length vimg_temporal.h's lookup finds, 0 where it finds none or the
    pixel is not live."""
    n, P = (np.asarray(a, dtype=F) for a in (normal, position))
    z = np.asarray(depth, dtype=F)[..., 0]
    h, w = z.shape
    sigma_normal, sigma_plane = F(sigma_normal), F(sigma_plane)
    one, zero, half = F(1), F(0), F(0.5)
    L = np.zeros((h, w), F)
    if prev is None:
        return L
    prev = np.asarray(prev, dtype=F)
    M = np.asarray(matrix, dtype=F).reshape(12)
    with np.errstate(all="ignore"):
        live = z > zero
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
        sumb, suml = np.zeros((h, w), F), np.zeros((h, w), F)
        for i, b in enumerate((ux * uy, tx * uy, ux * ty, tx * ty)):
            qx, qy = ix + (i & 1), iy + (i >> 1)
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            gx, gy = np.where(inside, qx, 0), np.where(inside, qy, 0)
            Lq, G0q, G1q = prev[0, gy, gx, 3], prev[1, gy, gx], prev[2, gy, gx]
            dn = one - ((n[..., 0] * G0q[..., 0] + n[..., 1] * G0q[..., 1]) + n[..., 2] * G0q[..., 2])
            e = G1q[..., :3] - P
            d = (n[..., 0] * e[..., 0] + n[..., 1] * e[..., 1]) + n[..., 2] * e[..., 2]
            take = seen & inside & (b > zero) & (Lq > zero) & (dn < sigma_normal) & (d * d < plane)
            sumb = np.where(take, sumb + b, sumb)
            suml = np.where(take, suml + b * Lq, suml)
        found = seen & (sumb > zero)
        L = np.where(found, suml / sumb, zero).astype(F)
    return L


def mask(normal, position, depth, prev=None, matrix=None, *, stride=2, phase=0, min_history=1.0, sigma_normal=0.1,
         sigma_plane=0.00005):
    """[H, W, 3] float32 guides, the previous history [3, H, W, 4] (or None) and its 12-float matrix in; (mask [H, W]
    uint8, length [H, W] float32, counts uint32[4]: masked, needed, extra, live) out."""
    z = np.asarray(depth, dtype=F)[..., 0]
    h, w = z.shape
    assert stride == 0 and phase == 0 or 2 <= stride <= 4 and 0 <= phase < stride * stride
    with np.errstate(invalid="ignore"):
        live = z > F(0)
        L = length(normal, position, depth, prev, matrix, sigma_normal=sigma_normal, sigma_plane=sigma_plane)
        need = live & (L < F(min_history))
    lat = lattice(h, w, stride, phase)
    m = (lat | need).astype(np.uint8)
    counts = np.array([m.sum(), need.sum(), (need & ~lat).sum(), live.sum()], np.uint32)
    assert L.dtype == F
    return m, L, counts


def read(counts):
    return {k: int(v) for k, v in zip(COUNTS, np.asarray(counts).view(np.uint32))}


def planted(h, w, seed=0, step=1.25, infinite=True):
    """A previous history and current guides of h x w with everything that can go wrong planted, as far as the frame has
    room.  A wall facing the viewer, P = (x + 0.5, y + 0.5, -8); the matrix shifts a point by ``step`` columns and 0.75 rows
    (fractional: four taps with b > 0), so the right and bottom edges look past the history or keep one or two taps of
    it.  History lengths are random in 0.25 .. 6 with zeros, negatives, NaNs and (``infinite``) an inf planted; the guides
    get misses, NaN normals, positions and depths, a flipped normal, a plane offset, and positions that project behind
    the camera (the matrix's last row reads P.z), off every edge and into (w - 1, w).  Returns (guides dict, prev,
    matrix)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    P = np.stack([xx + 0.5, yy + 0.5, np.full((h, w), -8.0)], -1).astype(F)
    n = np.zeros((h, w, 3), F)
    n[..., 2] = 1
    z = np.full((h, w), 8.0, F)
    prev = np.zeros((3, h, w, 4), F)
    prev[0, ..., :3] = rng.uniform(0, 1, (h, w, 3))
    prev[0, ..., 3] = rng.uniform(0.25, 6.0, (h, w))
    prev[1, ..., :3], prev[1, ..., 3] = n, z
    prev[2, ..., :3] = P
    # hx = 8 (P.x + step), hy = 8 (P.y + 0.75), hw = -P.z = 8: a perspective divide that is exact for this wall
    matrix = np.array([8, 0, 0, 8 * step, 0, 8, 0, 6.0, 0, 0, -1, 0], F)
    cur = dict(normal=n.copy(), position=P.copy(), depth=np.repeat(z[..., None], 3, -1).copy())
    flat = [(y, x) for y in range(h) for x in range(w)]
    picks = iter(rng.permutation(len(flat)))

    def some(k):
        return [flat[i] for i, _ in zip(picks, range(k))]

    few = max(1, (h * w) // 40)
    for y, x in some(few):
        prev[0, y, x, 3] = 0                                   # history lengths: nothing to carry
    for y, x in some(few):
        prev[0, y, x, 3] = -2
    for y, x in some(few):
        prev[0, y, x, 3] = np.nan
    for y, x in some(1 if infinite else 0):
        prev[0, y, x, 3] = np.inf
    for y, x in some(few):
        prev[0, y, x, :3] = np.nan                             # a NaN history colour decides nothing
    for y, x in some(few):
        prev[1, y, x, :3] = (0, 0, -1)                         # the history's surface faces away
    for y, x in some(few):
        prev[2, y, x, 2] = -8.5                                # ... or lies off the plane
    for y, x in some(few):
        cur["depth"][y, x] = 0                                 # misses
        cur["normal"][y, x] = 0
    for y, x in some(few):
        cur["depth"][y, x] = np.nan
    for y, x in some(few):
        cur["depth"][y, x] = -3
    for y, x in some(few):
        cur["normal"][y, x, 1] = np.nan
    for y, x in some(few):
        cur["position"][y, x, 0] = np.nan
    for y, x in some(few):
        cur["position"][y, x, 2] = 8                           # behind the old camera: hw = -8
    for y, x in some(few):
        cur["position"][y, x, 2] = 0                           # hw = 0
    for (y, x), px in zip(some(6), (-step - 0.75, -step - 2.0, w - step - 0.25, w - step + 0.5, w - step - 0.75, -step - 0.25)):
        cur["position"][y, x, 0] = px + 0.5                    # fx = -0.75, -2, w - 0.25, w + 0.5, w - 0.75, -0.25
    for (y, x), py in zip(some(4), (-1.5, -3.0, h - 1.0, h + 0.25)):
        cur["position"][y, x, 1] = py + 0.5                    # fy = -0.75, -2.25, h - 0.25, h + 1
    return cur, prev, matrix
