"""The contract of include/vimg_motion.h restated in numpy, float32 operation for operation: every + - * / below is one
IEEE float32 operation on float32 arrays, in the header's order, so the result is the library's bit for bit."""
import numpy as np

F = np.float32
NO_HIT = 0xFFFFFFFF
TRIANGLE, SPHERE = 0, 1
STATIC, MOVED_TRIANGLE, MOVED_SPHERE, OUT_OF_RANGE = 0, 1, 2, 3


def hit_records(t, prim, b1, b2):
    """[N, 4] float32 VimgRayHit records {t, prim, b1, b2}: prim's uint32 bits in the second float."""
    n = len(prim)
    h = np.zeros((n, 4), F)
    h[:, 0], h[:, 2], h[:, 3] = t, b1, b2
    h.view(np.uint32)[:, 1] = np.asarray(prim, np.uint32)
    return h


def previous_position(position, hits, rays, prims, tri_vertices, num_vertices, num_spheres, old_vertices=None, new_vertices=None,
                      old_spheres=None, new_spheres=None):
    """(Q [H, W, 3] float32, code [H, W] uint8).  ``position`` [H, W, 3]; ``hits`` [H * W, 4] float32 records; ``rays``
    [H * W, 8] or None; ``prims`` [num_prims, 2] and ``tri_vertices`` [num_tris, 3] uint32; the old / new tables float32
    or None, pairwise."""
    assert (old_vertices is None) == (new_vertices is None) and (old_spheres is None) == (new_spheres is None)
    h, w = position.shape[:2]
    n = h * w
    P = np.ascontiguousarray(position, F).reshape(n, 3)
    hits = np.ascontiguousarray(hits, F).reshape(n, 4)
    prims = np.asarray(prims, np.uint32).reshape(-1, 2)
    tri_vertices = np.asarray(tri_vertices, np.uint32).reshape(-1, 3)
    t, b1, b2 = hits[:, 0], hits[:, 2], hits[:, 3]
    prim = hits.view(np.uint32)[:, 1].astype(np.int64)
    D = np.zeros((n, 3), F)
    code = np.zeros(n, np.uint8)
    hit = prim != NO_HIT
    code[hit] = OUT_OF_RANGE
    known = hit & (prim < len(prims))
    kind, index = np.zeros(n, np.int64), np.zeros(n, np.int64)
    kind[known], index[known] = prims[prim[known], 0], prims[prim[known], 1]

    tri = known & (kind == TRIANGLE) & (index < len(tri_vertices))
    rows = np.zeros((n, 3), np.int64)
    rows[tri] = tri_vertices[index[tri]]
    tri &= (rows < num_vertices).all(axis=1)
    code[tri] = MOVED_TRIANGLE
    if old_vertices is not None and tri.any():
        old, new = np.asarray(old_vertices, F).reshape(-1, 3), np.asarray(new_vertices, F).reshape(-1, 3)
        r = rows[tri]
        e0, e1, e2 = (old[r[:, k]] - new[r[:, k]] for k in range(3))
        c1, c2 = b1[tri][:, None], b2[tri][:, None]
        w0 = (F(1) - c1) - c2
        with np.errstate(all="ignore"):
            D[tri] = (w0 * e0 + c1 * e1) + c2 * e2

    sph = known & (kind == SPHERE) & (index < num_spheres)
    code[sph] = MOVED_SPHERE
    if old_spheres is not None and sph.any():
        old, new = np.asarray(old_spheres, F).reshape(-1, 4)[index[sph]], np.asarray(new_spheres, F).reshape(-1, 4)[index[sph]]
        rays_s = np.ascontiguousarray(rays, F).reshape(n, 8)[sph]
        with np.errstate(all="ignore"):
            d = old[:, :3] - new[:, :3]
            u = (rays_s[:, 0:3] + t[sph][:, None] * rays_s[:, 4:7]) - new[:, :3]
            s = (old[:, 3] / new[:, 3])[:, None]
            scaled = d + (u * s - u)
        D[sph] = np.where((new[:, 3] > 0)[:, None], scaled, d)

    zero = (D == 0).all(axis=1)
    with np.errstate(all="ignore"):
        Q = np.where(zero[:, None], P, P + D)
    code[zero & (code != OUT_OF_RANGE)] = STATIC
    return Q.reshape(h, w, 3), code.reshape(h, w)
