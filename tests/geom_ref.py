"""TEST INFRASTRUCTURE: a float64 brute-force intersector, written from textbook geometry (numpy, vectorised) so
that the walk, the intersectors and the trees of the oracle and of the kernels can be held to something that is
none of them.  It has no tree: every ray meets every primitive.  The algorithms differ from the code under test on
purpose: ray / triangle is Moeller-Trumbore (the code under test shears the triangle into ray space and signs
three edge functions), ray / sphere projects the centre on the ray and takes both roots (the code under test solves
the quadratic in its numerically stable one-root form).

A sphere contributes two candidates to a ray, one per root; a triangle one.  Per candidate the model gives

  t          the ray parameter (of the direction AS GIVEN, not normalised); +inf where there is none
  b1, b2     the weights of the triangle's 2nd and 3rd vertex (tri_hit_info's convention); 0 for a sphere
  n          the geometric normal: normalize((p1 - p0) x (p2 - p0)), never turned towards the ray; for a sphere
             the outward normal at the root
  clear      the clearance, signed: for a triangle the distance in its plane from the hit point to the nearest
             edge (negative outside); for a sphere radius - closest approach of the ray's LINE to the centre
             (negative: the line passes by)
  dn         |d . n| for the unit direction
  S          the largest operand: the largest magnitude among the origin's coordinates, the primitive's and t
  bound      the error a float32 evaluation may have in t and in p = o + t d (see `_bound`)

and, against a range [t_min, t_max], whether the candidate is a hit in float64, a ROBUST hit (every clearance -
to the edges or the limb, to t_min and to t_max - exceeds delta) or a ROBUST miss (the ray passes the primitive,
or the candidate leaves the range, by more than delta).  delta = DELTA x the bound.  What is neither is the fringe
that no float32 intersector is asked about."""
import ctypes as C

import numpy as np

F = np.float64
EPS = 2.0 ** -24                  # unit round-off of float32
TOL = 32 * EPS                    # "32 ulp" of an operand of size 1
DELTA = 4.0                       # robust = clear by DELTA x the bound
PARALLEL = 1e-9                   # |d . n| below this: the ray runs in (or beside) the triangle's plane


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


def _absmax(*arrays):
    out = None
    for a in arrays:
        m = np.abs(a).max(axis=-1)
        out = m if out is None else np.maximum(out, m)
    return out


def _bound(S, dn):
    """The error bound of t and p: 32 ulp of the largest operand, over |d . n|.  A float32 intersector holds the
    ray's distance to the primitive's surface (the plane of a triangle, the sphere along its normal) to a few ulp
    of the operands it subtracts - the origin, the primitive's coordinates, the point o + t d - whatever its
    algorithm; the ray parameter is that distance divided by |d . n|, and so is the hit point along the ray."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return TOL * S / dn


class Geometry:
    """Triangles [T, 3, 3] and spheres [S, 4] (centre, radius) in float64, and the primitive id of each."""

    def __init__(self, verts, tris, spheres, tri_prim=None, sph_prim=None):
        verts = np.asarray(verts, F).reshape(-1, 3)
        tris = np.asarray(tris, np.int64).reshape(-1, 3)
        self.tri = verts[tris] if len(tris) else np.zeros((0, 3, 3), F)
        self.sph = np.asarray(spheres, F).reshape(-1, 4)
        nt, ns = len(self.tri), len(self.sph)
        self.tri_prim = np.arange(nt) if tri_prim is None else np.asarray(tri_prim, np.int64)
        self.sph_prim = nt + np.arange(ns) if sph_prim is None else np.asarray(sph_prim, np.int64)
        n = nt + ns
        self.kind = np.zeros(n, np.int64)              # 0 triangle, 1 sphere
        self.local = np.zeros(n, np.int64)             # index into tri / sph
        self.kind[self.sph_prim] = 1
        self.local[self.tri_prim] = np.arange(nt)
        self.local[self.sph_prim] = np.arange(ns)
        # candidate columns of a sweep: the triangles, the spheres' near roots, the spheres' far roots
        self.col_prim = np.concatenate([self.tri_prim, self.sph_prim, self.sph_prim])

    @property
    def num_prims(self):
        return len(self.kind)

    @classmethod
    def of_scene(cls, scene, verts=None, spheres=None):
        """What HostScene.geometry() and view.prims give; `verts` / `spheres` replace the positions (the arrays a
        test sent to a resident scene itself)."""
        v = scene.view.contents
        prims = np.ctypeslib.as_array(C.cast(v.prims, C.POINTER(C.c_uint32)), (v.num_prims, 2)).astype(np.int64)
        gv, _, gs = scene.geometry()
        verts = gv if verts is None else verts
        spheres = gs if spheres is None else spheres
        tris = np.zeros((0, 3), np.int64)
        if v.num_tris:
            idx = np.ctypeslib.as_array(v.tri_indices, (v.num_tris, 3)).astype(np.int64)
            mesh_of = np.ctypeslib.as_array(v.tri_mesh, (v.num_tris,)).astype(np.int64)
            first = np.array([v.meshes[i].first_vertex for i in range(v.num_meshes)], np.int64)
            tris = idx + first[mesh_of][:, None]
        is_sph = prims[:, 0] == 1
        tri_prim = np.empty(len(tris), np.int64)
        tri_prim[prims[~is_sph, 1]] = np.nonzero(~is_sph)[0]
        sph_prim = np.empty(len(spheres), np.int64)
        sph_prim[prims[is_sph, 1]] = np.nonzero(is_sph)[0]
        return cls(verts, tris, np.asarray(spheres, F).reshape(-1, 4)[:, :4], tri_prim, sph_prim)


def split_rays(rays):
    """[N, 8] float32 VimgRay records (org, t_min, dir, t_max) -> float64 o, d, t_min, t_max."""
    r = np.asarray(rays, F)
    return r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7]


# ------------------------------------------------------------------------------------------ the two intersections
def tri_candidates(o, d, p0, p1, p2):
    """Moeller-Trumbore.  All arguments broadcast on their leading axes."""
    e1, e2 = p1 - p0, p2 - p0
    nn = np.cross(e1, e2)
    twice_area = _norm(nn)
    l0, l1, l2 = _norm(p2 - p1), _norm(e2), _norm(e1)            # the edges opposite p0, p1, p2
    longest = np.maximum(l0, np.maximum(l1, l2))
    flat = twice_area <= 1e-12 * longest * longest               # zero area: never hit
    dl = _norm(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = nn / twice_area[..., None]
        pv = np.cross(d, e2)
        det = _dot(e1, pv)
        tv = o - p0
        b1 = _dot(tv, pv) / det
        qv = np.cross(tv, e1)
        b2 = _dot(d, qv) / det
        t = _dot(e2, qv) / det
        b0 = 1.0 - b1 - b2
        clear = np.minimum(b0 * twice_area / l0, np.minimum(b1 * twice_area / l1, b2 * twice_area / l2))
        dn = np.abs(_dot(d, n)) / dl
    corner = np.maximum(_absmax(p0), np.maximum(_absmax(p1), _absmax(p2)))
    S0 = np.maximum(_absmax(o), corner)
    parallel = ~flat & ~(dn >= PARALLEL)
    # a ray beside the plane, farther from it than delta, misses whatever its direction does
    beside = np.abs(_dot(o - p0, np.where(flat[..., None], 0.0, n))) > DELTA * TOL * S0
    none = flat | parallel | ~np.isfinite(t)
    t = np.where(none, np.inf, t)
    S = np.maximum(S0, np.where(none, 0.0, np.abs(t)))
    bound = _bound(S, dn)
    shape = t.shape
    return dict(t=t, b1=np.where(none, 0.0, b1), b2=np.where(none, 0.0, b2), n=np.broadcast_to(n, shape + (3,)),
                clear=np.where(none, -np.inf, clear), dn=np.broadcast_to(dn, shape), S=S, bound=bound,
                bound_t=bound / dl, delta_clear=DELTA * bound,
                sure_miss=np.broadcast_to(flat, shape) | (parallel & beside),
                unsure=parallel & ~beside, height=np.broadcast_to(twice_area / longest, shape),
                corner_sine=np.broadcast_to(twice_area / (l1 * l2 + (l1 * l2 == 0)), shape))


def sphere_candidates(o, d, c, r, far):
    """The root (near: far = False) of |o + t d - c| = r through the projection of the centre on the ray."""
    dl = _norm(d)
    dh = d / dl[..., None]
    f = c - o
    along = _dot(f, dh)
    m = _norm(f - along[..., None] * dh)                          # closest approach of the line to the centre
    h2 = r * r - m * m
    h = np.sqrt(np.maximum(h2, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(h2 >= 0, (along + h if far else along - h) / dl, np.inf)
        p = o + np.where(np.isfinite(t), t, 0.0)[..., None] * d
        n = (p - c) / r[..., None]
        dn = h / r
    S = np.maximum(np.maximum(_absmax(o), _absmax(c) + r), np.where(np.isfinite(t), np.abs(t), 0.0))
    bound = _bound(S, dn)
    zero = np.zeros(t.shape)
    return dict(t=t, b1=zero, b2=zero, n=n, clear=r - m, dn=dn, S=S, bound=bound, bound_t=bound / dl,
                delta_clear=DELTA * TOL * S,                      # the closest approach needs no quotient
                sure_miss=np.zeros(t.shape, bool), unsure=np.zeros(t.shape, bool), height=zero, corner_sine=zero + 1.0)


def classify(c, t_min, t_max):
    """f64 hit / robust hit / robust miss of candidates against a range (arrays that broadcast with c['t'])."""
    t, clear = c["t"], c["clear"]
    with np.errstate(invalid="ignore"):
        dt = DELTA * c["bound_t"]
        has = np.isfinite(t)
        hit = has & (clear >= 0) & (t >= t_min) & (t <= t_max)
        in_range = (t - t_min > dt) & (t_max - t > dt)
        out_range = (t_min - t > dt) | (t - t_max > dt)
        robust_hit = has & ~c["unsure"] & (clear > c["delta_clear"]) & in_range
        robust_miss = c["sure_miss"] | (~c["unsure"] & ((clear < -c["delta_clear"]) | (has & out_range)))
    return hit, robust_hit, robust_miss


# ------------------------------------------------------------------------------------------ all primitives
def _columns(geo, o, d):
    """Candidates of rays [R] against every column of geo: dict of [R, C] arrays."""
    parts = []
    if len(geo.tri):
        parts.append(tri_candidates(o[:, None, :], d[:, None, :], geo.tri[None, :, 0], geo.tri[None, :, 1], geo.tri[None, :, 2]))
    if len(geo.sph):
        for far in (False, True):
            parts.append(sphere_candidates(o[:, None, :], d[:, None, :], geo.sph[None, :, :3], geo.sph[None, :, 3], far))
    keys = ("t", "clear", "bound", "bound_t", "delta_clear", "sure_miss", "unsure")
    return {k: np.concatenate([np.broadcast_to(p[k], p["t"].shape) for p in parts], axis=1) for k in keys}


def sweep(rays, geo, chunk=2_000_000):
    """Every ray against every primitive.  Per ray:
      t_near, prim_near   the nearest float64 hit in range (inf, -1: none)
      near_robust         that hit is robust
      t_robust, bound_robust, prim_robust   the nearest ROBUST hit and the bound of its t (inf: none)
      any_robust          some robust hit lies in range
      all_miss            every primitive is a robust miss"""
    o, d, t_min, t_max = split_rays(rays)
    n = len(o)
    out = dict(t_near=np.full(n, np.inf), prim_near=np.full(n, -1), near_robust=np.zeros(n, bool),
               t_robust=np.full(n, np.inf), bound_robust=np.zeros(n), prim_robust=np.full(n, -1),
               any_robust=np.zeros(n, bool), all_miss=np.zeros(n, bool))
    ncol = max(len(geo.col_prim), 1)
    step = max(1, chunk // ncol)
    for a in range(0, n, step):
        s = slice(a, a + step)
        c = _columns(geo, o[s], d[s])
        hit, rh, rm = classify(c, t_min[s, None], t_max[s, None])
        rows = np.arange(hit.shape[0])
        tn = np.where(hit, c["t"], np.inf)
        k = tn.argmin(1)
        some = hit[rows, k]
        out["t_near"][s] = tn[rows, k]
        out["prim_near"][s] = np.where(some, geo.col_prim[k], -1)
        out["near_robust"][s] = some & rh[rows, k]
        tr = np.where(rh, c["t"], np.inf)
        k = tr.argmin(1)
        some = rh[rows, k]
        out["t_robust"][s] = tr[rows, k]
        out["bound_robust"][s] = np.where(some, c["bound_t"][rows, k], 0.0)
        out["prim_robust"][s] = np.where(some, geo.col_prim[k], -1)
        out["any_robust"][s] = rh.any(1)
        out["all_miss"][s] = rm.all(1)
    return out


def closest(rays, verts, tris, spheres, tri_prim=None, sph_prim=None):
    """`sweep` from plain arrays: vertices [V, 3], index triples [T, 3], spheres [S, 4]."""
    return sweep(rays, Geometry(verts, tris, spheres, tri_prim, sph_prim))


def occluded(rays, verts, tris, spheres, tri_prim=None, sph_prim=None):
    """(must be occluded, must be free) per ray; where neither holds the model does not say."""
    r = closest(rays, verts, tris, spheres, tri_prim, sph_prim)
    return r["any_robust"], r["all_miss"]


def pairs(rays, geo, prim, t_hint):
    """Ray i against primitive prim[i] alone: the candidate dict, pairwise.  Of a sphere's two roots the one nearer
    to t_hint (the t a backend reported) is taken; whether a nearer one was due is the sweep's business."""
    o, d, _, _ = split_rays(rays)
    prim = np.asarray(prim, np.int64)
    n = len(prim)
    keys = ("t", "b1", "b2", "clear", "dn", "S", "bound", "bound_t", "delta_clear", "unsure", "height", "corner_sine")
    out = {k: np.zeros(n, bool if k == "unsure" else F) for k in keys}
    out["n"] = np.zeros((n, 3))
    out["p"] = np.zeros((n, 3))
    is_tri = geo.kind[prim] == 0
    if is_tri.any():
        T = geo.tri[geo.local[prim[is_tri]]]
        c = tri_candidates(o[is_tri], d[is_tri], T[:, 0], T[:, 1], T[:, 2])
        for k in keys + ("n",):
            out[k][is_tri] = c[k]
    sp = ~is_tri
    if sp.any():
        Sp = geo.sph[geo.local[prim[sp]]]
        near = sphere_candidates(o[sp], d[sp], Sp[:, :3], Sp[:, 3], False)
        far = sphere_candidates(o[sp], d[sp], Sp[:, :3], Sp[:, 3], True)
        hint = np.asarray(t_hint, F)[sp]
        with np.errstate(invalid="ignore"):
            take_far = np.abs(far["t"] - hint) < np.abs(near["t"] - hint)
        for k in keys + ("n",):
            out[k][sp] = np.where(take_far[:, None] if k == "n" else take_far, far[k], near[k])
    out["p"] = o + np.where(np.isfinite(out["t"]), out["t"], 0.0)[:, None] * d
    out["is_tri"] = is_tri
    return out
