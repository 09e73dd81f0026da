"""TEST INFRASTRUCTURE: an independent float64 model of the render-time lookups of the path, written
from the geometry and the published formulas (numpy, vectorised), so that the oracle and the kernels
can be held to something that is neither of them.  Nothing here is a translation of the reference or of
oracle/oracle.cpp: each function states the mathematics and cites the reference lines whose BEHAVIOUR
it models.  Where the reference departs from the textbook the departure is modelled and named (DESIGN.md
§6 quirk list: Q6, Q13, Q19-Q25).

  wrap, bilinear, trilinear      include/texture/texture_common.h:22-53, src/image_texture.cpp:132-189
  rg_lookup                      include/texture/texture_RG.h:32-57
  checker_parity                 include/texture/texture_RGB.h:45-81
  texture_lod                    include/texture/texture_RGB.h:138-149, src/image_texture.cpp:162-172
  dir_to_uv, uv_to_dir, env_*    include/background.h:25-179, include/rng/sampling.h:107-197
  thin_lens_ray, cone_*          src/tl_camera.cpp:6-53, include/ray.h:36-60
  cone_surface_spread, cone_reflect, cone_refract     include/ray.h:52-174 (Q29-Q32)
  shading_frame                  src/geometry/triangle.cpp:13-153, include/hit_utils.h:32-59

The mip chain itself is prestep_ref.mip_chain (pinned against the host library there)."""
import numpy as np

WRAP_CLAMP, WRAP_MIRROR, WRAP_REPEAT = 0, 1, 2
D = np.float64


# ------------------------------------------------------------------------------------------ lookups
def wrap(x, mode):
    """A texture coordinate brought into [0, 1].  clamp: saturate.  repeat: the fractional part.
    mirror as the reference has it (Q20): a positive coordinate is NOT mirrored, it repeats; a negative
    one is reflected only in the periods whose integer part (rounded towards zero) is odd, i.e. on
    (-2, -1), (-4, -3) ...; on (-1, 0), (-3, -2) ... it repeats as well."""
    x = np.asarray(x, dtype=D)
    if mode == WRAP_CLAMP:
        return np.clip(x, 0.0, 1.0)
    rep = x - np.floor(x)
    if mode == WRAP_REPEAT:
        return rep
    k = np.ceil(x)                                   # the integer part of a negative coordinate
    reflected = (x < 0) & (np.mod(k, 2) != 0) & (x != k)
    return np.where(reflected, k - x, rep)


def _texel_pos(t, n):
    """Continuous position t in [0, 1] on an axis of n texels -> (left texel, right texel, weight of the
    right one).  Q19: texel i sits AT i / n, not at (i + 0.5) / n, so the picture a lookup reconstructs is
    the textbook one shifted by half a texel towards larger coordinates; the last texel is held beyond
    (n - 1) / n."""
    p = t * n
    i0 = np.clip(np.floor(p), 0, n - 1).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, p - i0


def bilinear(level, u, v, wrap_u, wrap_v):
    """One level ([h, w, c] array) at arrays of (u, v)."""
    level = np.asarray(level, dtype=D)
    h, w = level.shape[:2]
    x0, x1, fx = _texel_pos(wrap(u, wrap_u), w)
    y0, y1, fy = _texel_pos(wrap(v, wrap_v), h)
    fx, fy = fx[..., None], fy[..., None]
    top = level[y0, x0] * (1 - fx) + level[y0, x1] * fx
    bot = level[y1, x0] * (1 - fx) + level[y1, x1] * fx
    return top * (1 - fy) + bot * fy


def clamp_lod(lam, num_levels):
    """The level a lookup blends at: NaN -> 0, then [0, levels - 1]."""
    lam = np.asarray(lam, dtype=D)
    return np.clip(np.where(np.isnan(lam), 0.0, lam), 0.0, float(num_levels - 1))


def trilinear(chain, lam, u, v, wrap_u, wrap_v):
    """Blend of the two levels around lam (already biased; clamped here) of a chain of [h, w, 3] levels."""
    lam = clamp_lod(lam, len(chain))
    l0 = np.floor(lam).astype(np.int64)
    l1 = np.minimum(l0 + 1, len(chain) - 1)
    f = (lam - l0)[..., None]
    out = np.zeros(lam.shape + (3,), dtype=D)
    for k in range(len(chain)):
        m0, m1 = l0 == k, l1 == k
        if m0.any():
            out[m0] += bilinear(chain[k], u[m0], v[m0], wrap_u, wrap_v) * (1 - f[m0])
        if m1.any():
            out[m1] += bilinear(chain[k], u[m1], v[m1], wrap_u, wrap_v) * f[m1]
    return out


def rg_lookup(rg, u, v, wrap_u, wrap_v):
    """The two-channel map ([h, w, 2]) at (u, v): a bilinear lookup whose two +x neighbours are fetched
    from the row-major storage at `x + y * HEIGHT` instead of `x + y * width` (Q6).  On a square map that is
    the plain lookup; on a wide one (w > h) the +x taps come from another place in the map.  A tall map
    (h > w) would be read past its end, so callers keep w >= h."""
    rg = np.asarray(rg, dtype=D)
    h, w = rg.shape[:2]
    assert w >= h, "Q6 indexes past the end of a map that is taller than wide"
    flat = rg.reshape(h * w, 2)
    x0, x1, fx = _texel_pos(wrap(u, wrap_u), w)
    y0, y1, fy = _texel_pos(wrap(v, wrap_v), h)
    fx, fy = fx[..., None], fy[..., None]
    top = flat[x0 + y0 * w] * (1 - fx) + flat[x1 + y0 * h] * fx
    bot = flat[x0 + y1 * w] * (1 - fx) + flat[x1 + y1 * h] * fx
    return top * (1 - fy) + bot * fy


def checker_parity(u, v, cells_u, cells_v):
    """0 where a checkerboard of cells_u x cells_v cells over the unit square shows its first colour, 1 where
    its second: the cell (floor(u cells_u), floor(v cells_v)) is of the first colour when the sum is even.  No
    wrap mode and no level of detail take part.  (Non-negative uv only: the reference converts the floor to an
    unsigned integer.)"""
    return ((np.floor(np.asarray(u, D) * cells_u) + np.floor(np.asarray(v, D) * cells_v)) % 2).astype(np.int64)


# --------------------------------------------------------------------------------- ray-cone texture LOD
def texture_lod(primitive_area, tex_coord_area, cone_width, abs_d_dot_ng, tex_w, tex_h, num_levels):
    """Ray-cone level of detail at a hit (Akenine-Moeller et al., "Texture level of detail strategies for
    real-time ray tracing", eq. 3-5 of the ray-cone section):

        lambda = 1/2 log2(t_a w h / p_a) + log2(|width| / |d . n_g|)

    with t_a the triangle's area in uv space and p_a its area in world space.  The reference passes TWICE
    the world-space area for p_a and the full parallelogram for t_a's counterpart (Q13: both are the cross
    product's length, so the factor cancels in the ratio), subtracts a bias of 2 levels (Q21), maps NaN to 0
    and clamps to the chain."""
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = 0.5 * np.log2(np.asarray(tex_coord_area, D) / np.asarray(primitive_area, D))
        lam = lam + np.log2(np.abs(np.asarray(cone_width, D)) / np.asarray(abs_d_dot_ng, D))
        lam = lam + 0.5 * np.log2(float(tex_w) * float(tex_h))
    lam = np.where(np.isnan(lam), 0.0, lam) - 2.0
    return clamp_lod(lam, num_levels)


def cone_spread(vfov_deg, res_y):
    """Spread angle of a primary ray's cone: the angle one pixel row subtends at the image centre."""
    return np.arctan(2.0 * np.tan(np.deg2rad(D(vfov_deg)) / 2.0) / res_y)


def cone_width_at(spread, t, width0=0.0):
    """Width of a cone of the given spread after a distance t (small-angle form the reference uses)."""
    return np.abs(spread * np.asarray(t, D) + width0)


# --------------------------------------------------------------------------- ray cones beyond the first hit
def cone_surface_spread(curvature, width, d, n):
    """The angle by which the surface normal turns across the cone's footprint: a cone of width w meets a surface
    seen under cos = -d . n in a footprint w / cos long, and the normal of a surface of mean curvature H turns by H
    per unit of length: beta = H w / cos.  Signed: seen from behind (d . n > 0) the same surface curves the other
    way.  As the reference has it: the width is the cone's width as it stands at the ray's ORIGIN, not grown to the
    hit (Q29), and |cos| < 1e-5 is replaced by 1e-5 with the sign of cos, a cos of exactly 0 counting as negative."""
    cos = -np.sum(np.asarray(d, D) * np.asarray(n, D), -1)
    cos = np.where(np.abs(cos) < 1e-5, np.where(cos > 0, 1e-5, -1e-5), cos)
    return np.asarray(curvature, D) * np.asarray(width, D) / cos


def cone_reflect(width, spread, t, beta):
    """The cone after travelling t and reflecting: it has grown to |w + spread t| (small-angle form), and a mirror whose
    normal turns by beta across the footprint turns the two boundary rays apart by 2 beta."""
    return np.abs(np.asarray(width, D) + np.asarray(spread, D) * np.asarray(t, D)), np.asarray(spread, D) + 2.0 * np.asarray(beta, D)


def _wrap_angle(a):
    return (a + np.pi) % (2.0 * np.pi) - np.pi


def cone_refract(width, spread, beta, eta, d, wo, details=False):
    """The cone after refraction, from the ray-cone construction in the plane of incidence, by angles (all angles
    counter-clockwise from the x axis; the surface is the line y = 0, its normal +y, x along the tangential part of d):

      - the two boundary rays of the incoming cone start w / 2 to either side of the axis and run at -+ spread / 2 to
        it until they meet the surface, at x_u and x_l;
      - there the normal is tilted by -+ beta / 2 (away from each other on a convex surface);
      - each boundary ray is refracted by Snell's law about its own normal, sin(theta_t) = eta sin(theta_i); a
        boundary ray beyond the critical angle runs on along the (tilted) surface, theta_t = +-90 degrees;
      - the new spread is the signed angle between the two refracted rays, the new width their separation measured
        across the refracted axis wo, where they cross the line through the origin perpendicular to it.

    As the reference has it: the plane's normal is -(eta wo + d) normalised (Q30: for the wo and eta its materials
    pass that is not the surface normal, which is along d - wo / eta'), eta is used as passed (Q31: the materials pass
    n_t / n_i, Snell's law in this form wants n_i / n_t), the width is taken as it stands, without spread * t (Q32),
    the boundary rays are labelled by the sign of the width (a width of 0 counting as negative) and the tilt by which
    of them meets the surface further along x."""
    width, spread, beta, eta = (np.asarray(a, D) for a in (width, spread, beta, eta))
    d, wo = np.asarray(d, D), np.asarray(wo, D)
    m = eta[..., None] * wo + d
    N = -m / np.linalg.norm(m, axis=-1, keepdims=True)
    tang = d - N * np.sum(N * d, -1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        X = tang / np.linalg.norm(tang, axis=-1, keepdims=True)         # 0 / 0 for eta = 1, where wo = d (Q30)
    phi_i = np.arctan2(np.sum(d * N, -1), np.sum(d * X, -1))
    phi_o = np.arctan2(np.sum(wo * N, -1), np.sum(wo * X, -1))
    s = np.where(width > 0, 1.0, -1.0)
    phi_u, phi_l = phi_i + spread * s * 0.5, phi_i - spread * s * 0.5
    # the boundary rays' starting points, w / 2 to the left of the axis (u) and to its right (l)
    sx, sy = -np.sin(phi_i) * width * 0.5, np.cos(phi_i) * width * 0.5
    with np.errstate(divide="ignore", invalid="ignore"):
        x_u = sx - sy / np.tan(phi_u)
        x_l = -sx + sy / np.tan(phi_l)
    sign = np.where(x_u > x_l, 1.0, -1.0)
    tilt = -beta * sign * 0.5
    out, tir = [], []
    for phi, psi in ((phi_u, np.pi / 2 + tilt), (phi_l, np.pi / 2 - tilt)):
        theta_i = _wrap_angle(phi - (psi + np.pi))             # from the inward normal to the ray
        sin_t = eta * np.sin(theta_i)
        tir.append(np.abs(sin_t) > 1.0)
        out.append(psi + np.pi + np.arcsin(np.clip(sin_t, -1.0, 1.0)))
    new_spread = sign * _wrap_angle(out[0] - out[1])
    with np.errstate(divide="ignore", invalid="ignore"):
        lam_u = -x_u * np.sin(out[0]) / np.cos(out[0] - phi_o)
        lam_l = -x_l * np.sin(out[1]) / np.cos(out[1] - phi_o)
    new_width = lam_u - lam_l
    if details:
        return new_width, new_spread, dict(tir_u=tir[0], tir_l=tir[1], phi_i=phi_i, phi_o=phi_o, x_u=x_u, x_l=x_l,
                                           out_u=out[0], out_l=out[1], normal=N,
                                           tangential=np.linalg.norm(tang, axis=-1))
    return new_width, new_spread


# ------------------------------------------------------------------------------------------- env map
def _rot(m16, d):
    """Direction through a column-major 4x4 (w = 0), normalised."""
    m = np.asarray(m16, dtype=D).reshape(4, 4).T[:3, :3]
    r = np.asarray(d, dtype=D) @ m.T
    return r / np.linalg.norm(r, axis=-1, keepdims=True)


def dir_to_uv(d, world_to_env=None):
    """Equirectangular coordinates of a world direction: v = polar angle from +y over pi, u = azimuth over
    2 pi, with u = 0.5 towards +z and u growing towards -x."""
    e = _rot(world_to_env, d) if world_to_env is not None else np.asarray(d, D) / np.linalg.norm(d, axis=-1, keepdims=True)
    u = 0.5 * (1.0 + np.arctan2(-e[..., 0], e[..., 2]) / np.pi)
    v = np.arccos(np.clip(e[..., 1], -1.0, 1.0)) / np.pi
    return u, v


def uv_to_dir(u, v, env_to_world=None):
    """The inverse map: the world direction of equirectangular (u, v)."""
    az, el = 2.0 * np.pi * np.asarray(u, D), np.pi * np.asarray(v, D)
    e = np.stack([np.sin(az) * np.sin(el), np.cos(el), -np.cos(az) * np.sin(el)], -1)
    return _rot(env_to_world, e) if env_to_world is not None else e


def env_texel(u, v, w, h):
    """The texel (row, column) whose sampling cell holds (u, v): cells are [i / n, (i + 1) / n)."""
    col = np.clip(np.floor(np.asarray(u, D) * w), 0, w - 1).astype(np.int64)
    row = np.clip(np.floor(np.asarray(v, D) * h), 0, h - 1).astype(np.int64)
    return row, col


def env_texel_prob(row_cdf, col_cdfs):
    """Probability of each texel cell from the two CDF tables ([h + 1], [h, w + 1]) -> [h, w]."""
    r = np.diff(np.asarray(row_cdf, D))
    c = np.diff(np.asarray(col_cdfs, D), axis=1)
    return r[:, None] * c


def env_texel_prob_ideal(img):
    """What the tables encode: luminance times the sine of the cell centre's polar angle, normalised."""
    img = np.asarray(img, D)
    h = img.shape[0]
    lum = img @ np.array([0.212671, 0.715160, 0.072169])
    wgt = np.abs(lum) * np.sin(np.pi * (np.arange(h) + 0.5) / h)[:, None]
    tot = wgt.sum()
    return wgt / tot if tot > 0 else np.full(wgt.shape, 1.0 / wgt.size)


def env_pdf(prob, d, world_to_env=None):
    """Solid-angle density of the direction d: the cell's probability over the cell's solid angle measured
    AT d, (2 pi / w)(pi / h) sin(theta_d) (Q22: not the cell's exact solid angle, so the density varies with
    1 / sin(theta) inside a cell and still integrates to one)."""
    h, w = prob.shape
    u, v = dir_to_uv(d, world_to_env)
    row, col = env_texel(u, v, w, h)
    with np.errstate(divide="ignore"):
        return prob[row, col] * w * h / (2.0 * np.pi ** 2 * np.sin(np.pi * v))


def env_radiance(chain, d, world_to_env, scale, wrap_u, wrap_v, lam=0.0):
    """L(omega): the radiance a ray leaving along d with a zero cone picks up - level 0 of the env texture,
    reconstructed with the half-texel convention of `bilinear` (Q19), times the radiance scale."""
    u, v = dir_to_uv(d, world_to_env)
    return trilinear(chain, np.full(u.shape, lam, D), u, v, wrap_u, wrap_v) * scale


def env_radiance_uv(level0, u, v, scale, wrap_u, wrap_v):
    return bilinear(level0, u, v, wrap_u, wrap_v) * scale


# -------------------------------------------------------------------------------------------- camera
def pinhole_dir_cam(x, y, vfov_deg, res):
    """Camera-space direction (looking down -z, +y up... as the film is addressed) through film point (x, y)
    in pixels: the film plane at distance 1 is 2 tan(vfov / 2) high."""
    hgt = 2.0 * np.tan(np.deg2rad(D(vfov_deg)) / 2.0)
    wid = hgt * res[0] / res[1]
    d = np.stack([wid * (np.asarray(x, D) / res[0] - 0.5), hgt * (np.asarray(y, D) / res[1] - 0.5),
                  -np.ones_like(np.asarray(x, D))], -1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def thin_lens_ray(cam_to_world, vfov_deg, res, aperture_radius, focal_dist, x, y, rand1, rand2):
    """Thin-lens camera ray: the lens is the disc of radius R in the camera's z = 0 plane, sampled uniformly
    in area (r = R sqrt(rand1), phi = 2 pi rand2); every ray of a film point passes through the point where
    that film point's pinhole ray meets the plane of focus z = -focal.  Returns world (origin, direction)."""
    m = np.asarray(cam_to_world, dtype=D).reshape(4, 4).T
    dc = pinhole_dir_cam(x, y, vfov_deg, res)
    oc = np.zeros_like(dc)
    if aperture_radius > 0:
        r, phi = aperture_radius * np.sqrt(np.asarray(rand1, D)), 2.0 * np.pi * np.asarray(rand2, D)
        oc = np.stack([r * np.cos(phi), r * np.sin(phi), np.zeros_like(r)], -1)
        focus = dc * (focal_dist / np.abs(dc[..., 2:3]))
        dc = focus - oc
        dc = dc / np.linalg.norm(dc, axis=-1, keepdims=True)
    o = oc @ m[:3, :3].T + m[:3, 3]
    d = dc @ m[:3, :3].T
    return o, d / np.linalg.norm(d, axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------- shading frame
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def branchless_onb(n):
    """Frisvad's orthonormal basis around unit n (the form without the sqrt; include/hit_utils.h:43-59)."""
    n = np.asarray(n, D)
    a = 1.0 / (1.0 + n[..., 2])
    b = -n[..., 0] * n[..., 1] * a
    t = np.stack([1.0 - n[..., 0] ** 2 * a, b, -n[..., 0]], -1)
    s = np.stack([b, 1.0 - n[..., 1] ** 2 * a, -n[..., 1]], -1)
    return t, s


def shading_frame(n_interp, dpdu, normal_texel=None):
    """(n_s, tangent, bitangent) at a hit with interpolated unit normal n_interp and surface derivative dpdu.
    With a normal map, the texel is read AS STORED - normalised, no 2 t - 1 decode - and taken as coordinates
    in Frisvad's basis around n_interp, not in the uv-aligned tangent frame (Q23); the tangent is then dpdu
    made orthogonal to the new normal, the bitangent completes a right-handed frame."""
    n = _unit(np.asarray(n_interp, D))
    if normal_texel is not None:
        c = _unit(np.asarray(normal_texel, D))
        t, s = branchless_onb(n)
        n = t * c[..., 0:1] + s * c[..., 1:2] + n * c[..., 2:3]
    dpdu = np.asarray(dpdu, D)
    tangent = _unit(dpdu - n * np.sum(n * dpdu, -1, keepdims=True))
    return n, tangent, np.cross(n, tangent)
