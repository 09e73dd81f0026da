"""Known answers for what every path vertex evaluates: the Principled lobes, the Lambertian, the smooth
dielectric and the light samplers, against tests/shading_ref.py - a float64 model written from the publications, not
from the oracle.  Every check runs on the CPU oracle and, marked gpu, on the GPU with the same bound (the Backend of
tests/test_path_known_answers.py: at most 65 536 items per GPU test).

Bounds come from the model: 32 ulp of the largest operand where the expression is well conditioned, and the
condition-number terms shading_ref derives where it is not.  Statistics: 5 sigma of their own counts.  Where the
oracle cannot meet a derived bound, the case's bound is 4 x the oracle's measured worst error in units of the derived
bound (LOBE_MEASURED, beside the assertion and in DESIGN.md §6); it is measured on the oracle and the GPU must meet
the same figure."""
import numpy as np
import pytest

import oracle_lib as O
import path_ref as PR
import shading_ref as S
import vimg_amd
from vimg_amd import abi
from test_path_known_answers import BACKENDS, Backend, EPS, TOL

_unit = S.unit


# =============================================================================== carriers
# Every mesh uv lies in [2, 3]: under WRAP_CLAMP a 1 x 1 map is then read with an interpolation weight of exactly 1, so
# the lookup returns the texel's bits.  Inside (0, 1) it does not (Q33): c (1 - a) + c a rounds.  The analytic sphere
# makes its own uvs in [0, 1], so on it the textured build is held to the model but not to the baked build's bits.
UV_SHIFT = 2.0


def _rot(ax_deg, ay_deg):
    ax, ay = np.deg2rad(ax_deg), np.deg2rad(ay_deg)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    return ry @ rx


def _quad_mesh(rot, centre, half=2.0):
    """Two triangles, uv over [0, 1]^2, geometric normal rot @ +z."""
    v = np.array([[-half, -half, 0], [half, -half, 0], [half, half, 0], [-half, half, 0]], np.float64) @ rot.T + np.asarray(centre)
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32) + UV_SHIFT
    return v.astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.uint32), uv, None


def _sphere_mesh(n_lat, centre, radius=1.0):
    """n_lat x 2 n_lat tessellated sphere with vertex normals, uv = (phi / 2 pi, theta / pi), every triangle wound so
    that its geometric normal points outwards; the degenerate triangles at the poles are left out."""
    th = np.linspace(0, np.pi, n_lat + 1)
    ph = np.linspace(0, 2 * np.pi, 2 * n_lat + 1)
    T, Ph = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(Ph), np.cos(T), np.sin(T) * np.sin(Ph)], -1).reshape(-1, 3)
    uv = np.stack([Ph / (2 * np.pi), T / np.pi], -1).reshape(-1, 2)
    nl = 2 * n_lat
    idx = []
    for i in range(n_lat):
        for j in range(nl):
            a, b, c, e = i * (nl + 1) + j, i * (nl + 1) + j + 1, (i + 1) * (nl + 1) + j, (i + 1) * (nl + 1) + j + 1
            if i > 0:
                idx.append([a, c, b])
            if i < n_lat - 1:
                idx.append([b, c, e])
    idx = np.asarray(idx, np.uint32)
    v = (d * radius + np.asarray(centre)).astype(np.float32)
    p = v.astype(np.float64)[idx.astype(np.int64)]
    out = np.sum(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) * (p.mean(1) - np.asarray(centre)), -1)
    idx[out < 0] = idx[out < 0][:, [0, 2, 1]]
    return v, idx, (uv + UV_SHIFT).astype(np.float32), d.astype(np.float32)


# The two spheres stand near the origin: their normals come from hit positions, whose float32 rounding grows with the
# coordinates, and the model's bound is for operands of size one.  The quads' normals do not depend on where they stand.
CARRIER_AT = {"quad": (6.0, 0.0, 0.0), "tilted": (-7.0, 1.0, -2.0), "sphere": (0.0, 0.0, 0.0), "facets": (0.0, 3.0, 0.0)}
TILT = _rot(37.0, 23.0)
_meshes = {"quad": _quad_mesh(np.eye(3), CARRIER_AT["quad"]), "tilted": _quad_mesh(TILT, CARRIER_AT["tilted"]),
           "facets": _sphere_mesh(16, CARRIER_AT["facets"])}
BASE = (0.7, 0.6, 0.5)


def _material_scene(kind, params, base, textured):
    """The four carriers under ONE material.  textured: the colour in a 1 x 1 image and metallic / roughness in a 1 x 1
    RG map with unit factors (the stage computes the terms); else a constant colour and the factors (baked record)."""
    s = vimg_amd.HostScene()
    s.set_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, (8, 8))
    p = dict(params)
    if textured:
        tex = s.add_texture_image(np.float32(base).reshape(1, 1, 3), abi.WRAP_CLAMP, abi.WRAP_CLAMP)
    else:
        tex = s.add_texture_const(base)
    if kind == "principled" and textured:
        rg = np.float32([[[p.pop("metallic", 0.0), p.pop("roughness", 0.5)]]])
        m = s.add_material(kind, tex=tex, mr_tex=s.add_texture_rg(rg, abi.WRAP_CLAMP, abi.WRAP_CLAMP), metallic=1.0, roughness=1.0, **p)
    else:
        m = s.add_material(kind, tex=tex, **p)
    for name in ("quad", "tilted", "facets"):
        v, idx, uv, nrm = _meshes[name]
        s.add_mesh(v, idx, m, normals=nrm, uv_sets=[uv], color_uv=0, mr_uv=0)
    s.add_sphere(CARRIER_AT["sphere"], 1.0, m)
    s.set_background_const((0.5, 0.5, 0.5), add_to_lights=True)
    s.build_bvh(abi.BVH_SWEEP)
    return s


def _perp(n, rng):
    w = rng.normal(size=n.shape)
    return _unit(w - n * S.dot(w, n)[..., None])


def _tri_frame(mesh, tri, o, d):
    """Where the float32 ray (o, d) meets the plane of triangle `tri` of the mesh, in float64: the point, its
    barycentrics (u, v, w: q = u p0 + v p1 + w p2), the geometric normal, the interpolated shading normal and the frame
    (tangent along dp/du of the colour uvs made orthogonal to n_s, bitangent n_s x tangent)."""
    v, idx, uv, nrm = mesh
    vi = idx.astype(np.int64)[tri]
    p = v.astype(np.float64)[vi]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    nn = np.cross(e1, e2)
    n_g = _unit(nn)
    t = S.dot(p[:, 0] - o, n_g) / S.dot(d, n_g)
    q = o + d * t[:, None]
    rel = q - p[:, 0]
    den = S.dot(nn, nn)
    b1 = S.dot(np.cross(rel, e2), nn) / den
    b2 = S.dot(np.cross(e1, rel), nn) / den
    bary = np.stack([1 - b1 - b2, b1, b2], -1)
    n_s = n_g if nrm is None else _unit(np.einsum("nk,nkc->nc", bary, nrm.astype(np.float64)[vi]))
    tuv = uv.astype(np.float64)[vi]
    duv = np.stack([tuv[:, 1] - tuv[:, 0], tuv[:, 2] - tuv[:, 0]], 1)
    dpdu = np.linalg.solve(duv, np.stack([e1, e2], 1))[:, 0]
    n_s, tangent, bitangent = PR.shading_frame(n_s, dpdu)
    return dict(q=q, t=t, bary=bary, n_g=n_g, n_s=n_s, frame=(tangent, bitangent, n_s))


COS_I = (0.02, 0.1, 0.3, 0.6, 0.84, 1.0)


def _incidences(carrier, per, rng, cos_list=COS_I):
    """Float32 rays onto the carrier at the listed cosines against the geometric normal, from above and from below
    it, `per` rays each, and the float64 geometry of each ray's hit from the geometry alone.  On the faceted sphere
    the hits lie 0.03 .. 0.1 (in barycentrics) from a facet edge, where the interpolated normal leans furthest."""
    n = len(cos_list) * 2 * per
    cos = np.repeat(np.asarray(cos_list, np.float64), 2 * per)
    below = np.tile(np.repeat([False, True], per), len(cos_list))
    if carrier == "sphere":
        c = np.asarray(CARRIER_AT["sphere"], np.float64)
        n_out = _unit(rng.normal(size=(n, 3)))
        q = c + n_out
        tri = None
    else:
        mesh = _meshes[carrier]
        tri = rng.integers(0, len(mesh[1]), n)
        if carrier == "facets":                         # away from the poles, where the facets become slivers
            ok = np.nonzero(np.abs(mesh[2][mesh[1][:, 0], 1] - UV_SHIFT - 0.5) < 0.35)[0]
            tri = ok[rng.integers(0, len(ok), n)]
            small = rng.uniform(0.03, 0.1, n)
            other = rng.uniform(0.1, 0.8, n)
            bary = np.stack([small, other, 1 - small - other], -1)
            bary = np.take_along_axis(bary, np.argsort(rng.random((n, 3)), 1), 1)
        else:
            bary = rng.dirichlet([2, 2, 2], n) * 0.8 + 0.2 / 3
        p = mesh[0].astype(np.float64)[mesh[1].astype(np.int64)[tri]]
        q = np.einsum("nk,nkc->nc", bary, p)
        n_out = _unit(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]))
    w = _perp(n_out, rng)
    sin = np.sqrt(1 - cos * cos)
    # from above: towards the surface against n_out; from below: leaving through it
    d = np.where(below[:, None], cos[:, None] * n_out + sin[:, None] * w, -(cos[:, None] * n_out + sin[:, None] * w))
    back = np.where(below & (carrier == "sphere"), 0.9 * cos, 1.0)      # inside the unit sphere: the chord is 2 cos
    if carrier == "facets":
        # inside the inscribed mesh a grazing ray has little room: the longest of 0.9 cos 2^-j that starts below every
        # facet's plane by 2e-5 (the origin's float32 rounding is 5e-7)
        pl = mesh[0].astype(np.float64)[mesh[1].astype(np.int64)]
        pn = _unit(np.cross(pl[:, 1] - pl[:, 0], pl[:, 2] - pl[:, 0]))
        found = ~below
        for j in range(10):
            cand = 0.9 * cos * 2.0 ** -j
            o_c = q - d * cand[:, None]
            inside = ((o_c[:, None, :] - pl[None, :, 0, :]) * pn[None]).sum(-1).max(1) < -2e-5
            back = np.where(below & ~found & inside, cand, back)
            found |= inside
        assert found.all()
    o = (q - d * back[:, None]).astype(np.float32)
    d = _unit(d).astype(np.float32)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    if carrier == "sphere":
        oc = o64 - c
        bq = S.dot(oc, d64)
        disc = np.sqrt(bq * bq - S.dot(d64, d64) * (S.dot(oc, oc) - 1.0))
        t = np.where(below, -bq + disc, -bq - disc) / S.dot(d64, d64)
        hit = o64 + d64 * t[:, None]
        n_s = _unit(hit - c)
        tg, bt = PR.branchless_onb(n_s)                # any frame: only isotropic materials go on this carrier
        geo = dict(q=hit, n_g=n_s, n_s=n_s, frame=(tg, bt, n_s))
    else:
        geo = _tri_frame(mesh, tri, o64, d64)
        assert geo["bary"].min() > 0.01
    # the input error of the lobes: on a curved carrier the normal follows the hit point, which float32 places along
    # the ray to (largest operand) / |d . n| (the bound of t in the geometry tests)
    geo["eps_in"] = np.full(n, S.EPS_IN)
    if carrier in ("sphere", "facets"):
        geo["eps_in"] = S.EPS_IN * np.maximum(1.0, np.abs(o64).max(1)) / np.abs(S.dot(d64, geo["n_g"]))
    return np.concatenate([o, d], 1), geo, below


def _wo_set(geo, d, eta, k, rng):
    """k outgoing directions per ray: uniform over the sphere, and clusters within 0.05 and 0.005 of the mirror
    direction and of the direction Snell's law gives at the shading normal for eta (or 1 / eta from below)."""
    n = len(d)
    n_s = geo["n_s"]
    cos = -S.dot(d, n_s)
    mirror = d + 2 * cos[:, None] * n_s
    e = np.where(-S.dot(d, geo["n_g"]) >= 0, eta, 1.0 / eta)
    nn = np.where((cos >= 0)[:, None], n_s, -n_s)
    ci = np.abs(cos)
    kk = 1.0 / e
    s2 = kk * kk * (1 - ci * ci)
    snell = kk[:, None] * d + (kk * ci - np.sqrt(np.maximum(1 - s2, 0)))[:, None] * nn
    snell = np.where((s2 > 1)[:, None], mirror, snell)
    wo = _unit(rng.normal(size=(n, k, 3)))
    part = k // 8
    for j, (centre, r) in enumerate(((mirror, 0.05), (mirror, 0.005), (snell, 0.05), (snell, 0.005))):
        sl = slice(k // 2 + j * part, k // 2 + (j + 1) * part)
        # 0.3 r .. r from the centre ACROSS it: never inside the 1e-3 where the half-vector has no direction
        off = rng.normal(size=(n, part, 3))
        off = _unit(off - centre[:, None, :] * S.dot(off, centre[:, None, :])[..., None])
        wo[:, sl] = _unit(centre[:, None, :] + r * off * rng.uniform(0.3, 1.0, (n, part, 1)))
    return wo.astype(np.float32)


# =============================================================================== materials
# name: (parameters, base colour, carriers).  Anisotropic materials need a tangent the model knows: the quads and
# the faceted sphere.  Together the list reaches every branch of shading_ref.principled.
ALL, MESHES = ("quad", "tilted", "sphere", "facets"), ("tilted", "facets")
MATERIALS = {
    "diffuse": (dict(roughness=0.3, specular=0.0), BASE, ALL),
    "diffuse-r0": (dict(roughness=0.0, specular=0.5, subsurface=0.5), BASE, ALL),        # below the clamp: Q14
    "subsurface": (dict(roughness=1.0, specular=0.0, subsurface=1.0), BASE, ALL),
    "sheen": (dict(roughness=0.3, specular=0.0, sheen=1.0, sheen_tint=1.0), (0.9, 0.05, 0.02), ALL),
    "sheen-untinted-black": (dict(roughness=0.3, sheen=1.0, sheen_tint=0.0, spec_tint=1.0), (0.0, 0.0, 0.0), ALL),
    "metal": (dict(metallic=1.0, roughness=0.3), BASE, ALL),
    "metal-r0": (dict(metallic=1.0, roughness=0.0), BASE, ALL),
    "metal-r0.01-aniso1": (dict(metallic=1.0, roughness=0.01, anisotropic=1.0), BASE, MESHES),
    "metal-aniso0.5": (dict(metallic=0.3, roughness=0.3, anisotropic=0.5, spec_tint=1.0, specular=1.0), (0.9, 0.05, 0.02), MESHES),
    "clearcoat-gloss0": (dict(metallic=0.0, roughness=1.0, specular=0.0, clearcoat=1.0, clearcoat_gloss=0.0), BASE, ALL),
    "clearcoat-gloss0.5": (dict(metallic=0.3, roughness=0.3, clearcoat=1.0, clearcoat_gloss=0.5), BASE, ALL),
    "clearcoat-gloss1": (dict(metallic=0.3, roughness=0.3, clearcoat=0.5, clearcoat_gloss=1.0), BASE, ALL),
    "glass-eta1.5": (dict(spec_trans=1.0, roughness=0.3, eta=1.5), BASE, ALL),
    "glass-eta2.4-aniso": (dict(spec_trans=1.0, roughness=0.3, eta=2.4, anisotropic=0.5), (0.9, 0.05, 0.02), MESHES),
    "glass-eta1.33-half": (dict(spec_trans=0.5, roughness=0.3, eta=1.33, metallic=0.3, sheen=0.5, clearcoat=0.3), BASE, ALL),
    "glass-eta1": (dict(spec_trans=1.0, roughness=0.3, eta=1.0), BASE, ALL),
    "glass-r0.01": (dict(spec_trans=0.5, roughness=0.01, eta=1.5), BASE, ALL),
    "mix-alpha-below-0.1": (dict(metallic=0.3, roughness=0.25, subsurface=0.4, sheen=0.7, spec_tint=0.4, clearcoat=0.6,
                                 clearcoat_gloss=0.5, spec_trans=0.3, eta=1.5), BASE, ALL),
    "mix-alpha-above-0.1": (dict(metallic=0.3, roughness=0.5, subsurface=0.4, sheen=0.7, spec_tint=0.4, clearcoat=0.6,
                                 clearcoat_gloss=0.0, spec_trans=0.3, eta=1.5), BASE, ALL),
}
# Where the oracle misses the derived bound: its worst error on the CPU in units of that bound, per (material,
# quantity); the assertion is 4 x the figure.  Measured on the oracle only.
LOBE_MEASURED = {}

_scene_cache = {}


def _scenes(name):
    if name not in _scene_cache:
        params, base, _ = MATERIALS[name]
        _scene_cache[name] = tuple(_material_scene("principled", params, base, textured) for textured in (False, True))
    return _scene_cache[name]


def _worst(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("regularize", [0, 1])
@pytest.mark.parametrize("name", list(MATERIALS))
def test_principled_eval_is_the_models(name, regularize, backend):
    """BSDF_EVAL on every carrier of the material: f and pdf within the model's bound on every item that has an answer
    (at most 1 % have none, by the model's own rule), no NaN or Inf anywhere else, exact zeros where the side tests say
    so, and the baked build (constant colour, factors) and the computed one (1 x 1 image, 1 x 1 RG map) bit for bit
    the same on the mesh carriers (Q33 on the analytic sphere).
    Measured on the oracle, worst error / bound over the 19 materials and both flags (quad / turned quad / sphere /
    facets): f 0.23 / 0.42 / 0.25 / 0.23, pdf 0.25 / 0.42 / 0.30 / 0.26; left out at most 0.0005 of a case; the GPU gives
    the same figures.  LOBE_MEASURED is empty: no case needs it."""
    params, base, carriers = MATERIALS[name]
    baked, computed = _scenes(name)
    B, B2 = Backend(baked, backend), Backend(computed, backend)
    rng = np.random.default_rng(sum(map(ord, name)) + 1000 * regularize)
    k, per = 32, 10                  # 4 carriers x 12 incidences x 10 rays x 32 directions = 15 360 items per build
    for carrier in carriers:
        rays, geo, below = _incidences(carrier, per, rng)
        n = len(rays)
        wo = _wo_set(geo, rays[:, 3:6].astype(np.float64), np.float64(np.float32(params.get("eta", 1.5))), k, rng)
        x = np.concatenate([np.repeat(rays, k, 0), wo.reshape(-1, 3), np.zeros((n * k, 2), np.float32),
                            np.full((n * k, 1), regularize, np.float32)], 1)
        got = B.probe(O.PROBE_BSDF_EVAL, x)
        got2 = B2.probe(O.PROBE_BSDF_EVAL, x)
        if carrier != "sphere":
            assert np.array_equal(got.view(np.uint32), got2.view(np.uint32)), (name, carrier)
        assert np.all(got[:, 0] == 1) and np.all(got2[:, 0] == 1), (name, carrier)
        rep = lambda a: np.repeat(a, k, 0)
        m = S.principled(rep(-rays[:, 3:6].astype(np.float64)), wo.reshape(-1, 3).astype(np.float64),
                         tuple(rep(a) for a in geo["frame"]), rep(geo["n_g"]), np.float64(np.float32(base)), params,
                         regularize=bool(regularize), eps_in=rep(geo["eps_in"]))
        keep = ~m["undecided"]
        assert 1 - keep.mean() <= 0.01, (name, carrier, 1 - keep.mean())
        flipped = S.dot(geo["n_s"], -rays[:, 3:6]) * S.dot(geo["n_g"], -rays[:, 3:6]) < 0
        for build, g in (("baked", got), ("computed", got2)):       # the same bits but on the sphere: both meet the model
            f, pdf = g[:, 1:4].astype(np.float64), g[:, 4].astype(np.float64)
            assert np.all(np.isfinite(f[keep])) and np.all(np.isfinite(pdf[keep])), (name, carrier, build)
            e_f = _worst(np.abs(f - m["f"]).max(-1)[keep], m["f_bound"][keep])
            e_p = _worst(np.abs(pdf - m["pdf"])[keep], m["pdf_bound"][keep])
            if build == "baked":
                print(f"{name} reg {regularize} {carrier} {backend}: f error / bound {e_f:.3f}, pdf {e_p:.3f}; left out "
                      f"{1 - keep.mean():.4f}; frame turned on {int(flipped.sum())} of {n} rays; largest f {np.abs(m['f']).max():.3g}")
            assert np.all(f[m["zero_f"]] == 0) and np.all(pdf[m["zero_pdf"]] == 0), (name, carrier, build)
            assert e_f <= 4 * LOBE_MEASURED.get((name, "f"), 0.25), (name, carrier, build, e_f)
            assert e_p <= 4 * LOBE_MEASURED.get((name, "pdf"), 0.25), (name, carrier, build, e_p)
        if carrier == "facets":
            assert flipped.sum() > 0 and np.abs(S.dot(geo["n_s"], geo["n_g"]) - 1).max() > 1e-3


@pytest.mark.parametrize("backend", BACKENDS)
def test_lambertian_eval_is_the_models(backend):
    """The Lambertian on the four carriers, from either side: f = albedo max(0, n_s . wo) / pi against the UNTURNED
    shading normal, pdf the same without the albedo; the baked colour and the 1 x 1 image give the same bits."""
    baked, computed = (_material_scene("lambertian", {}, BASE, t) for t in (False, True))
    B, B2 = Backend(baked, backend), Backend(computed, backend)
    rng = np.random.default_rng(5)
    k = 32
    for carrier in ALL:
        rays, geo, below = _incidences(carrier, 10, rng)
        n = len(rays)
        wo = _wo_set(geo, rays[:, 3:6].astype(np.float64), np.float64(1.5), k, rng).reshape(-1, 3)
        x = np.concatenate([np.repeat(rays, k, 0), wo, np.zeros((n * k, 3), np.float32)], 1)
        got, got2 = B.probe(O.PROBE_BSDF_EVAL, x), B2.probe(O.PROBE_BSDF_EVAL, x)
        if carrier != "sphere":
            assert np.array_equal(got.view(np.uint32), got2.view(np.uint32)), carrier
        m = S.lambertian(wo.astype(np.float64), np.repeat(geo["n_s"], k, 0), np.float64(np.float32(BASE)))
        scale = np.repeat(geo["eps_in"], k) / S.EPS_IN             # the carrier's own conditioning of n_s
        for g in (got, got2):
            assert np.all(g[:, 0] == 1)
            e_f = _worst(np.abs(g[:, 1:4] - m["f"]).max(-1), m["f_bound"] * scale)
            e_p = _worst(np.abs(g[:, 4] - m["pdf"]), m["pdf_bound"] * scale)
            assert e_f <= 1 and e_p <= 1, (carrier, e_f, e_p)
        print(f"lambertian {carrier} {backend}: f error / bound {e_f:.3f}, pdf {e_p:.3f}")
        assert (m["pdf"] == 0).mean() > 0.2 and (m["pdf"] > 0).mean() > 0.2


# =============================================================================== BSDF_SAMPLE
SAMPLED = {   # five materials for the histograms, roughness >= 0.3 so that the quadrature converges on a modest grid
    "plastic": dict(metallic=0.0, roughness=0.6, specular=0.5, subsurface=0.3, sheen=0.7),
    "metal": dict(metallic=1.0, roughness=0.45),
    "clearcoat": dict(metallic=0.0, roughness=0.7, clearcoat=1.0, clearcoat_gloss=0.2),
    "glass": dict(spec_trans=1.0, roughness=0.5, eta=1.5),
    "mix": dict(metallic=0.3, roughness=0.5, subsurface=0.4, sheen=0.7, clearcoat=0.6, clearcoat_gloss=0.0, spec_trans=0.3,
                eta=1.5),
}
_FLAT_FRAME = (np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]))


def _cell_integrals(fn, nz=6, nphi=12):
    """Integral of fn(directions) over each of nz x nphi equal-solid-angle cells of the sphere about +z (midpoint
    rule, sub x sub points per cell, doubled until the sum of the cells' changes is below 1e-4 of the total);
    returns (cell integrals, each cell's last change: the stated error)."""
    prev, sub = None, 8
    while True:
        dirs, wgt = S.sphere_grid(nz * sub, nphi * sub)
        val = fn(dirs).reshape(nz, sub, nphi, sub).sum(axis=(1, 3)).reshape(-1) * wgt
        if prev is not None:
            change = np.abs(val - prev)
            if change.sum() <= 1e-4 * val.sum() or sub >= 64:
                return val, change
        prev, sub = val, sub * 2


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name,below", [(k, False) for k in SAMPLED] + [("glass", True), ("mix", True)])
def test_principled_samples_follow_the_models_pdf(name, below, backend):
    """BSDF_SAMPLE on the flat quad at one incidence (cos 0.84; from below only the glass lobe exists): every wo a
    unit vector on the side its eta says, the model's pdf positive there, the specular flag as the lobes set it, the
    6 x 12 cells filled as the MODEL's pdf integrates over them (5 sigma + the quadrature's stated error; the phantom
    density of Q18 masked), and the refused share 1 - the integral.
    Measured on the oracle (200 000 samples): worst cell 0.61 of its allowance, refused share - (1 - integral) at most
    5.2e-4 against an allowance of 2.6e-3, unflagged shares 0.5000 / 0.4446 / 0.2983 for 0.5 / 0.4444 / 0.2988; on the GPU
    (32 768): worst cell 0.56."""
    params = SAMPLED[name]
    p = {**S.PARAM_DEFAULTS, **params}
    s = _material_scene("principled", params, BASE, textured=False)
    B = Backend(s, backend)
    n = 200_000 if backend == "oracle" else 32_768
    d = _unit(np.array([0.5, 0.2, -0.84])) * (-1.0 if below else 1.0)
    d[0:2] = np.abs(d[0:2])
    c = np.asarray(CARRIER_AT["quad"])
    d32 = d.astype(np.float32)
    o = (c + np.array([0.1, -0.2, 0.0]) - 3.0 * d).astype(np.float32)
    x = np.concatenate([np.tile(np.concatenate([o, d32]), (n, 1)), np.arange(n, dtype=np.float32)[:, None],
                        np.zeros((n, 1), np.float32)], 1)
    sm = B.probe(O.PROBE_BSDF_SAMPLE, x)
    assert np.all(sm[:, 0] == 1)
    ok = sm[:, 1] == 1
    wo, eta_out, spec = sm[ok, 2:5].astype(np.float64), sm[ok, 5].astype(np.float64), sm[ok, 6]
    win = -d32.astype(np.float64)
    n_g = _FLAT_FRAME[2]
    assert np.abs(np.linalg.norm(wo, axis=1) - 1).max() <= TOL
    side = (wo @ n_g) * (win @ n_g)
    eta_side = np.float64(np.float32(p["eta"])) if not below else np.float64(np.float32(1.0) / np.float32(p["eta"]))
    refl = eta_out == 0
    assert np.all(side[refl] > 0) and np.all(side[~refl] < 0)
    assert np.all(np.abs(eta_out[~refl] - eta_side) <= TOL * eta_side)
    m = S.principled(np.tile(win, (len(wo), 1)), wo, _FLAT_FRAME, n_g, np.float64(np.float32(BASE)), params)
    assert np.all(m["pdf"][~m["undecided"]] > 0)
    choose = S.lobe_weights({k: S.f32(v) for k, v in p.items()})
    # the diffuse sampler refuses nothing on a flat carrier, and its samples alone carry no specular flag
    share = (spec == 0).sum() / n
    want = 0.0 if below else choose[0]
    sig = np.sqrt(max(want * (1 - want), 1e-12) / n)
    print(f"{name} below={below} {backend}: unflagged share {share:.4f} (model {want:.4f}), refused {1 - ok.mean():.4f}, "
          f"transmitted {np.mean(~refl):.4f}")
    assert abs(share - want) <= 5 * sig
    assert np.all(side[spec == 0] > 0) and np.all(refl[spec == 0])

    def pdf_of(dirs):
        mm = S.principled(np.tile(win, (len(dirs), 1)), dirs, _FLAT_FRAME, n_g, np.float64(np.float32(BASE)), params)
        phantom = ~mm["reflect"] & ~mm["possible_transmission"]
        return np.where(phantom, 0.0, mm["pdf"])
    expected, q_err = _cell_integrals(pdf_of)
    zi = np.minimum(((wo[:, 2] + 1) * 0.5 * 6).astype(int), 5)
    pi_ = np.minimum(((np.arctan2(wo[:, 1], wo[:, 0]) + np.pi) / (2 * np.pi) * 12).astype(int), 11)
    observed = np.bincount(zi * 12 + pi_, minlength=72) / n
    tol = 5 * np.sqrt(np.maximum(expected * (1 - expected), 1.0 / n) / n) + q_err
    worst = np.abs(observed - expected) / tol
    refused = 1.0 - ok.mean()
    tol_r = 5 * np.sqrt(max(refused * (1 - refused), 1.0 / n) / n) + q_err.sum()
    print(f"{name} below={below} {backend}: model pdf integrates to {expected.sum():.5f} (quadrature +- {q_err.sum():.1e}), "
          f"worst cell {worst.max():.2f} of its allowance, refused - (1 - integral) {refused - (1 - expected.sum()):+.5f} "
          f"(allowance {tol_r:.5f})")
    assert worst.max() <= 1.0, (int(worst.argmax()), observed[worst.argmax()], expected[worst.argmax()])
    assert abs(refused - (1 - expected.sum())) <= tol_r


# =============================================================================== dielectric
DIEL_COS = (1.0, 0.97, 0.9, 0.8, 0.6, 0.4, 0.2, 0.05)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("carrier", ["sphere", "tilted"])
@pytest.mark.parametrize("ior", [1.5, 1.05])
def test_dielectric_sends_rays_on_the_models_two_directions(ior, carrier, backend):
    """8 incidences from outside and 8 from inside, 2048 seeds each: every wo is the model's mirror or Snell direction
    (32 ulp, over cos(theta_t) for the refracted one, times the carrier's own conditioning of the normal), the
    reflected share per incidence within 5 sigma of the model's probability, every ray reflected beyond the critical
    angle, eta = ior outside and 1 / ior inside, the specular flag set.
    Measured on the oracle and on the GPU alike: mirror 0.16 of its bound, Snell 0.03, reflected share within 1.4 sigma;
    4 (ior 1.5) and 2 (ior 1.05) incidences beyond the critical angle."""
    s = _material_scene("dielectric", dict(ior=ior), BASE, textured=False)
    B = Backend(s, backend)
    rng = np.random.default_rng(int(ior * 100))
    rays, geo, below = _incidences(carrier, 1, rng, cos_list=DIEL_COS)
    seeds = 2048
    n = len(rays)
    x = np.concatenate([np.repeat(rays, seeds, 0), np.tile(np.arange(seeds, dtype=np.float32), n)[:, None],
                        np.zeros((n * seeds, 1), np.float32)], 1)
    sm = B.probe(O.PROBE_BSDF_SAMPLE, x).astype(np.float64).reshape(n, seeds, 7)
    assert np.all(sm[..., 0] == 1) and np.all(sm[..., 1] == 1) and np.all(sm[..., 6] == 1)
    m = S.dielectric(-rays[:, 3:6].astype(np.float64), geo["n_s"], ior)
    assert np.array_equal(m["front"], ~below)
    assert np.abs(sm[..., 5] - m["eta"][:, None]).max() <= TOL * m["eta"].max()
    scale = geo["eps_in"] / S.EPS_IN
    d_mirror = np.abs(sm[..., 2:5] - m["mirror"][:, None, :]).max(-1)
    d_snell = np.abs(sm[..., 2:5] - m["snell"][:, None, :]).max(-1)
    b_mirror = (TOL * scale)[:, None]
    with np.errstate(divide="ignore"):
        b_snell = np.where(m["tir"], 0.0, TOL * scale * np.maximum(1.0, ior) / m["cos_t"])[:, None]
    is_mirror, is_snell = d_mirror <= b_mirror, (d_snell <= b_snell) & ~m["tir"][:, None]
    assert np.all(is_mirror | is_snell)
    # the two are the same direction only at eta -> 1 and grazing: tell them apart where they differ
    apart = np.abs(m["mirror"] - m["snell"]).max(-1) > 4 * (b_mirror[:, 0] + b_snell[:, 0])
    assert apart.all()
    assert np.all(is_mirror[m["tir"]]) and m["tir"].sum() == {1.5: 4, 1.05: 2}[ior]      # cos(theta_c) = 0.745 / 0.305
    share = is_mirror.mean(1)
    sig = np.sqrt(np.maximum(m["p_reflect"] * (1 - m["p_reflect"]), 1e-12) / seeds)
    z = np.abs(share - m["p_reflect"]) / sig
    z[m["tir"]] = 0
    e_m = _worst(d_mirror[is_mirror], np.broadcast_to(b_mirror, d_mirror.shape)[is_mirror])
    e_s = _worst(d_snell[is_snell], np.broadcast_to(b_snell, d_snell.shape)[is_snell])
    print(f"ior {ior} {carrier} {backend}: mirror error / bound {e_m:.3f}, Snell {e_s:.3f}; reflected share worst {z.max():.2f} sigma; "
          f"{int(m['tir'].sum())} incidences beyond the critical angle; P(reflect) {m['p_reflect'].min():.4f} .. 1")
    assert z.max() <= 5.0


# =============================================================================== LIGHT_SAMPLE
EMIT = (3.0, 2.0, 1.0)


def _light_scene(spheres=(), meshes=()):
    """Emitters only: spheres (centre, radius) and meshes (vertices, indices, normals or None), all of one
    diffuse_light material; a black background that is no light.  Returns (scene, number of lights)."""
    s = vimg_amd.HostScene()
    s.set_camera((0, 0, 5), (0, 0, 0), (0, 1, 0), 40.0, (8, 8))
    lt = s.add_material("diffuse_light", emit=EMIT)
    for c, r in spheres:
        s.add_sphere(c, r, lt)
    for v, idx, nrm in meshes:
        s.add_mesh(np.float32(v), np.uint32(idx), lt, normals=None if nrm is None else np.float32(nrm))
    s.set_background_const((0.0, 0.0, 0.0), add_to_lights=False)
    s.build_bvh(abi.BVH_SWEEP)
    n_lights = len(spheres) + sum(len(m[1]) for m in meshes)
    assert s.view.contents.num_lights == n_lights
    return s, n_lights


def _sample_lights(B, points, seeds):
    """LIGHT_SAMPLE from every point, `seeds` samples each and no seed twice (the samples of two points are
    independent): ([points, seeds, 10] float64, q = p + dist wi)."""
    pts = np.asarray(points, np.float32)
    assert len(pts) * seeds < 1 << 24
    x = np.concatenate([np.repeat(pts, seeds, 0), np.arange(len(pts) * seeds, dtype=np.float32)[:, None]], 1)
    out = B.probe(O.PROBE_LIGHT_SAMPLE, x).astype(np.float64).reshape(len(pts), seeds, 10)
    q = pts.astype(np.float64)[:, None, :] + out[..., 7:8] * out[..., 3:6]
    return out, q


def _sigma_cells(counts, total, p):
    return np.abs(counts - total * p) / np.sqrt(total * p * (1 - p))


SPHERE_C = np.float64(np.float32([0.3, -0.2, 0.5]))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("radius", [1e-2, 1.0, 1e2])
def test_sphere_light_samples_lie_on_the_light_with_the_claimed_pdf(radius, backend):
    """One sphere light seen from 1.001 R, 2 R, 1e3 R, from inside and from the centre: q = p + dist wi lies on the
    sphere (32 ulp of the largest coordinate), wi is a unit vector, G is |n . wi| / dist^2 for the sphere's normal at q,
    the pdf the one the sampler claims for q (Q16: cone density times G outside, 1 / area inside), Le the emission
    outside the sphere and 0 from inside (the back of the surface), and from outside q lies inside the cap of polar
    half-angle theta_max about the centre -> point axis.
    Bounds: n at q is (q - c) / R with q good to 32 ulp of the largest coordinate L, so n . wi carries 32 ulp (1 + L / R)
    and G that over dist^2; the claimed density divides by 1 - cos(theta_max), where the float32 cos(theta_max) =
    sqrt(1 - R^2 / d^2) is good to 2 ulp of 1: relative 2 ulp / (1 - cos(theta_max)) - 0.24 at d = 1e3 R, where the
    float32 value of 1 - cos(theta_max) = 5e-7 has three bits (Q34).
    Measured on the oracle and on the GPU alike, in units of the bound: on the sphere 0.07, G 0.06, pdf 0.28 (the far
    points: 6.8 % of relative error against a bound of 24 %), never outside the cap; worst cell 2.4 sigma of 3125."""
    R = np.float64(np.float32(radius))
    s, n_lights = _light_scene(spheres=[(SPHERE_C, radius)])
    B = Backend(s, backend)
    rng = np.random.default_rng(3)
    u = _unit(rng.normal(size=(6, 3)))
    pts = np.concatenate([SPHERE_C + u[0:2] * R * 1.001, SPHERE_C + u[2:4] * R * 2, SPHERE_C + u[4:6] * R * 1e3,
                          SPHERE_C + u[0:2] * R * 0.5, [SPHERE_C]]).astype(np.float32)
    outside = np.arange(len(pts)) < 6
    seeds = 2048
    out, q = _sample_lights(B, pts, seeds)
    p64 = pts.astype(np.float64)[:, None, :]
    m = S.sphere_light(p64, SPHERE_C, radius, q)
    assert np.array_equal(m["inside"][:, 0], ~outside)
    L = np.maximum(np.abs(p64).max(-1), np.abs(SPHERE_C).max() + R) + out[..., 7]
    e_on = _worst(np.abs(np.linalg.norm(q - SPHERE_C, axis=-1) - R), TOL * L)
    assert np.abs(np.linalg.norm(out[..., 3:6], axis=-1) - 1).max() <= TOL
    b_cos = TOL * (1 + L / R)
    b_G = (b_cos + TOL * np.abs(S.dot(m["n"], m["wi"]))) / m["dist"] ** 2
    e_G = _worst(np.abs(out[..., 8] - m["G"]), b_G)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_cone = np.where(m["inside"], 0.0, 2 * EPS / (1 - m["cos_max"]))
    b_pdf = np.where(m["inside"], TOL * m["pdf"], b_G / (2 * np.pi * (1 - m["cos_max"])) + m["pdf"] * (TOL + rel_cone)) / n_lights
    e_pdf = _worst(np.abs(out[..., 6] - m["pdf"] / n_lights), b_pdf)
    le = S.one_sided_le(np.float64(np.float32(EMIT)), m["n"], m["wi"])
    # the side of the light a sample sees: decided where |n . wi| exceeds its bound
    sure = np.abs(S.dot(m["n"], m["wi"])) > b_cos
    assert np.array_equal(out[..., 0:3][sure], le[sure])
    assert np.all(out[~outside][..., 0:3] == 0) and sure[~outside].all()
    lit = (out[outside][..., 0] > 0).mean()
    e_cap = _worst(np.maximum(m["cos_max"] - m["cos_cap"], 0.0)[outside], b_cos[outside])
    print(f"R {radius:g} {backend}: on the sphere {e_on:.3f} of the bound, G {e_G:.3f}, pdf {e_pdf:.3f}, outside the cap by {e_cap:.3f}; "
          f"lit share outside {lit:.3f}; undecided side {1 - sure.mean():.4f}")
    assert e_on <= 1 and e_G <= 1 and e_pdf <= 1 and e_cap <= 1
    assert 1 - sure.mean() <= 0.01
    # distribution: from 2 R the cosine about the axis is uniform on [cos theta_max, 1] and the azimuth uniform;
    # from inside the sphere is covered uniformly (z and azimuth about any axis)
    n_d = 200_000 if backend == "oracle" else 16_384
    for k, label in ((2, "2 R"), (6, "inside")):
        _, q_d = _sample_lights(B, pts[k:k + 1], n_d)
        md = S.sphere_light(pts[k].astype(np.float64), SPHERE_C, radius, q_d[0])
        ax = md["axis"] if outside[k] else np.array([0.0, 0.0, 1.0])
        tg, bt = PR.branchless_onb(ax)
        nn = md["n"]
        lo = md["cos_max"] if outside[k] else -1.0
        ci = np.clip((((nn @ ax) - lo) / (1 - lo) * 8).astype(int), 0, 7)
        ai = np.minimum(((np.arctan2(nn @ bt, nn @ tg) + np.pi) / (2 * np.pi) * 8).astype(int), 7)
        z = _sigma_cells(np.bincount(ci * 8 + ai, minlength=64), n_d, 1 / 64)
        print(f"R {radius:g} {backend} {label}: worst of 8 x 8 cells {z.max():.2f} sigma of {n_d // 64}")
        assert z.max() <= 5.0


def _quad_light(with_normals):
    v = np.array([[-1.5, 2.0, -1.0], [1.5, 2.0, -1.0], [1.5, 2.2, 1.0], [-1.5, 2.2, 1.0]], np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    nrm = None
    if with_normals:                       # leaning outwards from the quad's centre, all on the quad's lower side
        g = _unit(np.cross(v[1] - v[0], v[2] - v[0]).astype(np.float64))
        nrm = _unit(g + 0.35 * _unit(v.astype(np.float64) - v.astype(np.float64).mean(0))).astype(np.float32)
    return v, idx, nrm


def _check_triangle_samples(out, q, pts, tris, n_lights, label):
    """Every sample on one of the triangles, with that triangle's and that point's figures; returns the triangle index
    per sample and its barycentrics."""
    p64 = pts.astype(np.float64)[:, None, :]
    L = np.maximum(np.abs(p64).max(-1), max(np.abs(t[0]).max() for t in tris)) + out[..., 7]
    best = np.full(q.shape[:2], -1)
    score = np.full(q.shape[:2], -np.inf)
    models = []
    for k, (v, nrm) in enumerate(tris):
        m = S.triangle_light(p64, v[0], v[1], v[2], q, normals=nrm)
        models.append(m)
        height = 2 * m["area"] / max(np.linalg.norm(v[1] - v[0]), np.linalg.norm(v[2] - v[1]), np.linalg.norm(v[0] - v[2]))
        sc = np.minimum(m["bary"].min(-1) * height, -np.abs(m["plane"]))
        best = np.where(sc > score, k, best)
        score = np.maximum(score, sc)
    pick = lambda key: np.choose(best, [mm[key] for mm in models]) if models[0][key].ndim == 2 else \
        np.stack([np.choose(best, [mm[key][..., c] for mm in models]) for c in range(3)], -1)
    e_on = _worst(-score, TOL * L)                     # plane distance and barycentrics (as lengths) >= -bound
    n, wi, dist, G, pdf, bary = (pick(k) for k in ("n", "wi", "dist", "G", "pdf", "bary"))
    cos = S.dot(n, wi)
    b_cos = TOL * (1 + L / dist)                          # wi = (q - p) / dist with q good to 32 ulp of L
    b_G = (b_cos + TOL * np.abs(cos)) / dist ** 2
    e_G = _worst(np.abs(out[..., 8] - G), b_G)
    e_pdf = _worst(np.abs(out[..., 6] - pdf / n_lights), TOL * pdf / n_lights)
    e_wi = np.abs(out[..., 3:6] - wi).max()
    sure = np.abs(cos) > b_cos
    le = S.one_sided_le(np.float64(np.float32(EMIT)), n, wi)
    assert np.array_equal(out[..., 0:3][sure], le[sure]), label
    print(f"{label}: on a triangle {e_on:.3f} of the bound, G {e_G:.3f}, pdf {e_pdf:.3f}, undecided side {1 - sure.mean():.4f}")
    assert np.abs(np.linalg.norm(out[..., 3:6], axis=-1) - 1).max() <= TOL and e_wi <= TOL
    assert e_on <= 1 and e_G <= 1 and e_pdf <= 1 and 1 - sure.mean() <= 0.01
    return best, bary, le


def _sub_triangle(bary):
    """Which of the 16 equal sub-triangles (a 4 x 4 barycentric grid) holds the point."""
    a, b = bary[..., 0] * 4, bary[..., 1] * 4
    i, j = np.minimum(np.floor(a).astype(int), 3), np.minimum(np.floor(b).astype(int), 3)
    upper = (a - i) + (b - j) > 1                      # the inverted triangle of the cell
    row_start = np.array([0, 7, 12, 15])               # row i holds 2 (4 - i) - 1 sub-triangles
    return np.clip(row_start[i] + 2 * j + upper, 0, 15)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("with_normals", [False, True])
def test_quad_light_is_filled_uniformly_and_radiates_from_one_side(with_normals, backend):
    """A quad light (two triangles) with and without vertex normals, seen from three points below it and one above:
    every sample on one of the two triangles, G with the INTERPOLATED normal where the mesh has normals, pdf
    1 / area / 2, Le the emission from below and 0 from above; both triangles chosen equally and each filled uniformly
    in area (16 sub-triangles), 5 sigma per cell.
    Measured on the oracle: on a triangle 0.06 of the bound, G 0.06, pdf 0.02; triangles 0.04 sigma, worst sub-triangle
    2.0 sigma of 6250 (GPU: 2.5 sigma of 1024)."""
    v, idx, nrm = _quad_light(with_normals)
    s, n_lights = _light_scene(meshes=[(v, idx, nrm)])
    assert n_lights == 2
    B = Backend(s, backend)
    pts = np.float32([[0.2, 0.0, 0.1], [-1.0, 1.5, 0.5], [3.0, 1.0, -2.0], [0.1, 4.0, 0.0]])
    seeds = 50_000 if backend == "oracle" else 8192
    out, q = _sample_lights(B, pts, seeds)
    v64 = v.astype(np.float64)
    tris = [(v64[t], None if nrm is None else nrm.astype(np.float64)[t]) for t in idx]
    best, bary, le = _check_triangle_samples(out, q, pts, tris, n_lights, f"quad light normals={with_normals} {backend}")
    assert np.all(out[3][:, 0:3] == 0) and np.all(out[0][:, 0:3] == np.float32(EMIT))       # above: the back; below: lit
    if with_normals:
        assert np.abs(out[..., 8] - S.triangle_light(pts.astype(np.float64)[:, None, :], *tris[0][0], q)["G"]).max() > 1e-3
    total = best.size
    z_tri = abs((best == 0).sum() - total / 2) / np.sqrt(total / 4)
    cells = np.bincount((best * 16 + _sub_triangle(bary)).ravel(), minlength=32)
    z = _sigma_cells(cells, total, 1 / 32)
    print(f"quad light normals={with_normals} {backend}: triangles {z_tri:.2f} sigma, worst of 32 sub-triangles {z.max():.2f} sigma")
    assert z_tri <= 5 and z.max() <= 5


@pytest.mark.parametrize("backend", BACKENDS)
def test_three_emitters_are_chosen_equally(backend):
    """A sphere of radius 0.5, a lone triangle and a quad - four lights of very different areas: each is chosen for a
    quarter of the samples (5 sigma), every sample lies on the light it belongs to, and its pdf carries the prior 1 / 4
    on that light's own density."""
    tri_v = np.float32([[4.0, 0.0, 0.0], [4.0, 0.3, 0.0], [4.0, 0.0, 0.2]])
    qv, qidx, _ = _quad_light(False)
    centre, R = np.float64(np.float32([-3.0, 1.0, 0.5])), 0.5
    s, n_lights = _light_scene(spheres=[(centre, R)], meshes=[(tri_v, [[0, 1, 2]], None), (qv, qidx, None)])
    assert n_lights == 4
    B = Backend(s, backend)
    pts = np.float32([[0.0, 0.0, 0.0], [1.0, -1.0, 2.0]])
    seeds = 100_000 if backend == "oracle" else 16_384
    out, q = _sample_lights(B, pts, seeds)
    on_sphere = np.abs(np.linalg.norm(q - centre, axis=-1) - R) <= TOL * (6 + out[..., 7])
    ms = S.sphere_light(pts.astype(np.float64)[:, None, :], centre, R, q)
    e_s = _worst(np.abs(out[..., 6] - ms["pdf"] / 4)[on_sphere], (ms["pdf"] * (TOL * (1 + 6 / R) / np.abs(S.dot(ms["n"], ms["wi"]))
                                                                               + TOL + 2 * EPS / (1 - ms["cos_max"])) / 4)[on_sphere])
    tris = [(tri_v.astype(np.float64), None)] + [(qv.astype(np.float64)[t], None) for t in qidx]
    keep = ~on_sphere
    # the triangle checks take rectangular arrays: look at the samples of each point that are not on the sphere
    counts = np.zeros(4)
    counts[0] = on_sphere.sum()
    for k in range(len(pts)):
        sel = keep[k]
        best, _, _ = _check_triangle_samples(out[k:k + 1, sel], q[k:k + 1, sel], pts[k:k + 1], tris, 4, f"three emitters point {k} {backend}")
        counts[1:] += np.bincount(best.ravel(), minlength=3)
    z = _sigma_cells(counts, on_sphere.size, 0.25)
    print(f"three emitters {backend}: shares {counts / on_sphere.size}, worst {z.max():.2f} sigma; sphere pdf {e_s:.3f} of its bound")
    assert z.max() <= 5 and e_s <= 1


# =============================================================================== the model on its own
def test_model_lambertian_white_furnace():
    """The integral of f (with its cosine) over the sphere is the albedo: no energy made or lost."""
    n_s = _unit(np.array([0.3, -0.5, 0.8]))
    val, err = S.integrate_sphere(lambda w: S.lambertian(w, n_s, (1.0, 0.6, 0.25))["f"], n0=32)
    assert np.abs(val - (1.0, 0.6, 0.25)).max() <= 1e-4 + err
    val, _ = S.integrate_sphere(lambda w: S.lambertian(w, n_s, (1.0, 1.0, 1.0))["pdf"], n0=32)
    assert abs(val - 1) <= 1e-4


@pytest.mark.parametrize("ax,ay", [(0.3, 0.3), (0.2, 0.6), (0.05, 0.1)])
def test_model_gtr2_is_a_distribution_of_normals(ax, ay):
    """[B12] B.2: the projected area of the microfacets is the macro surface's, int D(h) (n . h) dh = 1."""
    val, err = S.integrate_sphere(lambda h: np.where(h[:, 2] > 0, S.gtr2(h, ax, ay)[0] * h[:, 2], 0.0), n0=128)
    assert abs(val - 1) <= 2e-4 + err, val


@pytest.mark.parametrize("a", [0.3, 0.1, 0.03])
def test_model_gtr1_is_a_distribution_of_normals(a):
    val, err = S.integrate_sphere(lambda h: np.where(h[:, 2] > 0, S.gtr1(h[:, 2], a)[0] * h[:, 2], 0.0), n0=128)
    assert abs(val - 1) <= 2e-4 + err, val


def test_model_is_reciprocal_without_transmission():
    """Helmholtz: f / cos(theta_o) is symmetric in its two directions for the diffuse, subsurface, sheen, clearcoat and
    metal lobes (anisotropic too), in a tilted frame."""
    rng = np.random.default_rng(1)
    n = _unit(np.array([0.2, 0.3, 0.9]))
    t, b = PR.branchless_onb(n)
    a, c = _unit(rng.normal(size=(2000, 3))), _unit(rng.normal(size=(2000, 3)))
    a, c = a * np.sign(a @ n)[:, None], c * np.sign(c @ n)[:, None]              # both above
    params = dict(metallic=0.3, roughness=0.4, anisotropic=0.6, subsurface=0.4, sheen=0.7, sheen_tint=0.8, spec_tint=0.5,
                  clearcoat=0.8, clearcoat_gloss=0.3)
    f_ac = S.principled(a, c, (t, b, n), n, BASE, params, lobes=True)
    f_ca = S.principled(c, a, (t, b, n), n, BASE, params, lobes=True)
    for lobe in ("diffuse", "subsurface", "sheen", "clearcoat", "metal"):
        lhs = f_ac["lobes"][lobe] / (c @ n)[:, None]
        rhs = f_ca["lobes"][lobe] / (a @ n)[:, None]
        assert np.abs(lhs).max() > 0 and np.abs(lhs - rhs).max() <= 1e-12 * np.abs(lhs).max(), lobe


def test_model_lobe_pdfs_are_normalised():
    """The diffuse pdf integrates to 1 over the hemisphere.  The clearcoat pdf D |n . h| / (4 h . wo) carries the
    reflection's Jacobian: at normal incidence wo stays above the surface for theta_h < 45 degrees, and GTR1's mass
    inside that cone is 1 - ln(1 + (a^2 - 1) / 2) / ln(a^2) in closed form.  The metal pdf is the density of visible
    normals [H14]: all of its mass is on reflected directions, above or below the horizon, so over the upper hemisphere
    it integrates to at most 1 and to more than 0.9 at normal incidence and roughness 0.5."""
    n = np.array([0.0, 0.0, 1.0])
    win = np.tile(n, (1, 1))
    for gloss in (0.0, 0.5):
        params = dict(clearcoat=1.0, clearcoat_gloss=gloss, roughness=0.5)
        pdfs = lambda w: S.principled(np.tile(n, (len(w), 1)), w, _FLAT_FRAME, n, BASE, params, lobes=True)["lobe_pdfs"]
        a2 = S.clearcoat_alpha(S.f32(gloss), False) ** 2
        val, err = S.integrate_sphere(lambda w: pdfs(w)["clearcoat"], n0=128, n_max=512)
        assert abs(val - (1 - np.log(1 + (a2 - 1) / 2) / np.log(a2))) <= 2e-4 + err, (gloss, val)
    val, err = S.integrate_sphere(lambda w: pdfs(w)["diffuse"], n0=64, n_max=256)
    assert abs(val - 1) <= 1e-4 + err
    val, err = S.integrate_sphere(lambda w: pdfs(w)["metal"], n0=128, n_max=256)
    assert 0.9 < val <= 1 + 1e-4 + err, val


def test_model_fresnel_and_snell():
    """Fresnel at normal incidence is ((eta - 1) / (eta + 1))^2 from either side, 1 beyond the critical angle, and
    Schlick's form agrees there; the Snell direction has sin(theta_t) = sin(theta_i) / eta and lies in the plane of
    incidence; the mirror direction keeps the angle."""
    for eta in (1.33, 1.5, 2.4, 1 / 1.5):
        assert abs(S.fresnel_dielectric(1.0, eta) - ((eta - 1) / (eta + 1)) ** 2) <= 1e-15
    assert S.fresnel_dielectric(0.5, 1 / 1.5) == 1.0                      # sin 60 degrees > 1 / 1.5
    assert abs(S.fresnel_dielectric(0.3, 1.0)) <= 1e-30
    rng = np.random.default_rng(2)
    n = _unit(rng.normal(size=(500, 3)))
    d = _unit(rng.normal(size=(500, 3)))
    for ior in (1.5, 1.05):
        m = S.dielectric(-d, n, ior)
        eta = m["eta"]                                                    # n_t / n_i on the ray's side
        ok = ~m["tir"]
        sin_i = np.sqrt(1 - m["cos_i"] ** 2)
        nn = np.where(m["front"][:, None], n, -n)
        sin_t = np.linalg.norm(np.cross(m["snell"], nn), axis=1)
        assert np.abs(sin_t - sin_i / eta)[ok].max() <= 1e-12
        assert np.abs(np.linalg.norm(m["snell"], axis=1) - 1)[ok].max() <= 1e-12
        assert np.abs(S.dot(np.cross(d, nn), m["snell"]))[ok].max() <= 1e-12
        assert np.all(S.dot(m["snell"], nn)[ok] < 0) and np.all(S.dot(m["mirror"], nn) > 0)
        assert np.abs(S.dot(m["mirror"], nn) - m["cos_i"]).max() <= 1e-12
        assert np.array_equal(m["tir"], sin_i / eta > 1)
        i32 = S.f32(ior)
        assert abs(S.dielectric(n[0], n[0], ior)["p_reflect"] - ((i32 - 1) / (i32 + 1)) ** 2) <= 1e-12


# =============================================================================== two renders
RENDER_MATS = {
    "lambertian": ("lambertian", {}),
    "plastic": ("principled", dict(metallic=0.0, roughness=0.5, specular=0.5, sheen=0.7)),
    "metal-aniso": ("principled", dict(metallic=1.0, roughness=0.4, anisotropic=0.5)),
    "clearcoat": ("principled", dict(metallic=0.0, roughness=0.6, clearcoat=1.0, clearcoat_gloss=0.5)),
}
RENDER_RES, RENDER_FOV, RENDER_COS = (8, 8), 2.0, 0.8


def _render_scene(kind, params, light=None):
    """Carrier (a) alone, seen by a 2 degree camera at cos(theta_i) = 0.8 from 30 units away (the 8 x 8 frame covers a
    square unit of the quad); a white background that is no light, or a sphere light and a black one."""
    s = vimg_amd.HostScene()
    sin = np.sqrt(1 - RENDER_COS ** 2)
    frm = 30.0 * np.array([sin * np.cos(0.4), sin * np.sin(0.4), RENDER_COS])
    s.set_camera(tuple(frm), (0, 0, 0), (0, 0, 1), RENDER_FOV, RENDER_RES)
    m = s.add_material(kind, tex=s.add_texture_const(BASE), **params)
    v, idx, uv, _ = _quad_mesh(np.eye(3), (0.0, 0.0, 0.0))
    s.add_mesh(v, idx, m, uv_sets=[uv], color_uv=0, mr_uv=0)
    if light is None:
        s.set_background_const((1.0, 1.0, 1.0), add_to_lights=False)
    else:
        s.add_sphere(light[0], light[1], s.add_material("diffuse_light", emit=EMIT))
        s.set_background_const((0.0, 0.0, 0.0), add_to_lights=False)
    s.build_bvh(abi.BVH_SWEEP)
    return s


def _pixel_dirs(s, ox=0.5, oy=0.5):
    """The pinhole direction through the point (ox, oy) of each pixel, [H, W, 3] in the image's row order (row 0 is the
    top), and where it meets z = 0."""
    cam = s.view.contents.camera
    c2w = np.array(list(cam.cam_to_world), dtype=np.float64).reshape(4, 4).T
    ys, xs = np.mgrid[0:RENDER_RES[1], 0:RENDER_RES[0]]
    d = PR.pinhole_dir_cam(xs.ravel() + ox, ys.ravel() + oy, RENDER_FOV, RENDER_RES) @ c2w[:3, :3].T
    d = d.reshape(RENDER_RES[1], RENDER_RES[0], 3)[::-1]                  # image row = H - 1 - y
    o = c2w[:3, 3]
    p = o - d * (o[2] / d[..., 2])[..., None]
    return d, p


def _bilinear_over_frame(corner_values):
    """Values at the four corner pixels (top-left, top-right, bottom-left, bottom-right) spread over the 8 x 8 frame:
    across 2 degrees every quantity here is linear to far below the tests' allowances (asserted at the centre)."""
    tl, tr, bl, br = (np.asarray(c, np.float64) for c in corner_values)
    a = (np.arange(RENDER_RES[0]) / (RENDER_RES[0] - 1))[None, :, None]
    b = (np.arange(RENDER_RES[1]) / (RENDER_RES[1] - 1))[:, None, None]
    return (tl * (1 - a) + tr * a) * (1 - b) + (bl * (1 - a) + br * a) * b


def _sampled_pair(kind, params, win, dirs):
    """What the integrators multiply a BSDF sample in direction `dirs` with, as two parts: the sample is DRAWN with the
    regularize flag as it stood before the bounce (off at the first hit), but EVALUATED with the flag as the sample
    sets it - on after a sample without the specular flag, i.e. one of the diffuse lobe (Q5, and Q35 for `material`).
    Returns [(density of such samples, f, pdf as evaluated)] for the specular-flagged and the unflagged samples."""
    base = np.float64(np.float32(BASE))
    if kind == "lambertian":
        m = S.lambertian(dirs, _FLAT_FRAME[2], base)
        return [(m["pdf"], m["f"], m["pdf"])]
    w = np.tile(win, (len(dirs), 1))
    m = S.principled(w, dirs, _FLAT_FRAME, _FLAT_FRAME[2], base, params, lobes=True)
    q = {k: S.f32(v) for k, v in {**S.PARAM_DEFAULTS, **params}.items()}
    same = S.alphas(q["roughness"], q["anisotropic"], True) == S.alphas(q["roughness"], q["anisotropic"], False) \
        and S.clearcoat_alpha(q["clearcoat_gloss"], True) == S.clearcoat_alpha(q["clearcoat_gloss"], False)
    m_r = m if same else S.principled(w, dirs, _FLAT_FRAME, _FLAT_FRAME[2], base, params, regularize=True)
    p_diff = S.lobe_weights({k: S.f32(v) for k, v in {**S.PARAM_DEFAULTS, **params}.items()})[0] * m["lobe_pdfs"]["diffuse"]
    return [(m["pdf"] - p_diff, m["f"], m["pdf"]), (p_diff, m_r["f"], m_r["pdf"])]


def _albedo_moments(kind, params, win):
    """Mean and second moment of f / pdf over the samples that leave the surface (nothing here transmits), per
    channel: the directional albedo int f over the reachable directions, but for Q35."""
    def both(dirs):
        up = dirs[:, 2] > 0
        out = np.zeros((len(dirs), 6))
        for dens, f, pdf in _sampled_pair(kind, params, win, dirs):
            ratio = np.where((up & (pdf > 0))[:, None], f * S._safe_div(1.0, pdf)[:, None], 0.0)
            out += np.concatenate([ratio, ratio * ratio], 1) * np.where(up, dens, 0.0)[:, None]
        return out
    val, err = S.integrate_sphere(both, n0=64, rel=1e-4, n_max=256)
    return val[:3], val[3:], err


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(RENDER_MATS))
def test_material_frame_is_the_directional_albedo(name, backend):
    """`material` at depth 2 under a white background that is no light: a sample carries f / pdf if the BSDF sample
    leaves the surface and 0 if it is refused, so a pixel's mean is the model's directional albedo over the reachable
    directions - exactly the colour for the Lambertian - within 5 standard errors of the model's own variance
    int f^2 / pdf - (int f)^2 at 4096 samples, per pixel and over the 64 pixels jointly.
    The expectation carries Q35: a sample of the diffuse lobe is evaluated with the regularised lobes.
    Measured on the oracle (the GPU's frames are the same): Lambertian 4.0e-5 of the colour (bound 2.4e-4); jointly -0.04 /
    0.86 / 1.27 sigma, worst pixel 3.4 sigma; without Q35 in the model the clearcoat frame is 5.2 sigma (0.53 %) low."""
    kind, params = RENDER_MATS[name]
    s = _render_scene(kind, params)
    spp = 4096
    img = Backend(s, backend).render("material", spp, 2)
    d, _ = _pixel_dirs(s)
    if kind == "lambertian":
        err = np.abs(img / np.float64(np.float32(BASE)) - 1).max()
        print(f"{name} {backend}: max |pixel / colour - 1| {err:.2e}")
        assert err <= (spp + 4) * EPS                      # a float32 running sum of n terms: (n - 1) u, and f / pdf to 4 ulp
        return
    corners = [d[0, 0], d[0, -1], d[-1, 0], d[-1, -1], d[RENDER_RES[1] // 2, RENDER_RES[0] // 2]]
    mom = [_albedo_moments(kind, params, -c) for c in corners]
    albedo, second = _bilinear_over_frame([m[0] for m in mom[:4]]), _bilinear_over_frame([m[1] for m in mom[:4]])
    q_err = max(m[2] for m in mom)
    centre = (RENDER_RES[1] // 2, RENDER_RES[0] // 2)
    lin_err = np.abs(albedo[centre] - mom[4][0]).max()               # centre pixel: interpolated against evaluated
    sem = np.sqrt(np.maximum(second - albedo ** 2, 0.0) / spp)
    z_px = (np.abs(img - albedo) - q_err - lin_err) / sem
    z_all = (np.abs(img.mean((0, 1)) - albedo.mean((0, 1))) - q_err - lin_err) / (np.sqrt((sem ** 2).sum((0, 1))) / 64)
    print(f"{name} {backend}: albedo {albedo.mean((0, 1))}, frame mean / model {img.mean((0, 1)) / albedo.mean((0, 1))}, "
          f"joint {z_all.max():.2f} sigma, worst pixel {z_px.max():.2f} sigma; quadrature {q_err:.1e}, interpolation {lin_err:.1e}")
    assert q_err <= 1e-3 * albedo.min() and lin_err <= 1e-3 * albedo.min()
    assert z_all.max() <= 5 and z_px.max() <= 5


LIGHT_AT, LIGHT_R = np.array([0.5, -0.3, 4.0]), 0.06


def _direct_light(kind, params, win, p, n_cos=6, n_phi=12):
    """The model's int_light f Le d omega at the point p of the quad (normal +z) for the sphere light, by quadrature
    over the light's surface in polar coordinates about the centre -> p axis (Gauss-Legendre in the cosine, where the
    integrand is smooth down to the limb; midpoints in the azimuth, where it is periodic); and what the reference's estimator
    converges to instead: next-event samples are drawn uniformly in a cap of polar half-angle theta_max about that
    axis ON the sphere but weighted with the cone's density times G (Q16), both strategies are balanced with that
    claimed density, and a BSDF sample is evaluated with the regularize flag it sets itself (Q5).
    Returns (truth [3], estimator's expectation [3])."""
    c, R = LIGHT_AT, np.float64(np.float32(LIGHT_R))
    axis = S.unit(p - c)
    x = R / np.linalg.norm(p - c)
    cos_vis, cos_max = x, np.sqrt(1 - x * x)             # visible cap: cos(theta) > R / d; sampled cap: theta < asin(R / d)
    tg, bt = PR.branchless_onb(axis)
    gx, gw = np.polynomial.legendre.leggauss(n_cos)
    u, gw = 0.5 * (gx + 1), 0.5 * gw
    phi = (np.arange(n_phi) + 0.5) / n_phi * 2 * np.pi
    emit = np.float64(np.float32(EMIT))
    claimed = 1.0 / (2 * np.pi * (1 - cos_max))          # the cone's density; times G it is the claimed area density

    def over(cos_lo):
        ct = cos_lo + (1 - cos_lo) * u                   # uniform in cos(theta): equal solid angle from the centre
        CT, PH = np.meshgrid(ct, phi, indexing="ij")
        st = np.sqrt(1 - CT * CT)
        nrm = (st * np.cos(PH))[..., None] * tg + (st * np.sin(PH))[..., None] * bt + CT[..., None] * axis
        m = S.sphere_light(p, c, LIGHT_R, (c + R * nrm).reshape(-1, 3))
        le = S.one_sided_le(emit, m["n"], m["wi"])
        dw = np.repeat(gw, n_phi)[:, None] * (2 * np.pi * (1 - cos_lo) / n_phi)
        return m, _sampled_pair(kind, params, win, m["wi"]), le, dw
    m, parts, le, dw = over(cos_vis)
    jac = m["G"] * R * R                                 # d omega (from p) per d omega (from the centre)
    truth = (parts[0][1] * le * jac[:, None] * dw).sum(0)
    # a BSDF sample that reaches the light: f / pdf as evaluated, weight pdf / (pdf + claimed) - G cancels in the balance
    by_bsdf = sum((f * S._safe_div(dens, pdf * (pdf + claimed) / pdf)[:, None] * le * jac[:, None] * dw).sum(0) for dens, f, pdf in parts)
    m, parts, le, dw = over(cos_max)
    f, pdf = parts[0][1], parts[0][2]                    # next-event estimation evaluates with the flag off
    # E[w_l f Le G / (claimed G)] under the TRUE area density 1 / (2 pi (1 - cos_max) R^2): w_l f Le per solid angle from c
    by_light = (f * le * (claimed / (pdf + claimed))[:, None] * dw).sum(0)
    return truth, by_light + by_bsdf


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["plastic", "metal-aniso", "clearcoat"])
def test_mis_frame_is_the_lights_integral(name, backend):
    """`mis` at depth 2 with one small sphere light over carrier (a), black background: the frame's mean is the model's
    int_light f Le d omega, evaluated over every pixel's square.  R / d = 0.015: the model's own figure for what Q16 and Q5
    do to the estimator's expectation is below 1e-3 (asserted).  Allowance: 5 standard errors of the 64-pixel mean,
    from the ORACLE's per-pixel spread about the model at this sample count, plus that bias.
    Measured on the oracle (the GPU's frames are the same): frame mean / model - 1 = +2.4e-4 / +0.6e-4 / +1.5e-4 at a
    standard error of 6e-5; bias of the expectation 0.5e-4 / 1.4e-4 / 0.5e-4."""
    kind, params = RENDER_MATS[name]
    s = _render_scene(kind, params, light=(LIGHT_AT, LIGHT_R))
    spp = 1024
    img = Backend(s, backend).render("mis", spp, 2)
    ref = img if backend == "oracle" else O.render(s, s.default_params(integrator="mis", samples=spp, depth=2))[0].astype(np.float64)
    # a pixel's samples cover its square: the model is averaged over the 2 x 2 Gauss points of the pixel, exact for
    # an integrand that is cubic across it
    truth, expect = np.zeros(img.shape), np.zeros(img.shape)
    g = 0.5 / np.sqrt(3.0)
    for ox in (0.5 - g, 0.5 + g):
        for oy in (0.5 - g, 0.5 + g):
            d, p = _pixel_dirs(s, ox, oy)
            for i in range(RENDER_RES[1]):
                for j in range(RENDER_RES[0]):
                    t, e = _direct_light(kind, params, -d[i, j], p[i, j])
                    truth[i, j] += t / 4
                    expect[i, j] += e / 4
    d, p = _pixel_dirs(s)
    bias = np.abs(expect.mean((0, 1)) / truth.mean((0, 1)) - 1).max()
    c = (RENDER_RES[1] // 2, RENDER_RES[0] // 2)
    q_err = np.abs(_direct_light(kind, params, -d[c], p[c], 12, 24)[0] - _direct_light(kind, params, -d[c], p[c])[0]).max()
    sem = (ref - truth).std((0, 1)) / 8
    got, want = img.mean((0, 1)), truth.mean((0, 1))
    print(f"{name} {backend}: frame mean / model {got / want}, SEM / model {sem / want}, bias of the expectation {bias:.2e}, "
          f"quadrature {q_err / want.min():.1e}")
    assert bias <= 1e-3 and q_err <= 1e-4 * want.min()
    # ... and the float32 running sum of a pixel's samples: (n - 1) u
    assert np.all(sem > 0) and np.all(np.abs(got - want) <= 5 * sem + (bias + spp * EPS) * want + q_err)
