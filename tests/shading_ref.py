"""A float64 model of what a path evaluates at every vertex: the Principled lobes, the Lambertian, the smooth
dielectric and the two area-light samplers.  numpy only; it imports nothing of the oracle and was
written from the published forms, each cited where it stands, and from the quirk list of SURVEY.md / DESIGN.md:

  [B12]  Burley, "Physically Based Shading at Disney", SIGGRAPH 2012 course notes: the diffuse and retro-reflection
         term (eq. 4), sheen (5.4), GTR1 / GTR2 (appendix B), the clearcoat (5.6: ior 1.5, fixed roughness 0.25 in G)
  [B15]  Burley, "Extending the Disney BRDF to a BSDF with Integrated Subsurface Scattering", SIGGRAPH 2015: the
         subsurface blend (Hanrahan-Krueger form, eq. 6), specular transmission with sqrt(base colour)
  [H14]  Heitz, "Understanding the Masking-Shadowing Function", JCGT 2014: Lambda of an anisotropic GGX (eq. 86), the
         density of visible normals D G1 (h.wi) / (n.wi) (eq. 16)
  [W07]  Walter et al., "Microfacet Models for Refraction through Rough Surfaces", EGSR 2007: the generalised
         half-vector (eq. 16), its Jacobian (eq. 17), the transmission term (eq. 21)
  [S94]  Schlick, "An Inexpensive BRDF Model for Physically-based Rendering", 1994: F0 + (1 - F0)(1 - c)^5
  [dG06] de Greve, "Reflections and Refractions in Ray Tracing", 2006: mirror and Snell directions, Schlick from the
         denser side on cos(theta_t)
  Fresnel's equations for unpolarised light, as in any optics text.

Directions: `win` points AWAY from the surface towards where the ray came from (the reference's dir_in = -ray.d), `wo`
away from the surface along the scattered ray.  Every function is vectorised over a leading axis.

Bounds.  A float32 evaluation of one of these expression trees keeps 32 ulp (TOL) when every factor is well
conditioned.  What enters a factor - a local component of a direction or of the half-vector, a dot product of unit
vectors - carries an ABSOLUTE error of EPS_IN = 8 * 2^-24 (a normalisation and a three-term dot product against a
frame vector that is itself a normalised float32 vector: 0.5 ulp per product and per sum, the frame's own components
as much again).  A factor g(x) turns that into a RELATIVE error kappa * EPS_IN with kappa = |g'(x) / g(x)|; a lobe is a
product of factors, so its relative bound is TOL + EPS_IN * sum(kappa); f and pdf are weighted sums of lobes, so their
bound is the sum of |weight * lobe| * (relative bound of the lobe).  The kappas that are not of order one:

  GTR2      den = hx^2 / ax^2 + hy^2 / ay^2 + hz^2, D ~ den^-2:      2 * (2|hx| / ax^2 + 2|hy| / ay^2 + 2|hz|) / den
  GTR1      den = 1 + (a^2 - 1) hz^2:                                2 |hz| (1 - a^2) / den
  Lambda    v = ((wx ax)^2 + (wy ay)^2) / wz^2, G = 2 / (1 + s), s = sqrt(1 + v):   dv / (2 s (1 + s))
  (1 - x)^5 inside F0 + (1 - F0)(1 - x)^5:                           5 (1 - x)^4 (1 - F0) / F
  Fresnel   F(c, eta), with its square root of 1 - (1 - c^2) / eta^2:  the larger of |F(c +- dc) - F(c)|, taken directly
            (it covers the jump to 1 at the critical angle), the same with the radicand moved by 2 ulp of
            max(1, 1 / eta^2), and 4 ulp on each amplitude; this one enters absolutely, |dF| times the rest of the term
  max(n.wo, 0) of the diffuse, subsurface and sheen lobes and of the diffuse pdf: absolutely too, the input error
            times the rest of the term - the float32 cosine may be positive where the exact one is clamped
  1 / |n.wi|, 1 / |h.wo|, 1 / |n.h|:                                 1 / |.|
  the half-vector's normalisation (w_i + eta w_o) / |w_i + eta w_o|: every error of a component of h is multiplied
            by (1 + eta) / |w_i + eta w_o|  (2 / |w_i + w_o| for a reflection)
"""
import numpy as np

D = np.float64
EPS = 2.0 ** -24
TOL = 32 * EPS
EPS_IN = 8 * EPS
LUMINANCE = np.array([0.212671, 0.715160, 0.072169])      # CIE Y of linear sRGB primaries, the digits of [B12]'s code
ROUGHNESS_MIN, ALPHA_MIN = 0.01, 1e-4
REG_THRESHOLD, REG_MIN, REG_MAX = 0.1, 0.03, 0.1

PARAM_DEFAULTS = dict(metallic=0.0, roughness=0.5, spec_trans=0.0, subsurface=0.0, specular=0.5, spec_tint=0.0,
                      anisotropic=0.0, sheen=0.0, sheen_tint=0.5, clearcoat=0.0, clearcoat_gloss=1.0, eta=1.5)


def unit(v):
    v = np.asarray(v, D)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def dot(a, b):
    return np.sum(np.asarray(a, D) * np.asarray(b, D), -1)


def f32(x):
    """The value a float32 parameter really has."""
    return D(np.float32(x))


def _safe_div(num, den):
    num, den = np.broadcast_arrays(np.asarray(num, D), np.asarray(den, D))
    out = np.zeros(num.shape, D)
    np.divide(num, den, out=out, where=den != 0)
    return out


# ------------------------------------------------------------------------------------------------- factors
def schlick_weight(x):
    return (1.0 - x) ** 5


def fresnel_dielectric(c, eta, amplitudes=False, t2_shift=0.0):
    """Unpolarised Fresnel reflectance at cosine c on the incident side, eta = n_t / n_i; 1 beyond the critical angle."""
    c = np.asarray(c, D)
    t2 = 1.0 - (1.0 - c * c) / (eta * eta) + t2_shift
    t = np.sqrt(np.maximum(t2, 0.0))
    ci = np.abs(c)
    rs = _safe_div(ci - eta * t, ci + eta * t)
    rp = _safe_div(eta * ci - t, eta * ci + t)
    F = np.where(t2 < 0, 1.0, 0.5 * (rs * rs + rp * rp))
    return (F, rs, rp) if amplitudes else F


def gtr2(h, ax, ay):
    """Anisotropic GGX ([B12] B.2 with gamma = 2; h in the local frame) and kappa against an error of a component."""
    den = (h[..., 0] / ax) ** 2 + (h[..., 1] / ay) ** 2 + h[..., 2] ** 2
    kappa = 2.0 * (2 * np.abs(h[..., 0]) / ax ** 2 + 2 * np.abs(h[..., 1]) / ay ** 2 + 2 * np.abs(h[..., 2])) / den
    return 1.0 / (np.pi * ax * ay * den * den), kappa


def gtr1(hz, a):
    """[B12] B.2 with gamma = 1: (a^2 - 1) / (pi ln(a^2) (1 + (a^2 - 1) hz^2))."""
    a2 = a * a
    den = 1.0 + (a2 - 1.0) * hz * hz
    return (a2 - 1.0) / (np.pi * np.log(a2) * den), 2.0 * np.abs(hz) * (1.0 - a2) / den


def smith_g1(w, ax, ay):
    """1 / (1 + Lambda) of an anisotropic GGX ([H14] eq. 86; w in the local frame), and kappa."""
    num = (w[..., 0] * ax) ** 2 + (w[..., 1] * ay) ** 2
    wz2 = w[..., 2] ** 2
    v = _safe_div(num, wz2)
    s = np.sqrt(1.0 + v)
    dv = _safe_div(2 * (np.abs(w[..., 0]) * ax * ax + np.abs(w[..., 1]) * ay * ay), wz2) + _safe_div(2 * v, np.abs(w[..., 2]))
    return 2.0 / (1.0 + s), dv / (2.0 * s * (1.0 + s))


def alphas(roughness, anisotropic, regularize):
    """[B12] 5.4 / B.2: aspect = sqrt(1 - 0.9 anisotropic), alpha = roughness^2 / aspect and * aspect; the roughness
    clamped to [0.01, 1], alpha at least 1e-4; path regularisation doubles an alpha below 0.1 into [0.03, 0.1]."""
    aspect = np.sqrt(1.0 - f32(0.9) * anisotropic)
    r = min(max(roughness, f32(ROUGHNESS_MIN)), 1.0)
    ax, ay = max(f32(ALPHA_MIN), r * r / aspect), max(f32(ALPHA_MIN), r * r * aspect)
    return regularized(ax, regularize), regularized(ay, regularize)


def regularized(alpha, regularize):
    if regularize and alpha < f32(REG_THRESHOLD):
        return min(max(2.0 * alpha, f32(REG_MIN)), f32(REG_MAX))
    return alpha


def clearcoat_alpha(gloss, regularize):
    """[B12] 5.6: the clearcoat's GTR1 roughness, lerp(0.1, 0.001, gloss)."""
    return regularized((1.0 - gloss) * f32(0.1) + gloss * f32(0.001), regularize)


def lobe_weights(p):
    """The weights of the four sampled lobes (diffuse, clearcoat, metal, glass), normalised: the lobe-choice
    probabilities.  Sheen rides on the diffuse samples."""
    m, st = p["metallic"], p["spec_trans"]
    w = np.array([(1 - m) * (1 - st), 0.25 * p["clearcoat"], 1 - st * (1 - m), (1 - m) * st])
    return w / w.sum()


def _tint(base):
    lum = dot(base, LUMINANCE)
    return np.where(lum[..., None] > 0, _safe_div(base, lum[..., None]), 1.0)         # C_tint = 1 for a black base


# ------------------------------------------------------------------------------------------------- Principled
def principled(win, wo, frame, n_g, base, params, regularize=False, lobes=False, eps_in=EPS_IN):
    """f (with the cosine of wo, [N, 3]), pdf [N] of the Principled BSDF and a bound for each.

    frame = (tangent, bitangent, n_s) of the hit, n_g its geometric normal, base the base colour [3] or [N, 3],
    params the material's numbers (PARAM_DEFAULTS).  Returns a dict: f, pdf, f_bound, pdf_bound, undecided (items
    that have no answer: |win + wo| or |win + eta wo| below 1e-3, or wo within the bound of the geometric horizon),
    zero_f / zero_pdf (items where the side tests make f / pdf exactly 0).  eps_in: the absolute error of the float32
    inputs, per item where the carrier's geometry amplifies it (a hit point on a curved surface at grazing incidence)."""
    e_in = np.asarray(eps_in, D)
    p = dict(PARAM_DEFAULTS)
    p.update(params)
    p = {k: f32(v) for k, v in p.items()}
    win, wo, n_g = np.asarray(win, D), np.asarray(wo, D), np.asarray(n_g, D)
    t, b, n = (np.asarray(a, D) for a in frame)
    base = np.broadcast_to(np.asarray(base, D), wo.shape)
    # the frame is turned when the shading and the geometric normal disagree about the side win is on
    flip = np.where(dot(n, win) * dot(n_g, win) < 0, -1.0, 1.0)[..., None]
    t, b, n = t * flip, b * flip, n * flip
    li = np.stack([dot(win, t), dot(win, b), dot(win, n)], -1)
    lo = np.stack([dot(wo, t), dot(wo, b), dot(wo, n)], -1)
    ig, og = dot(n_g, win), dot(n_g, wo)
    above_i, above_o = ig >= 0, og >= 0
    m, st = p["metallic"], p["spec_trans"]
    ax, ay = alphas(p["roughness"], p["anisotropic"], regularize)

    sum_r = win + wo
    len_r = np.linalg.norm(sum_r, axis=-1)
    h = _safe_div(sum_r, len_r[..., None])
    hk_r = np.maximum(1.0, _safe_div(2.0, len_r))                 # error of a component of h per error of an input
    lh = np.stack([dot(h, t), dot(h, b), dot(h, n)], -1)
    h_wo = dot(h, wo)
    g_in, k_gin = smith_g1(li, ax, ay)
    g_out, k_gout = smith_g1(lo, ax, ay)
    k_nin = _safe_div(1.0, np.abs(li[..., 2]))
    cos_o, cos_i = np.maximum(lo[..., 2], 0.0), np.maximum(li[..., 2], 0.0)
    ho = np.maximum(h_wo, 0.0)
    both_above = above_i & above_o

    out = {}                                                     # lobe -> (weight, value [N, 3] or [N], relative bound)

    # ---- diffuse: [B12] eq. 4 with the UNCLAMPED roughness (Q14), blended with [B15]'s subsurface form
    rough = p["roughness"]

    def fd(c, f90):
        return 1.0 + (f90 - 1.0) * schlick_weight(c)

    def k_fd(c, f90, df90):                                       # relative error of fd per unit input error
        return _safe_div(np.abs(f90 - 1.0) * 5 * (1 - c) ** 4 + schlick_weight(c) * df90, np.abs(fd(c, f90)))
    fd90 = 0.5 + 2.0 * rough * ho * ho
    dfd90 = 4.0 * rough * ho * hk_r
    base_diffuse = (fd(cos_i, fd90) * fd(cos_o, fd90) * cos_o / np.pi)[..., None] * base
    r_bd = k_fd(cos_i, fd90, dfd90) + k_fd(cos_o, fd90, dfd90)
    fss90 = rough * ho * ho
    dfss90 = 2.0 * rough * ho * hk_r
    inv = _safe_div(1.0, cos_o + cos_i)
    fdd = fd(cos_i, fss90) * fd(cos_o, fss90)
    bracket = fdd * (inv - 0.5) + 0.5
    d_bracket = fdd * (k_fd(cos_i, fss90, dfss90) + k_fd(cos_o, fss90, dfss90)) * np.abs(inv - 0.5) + fdd * 2 * inv * inv
    ss_diffuse = (1.25 / np.pi * bracket * cos_o)[..., None] * base
    r_ss = _safe_div(d_bracket, np.abs(bracket))
    w_diff = (1 - st) * (1 - m)
    ss = p["subsurface"]
    out["diffuse"] = (w_diff * (1 - ss), np.where(both_above[..., None], base_diffuse, 0.0), r_bd)
    out["subsurface"] = (w_diff * ss, np.where(both_above[..., None], ss_diffuse, 0.0), r_ss)
    pdf_diff = np.where(both_above, cos_o / np.pi, 0.0)
    # the cosine of wo is a CLAMPED factor of these three lobes and of the diffuse pdf: its error enters absolutely,
    # e_in times the rest of the term, also where the model's cosine is clamped to 0 and the float32 one is not
    per_cos = both_above * ((w_diff * (1 - ss) * fd(cos_i, fd90) * fd(cos_o, fd90) / np.pi
                             + w_diff * ss * 1.25 / np.pi * bracket) * base.max(-1))

    # ---- sheen: [B12] 5.4, tinted towards the base colour's hue
    c_tint = _tint(base)
    c_sheen = (1.0 - p["sheen_tint"]) + p["sheen_tint"] * c_tint
    sheen = c_sheen * (schlick_weight(ho) * cos_o)[..., None]
    r_sheen = _safe_div(5.0 * hk_r, 1.0 - ho)
    out["sheen"] = ((1 - m) * p["sheen"], np.where(both_above[..., None], sheen, 0.0), r_sheen)
    per_cos = per_cos + both_above * (1 - m) * p["sheen"] * c_sheen.max(-1) * schlick_weight(ho)

    # ---- clearcoat: [B12] 5.6; Schlick on |h.wo| with F0 of ior 1.5, GTR1, Smith G at alpha 0.25
    a_g = clearcoat_alpha(p["clearcoat_gloss"], regularize)
    r0_c = f32(0.04)
    h_wo_abs = np.abs(h_wo)
    f_c = r0_c + (1.0 - r0_c) * schlick_weight(h_wo_abs)
    k_fc = hk_r * 5 * (1 - h_wo_abs) ** 4 * (1 - r0_c) / f_c
    d_c, k_dc = gtr1(lh[..., 2], a_g)
    k_dc = k_dc * hk_r
    gc_in, k_gci = smith_g1(li, 0.25, 0.25)
    gc_out, k_gco = smith_g1(lo, 0.25, 0.25)
    cc = f_c * d_c * gc_in * gc_out * _safe_div(1.0, 4.0 * np.abs(li[..., 2]))
    r_cc = k_fc + k_dc + k_gci + k_gco + k_nin
    out["clearcoat"] = (0.25 * p["clearcoat"], np.where(both_above, cc, 0.0)[..., None] * np.ones(3), r_cc)
    pdf_cc = np.where(both_above, d_c * np.abs(lh[..., 2]) * _safe_div(1.0, 4.0 * h_wo_abs), 0.0)
    r_pcc = k_dc + hk_r * _safe_div(1.0, np.abs(lh[..., 2])) + hk_r * _safe_div(1.0, h_wo_abs)

    # ---- metal: F D G / (4 |n.wi|) with the cosine of wo cancelled; Schlick on the SIGNED h.wo (Q14) from
    # C0 = specular R0(eta) (1 - metallic) K_s + metallic base  ([B15] 3.1's achromatic specular, tinted)
    k_s = (1.0 - p["spec_tint"]) + p["spec_tint"] * c_tint
    r0 = (p["eta"] - 1.0) ** 2 / (p["eta"] + 1.0) ** 2
    c0 = p["specular"] * r0 * (1 - m) * k_s + m * base
    f_m = c0 + (1.0 - c0) * schlick_weight(h_wo)[..., None]
    k_fm = (hk_r * 5 * (1 - h_wo) ** 4)[..., None] * _safe_div(np.abs(1.0 - c0), np.abs(f_m))
    d_m, k_dm = gtr2(lh, ax, ay)
    k_dm = k_dm * hk_r
    dmd = d_m * _safe_div(1.0, 4.0 * np.abs(li[..., 2]))
    metal = f_m * (g_in * g_out * dmd)[..., None]
    r_metal = k_fm.max(-1) + k_dm + k_gin + k_gout + k_nin
    out["metal"] = (1 - st * (1 - m), np.where(both_above[..., None], metal, 0.0), r_metal)
    pdf_metal = np.where(both_above, g_in * dmd, 0.0)            # [H14] eq. 16 over the reflection Jacobian 4 (h.wi)
    r_pmetal = k_dm + k_gin + k_nin

    # ---- glass: [W07]; from below the geometric normal eta is inverted
    eta = np.where(above_i, p["eta"], 1.0 / p["eta"])
    reflect = ig * og >= 0
    sum_t = win + wo * eta[..., None]
    len_t = np.linalg.norm(sum_t, axis=-1)
    hk_t = np.maximum(1.0, _safe_div(1.0 + eta, len_t))
    hg = np.where(reflect[..., None], h, _safe_div(sum_t, len_t[..., None]))           # [W07] eq. 16
    hk_g = np.where(reflect, hk_r, hk_t)
    lhg = np.stack([dot(hg, t), dot(hg, b), dot(hg, n)], -1)
    h_in, h_out = dot(hg, win), dot(hg, wo)
    fr, rs, rp = fresnel_dielectric(h_in, eta, amplitudes=True)
    dc = e_in * hk_g
    # the two amplitudes are quotients of float32 numbers, 4 ulp of 1 each: F = (rs^2 + rp^2) / 2 keeps an absolute
    # error of (|rs| + |rp|) 4 ulp + (4 ulp)^2 however small it is (eta = 1: F is 0, its float32 value is not)
    # ... and cos^2(theta_t) = 1 - (1 - c^2) / eta^2 is a difference of numbers of size 1 and 1 / eta^2: an absolute
    # error of 2 ulp of the larger before the square root, which the root divides by 2 cos(theta_t)
    d_t2 = 2 * EPS * np.maximum(1.0, 1.0 / (eta * eta))
    d_fr = np.maximum(np.abs(fresnel_dielectric(h_in + dc, eta) - fr), np.abs(fresnel_dielectric(h_in - dc, eta) - fr)) \
        + np.maximum(np.abs(fresnel_dielectric(h_in, eta, t2_shift=d_t2) - fr), np.abs(fresnel_dielectric(h_in, eta, t2_shift=-d_t2) - fr)) \
        + (np.abs(rs) + np.abs(rp)) * 4 * EPS + (4 * EPS) ** 2
    d_g, k_dg = gtr2(lhg, ax, ay)
    k_dg = k_dg * hk_g
    inv_nin = _safe_div(1.0, np.abs(li[..., 2]))
    refl_core = d_g * inv_nin / 4.0
    glass_r = base * (fr * g_in * g_out * refl_core)[..., None]
    pdf_gr = fr * g_in * refl_core
    sd = h_in + eta * h_out                                       # = |win + eta wo| up to the sign of h
    inv_sd2 = _safe_div(1.0, sd * sd)
    trans_rest = d_g * np.abs(h_out * h_in) * inv_nin * inv_sd2
    trans_core = (1.0 - fr) * trans_rest
    glass_t = np.sqrt(base) * (trans_core * g_in * g_out)[..., None]                      # [B15]: sqrt(base) per crossing
    pdf_gt = trans_core * g_in * eta * eta                        # [H14] eq. 16 times [W07] eq. 17
    # the transmitted term's own factors: |h.wo| |h.wi| / (h.wi + eta h.wo)^2.  F's error enters absolutely, below
    r_gt_extra = hk_g * (_safe_div(1.0, np.abs(h_out)) + _safe_div(1.0, np.abs(h_in)) + 2.0 * _safe_div(1.0, np.abs(sd)))
    r_g_common = k_dg + k_gin + k_nin
    glass = np.where(reflect[..., None], glass_r, glass_t)
    r_glass = r_g_common + k_gout + np.where(reflect, 0.0, r_gt_extra)
    pdf_glass = np.where(reflect, pdf_gr, pdf_gt)
    r_pglass = r_g_common + np.where(reflect, 0.0, r_gt_extra)
    out["glass"] = ((1 - m) * st, glass, r_glass)
    # F and 1 - F: |dF| times everything else of the term
    dF_f = d_fr * np.where(reflect, base.max(-1) * g_in * g_out * refl_core,
                           np.sqrt(base.max(-1)) * trans_rest * g_in * g_out)
    dF_pdf = d_fr * np.where(reflect, g_in * refl_core, trans_rest * g_in * eta * eta)

    choose = lobe_weights(p)
    f = sum(w * v for w, v, _ in out.values())

    def scaled(value, r):                                        # value * (relative bound), 0 where the value is 0
        return np.where(value > 0, value * (TOL + e_in * np.where(value > 0, r, 0.0)), 0.0)
    f_bound = sum(scaled(np.abs(w * v).max(-1), r) for w, v, r in out.values()) + out["glass"][0] * dF_f + e_in * per_cos
    pdf_terms = [(choose[0], pdf_diff, 0.0), (choose[1], pdf_cc, r_pcc), (choose[2], pdf_metal, r_pmetal),
                 (choose[3], pdf_glass, r_pglass)]
    pdf = sum(c * v for c, v, _ in pdf_terms)
    pdf_bound = sum(scaled(c * v, r) for c, v, r in pdf_terms) + choose[3] * dF_pdf + e_in * choose[0] * both_above / np.pi
    # below the geometric normal: the glass lobe alone, its pdf NOT weighted by the lobe choice (the sampler has
    # no choice there either)
    below = ~above_i
    w_g = out["glass"][0]
    f = np.where(below[..., None], w_g * glass, f)
    f_bound = np.where(below, scaled(np.abs(w_g * glass).max(-1), r_glass) + w_g * dF_f, f_bound)
    pdf = np.where(below, pdf_glass, pdf)
    pdf_bound = np.where(below, scaled(pdf_glass, r_pglass) + dF_pdf, pdf_bound)
    undecided = (len_r < 1e-3) | (len_t < 1e-3) | (np.abs(og) <= 4 * e_in) | (np.abs(ig) <= 4 * e_in)
    # where the side tests alone make the answer exactly 0: no glass and wo across the surface (f and pdf); no
    # glass and win below (f only: the pdf there is the glass lobe's, whatever its weight)
    no_glass = w_g == 0
    zero_pdf = above_i & ~above_o & no_glass & ~undecided
    zero_f = (zero_pdf | (below & no_glass)) & ~undecided
    # a transmitted pair is possible when its half-vector, turned to the frame's upper side, has each direction on the
    # side of it that the direction has of the surface ([W07] eq. 16 with its sign rule); the pdf does not test it (Q18)
    res = dict(f=f, pdf=pdf, f_bound=f_bound, pdf_bound=pdf_bound, undecided=undecided, zero_f=zero_f, zero_pdf=zero_pdf,
               reflect=reflect, eta=eta, possible_transmission=(h_in * np.sign(lhg[..., 2]) * li[..., 2] > 0) & (h_out * np.sign(lhg[..., 2]) * lo[..., 2] > 0))
    if lobes:
        res["lobes"] = {k: w * v for k, (w, v, _) in out.items()}
        res["lobe_pdfs"] = dict(diffuse=pdf_diff, clearcoat=pdf_cc, metal=pdf_metal, glass=pdf_glass)
    return res


# ------------------------------------------------------------------------------------------------- Lambertian
def lambertian(wo, n_s, albedo):
    """f = albedo max(0, n_s.wo) / pi, pdf = max(0, n_s.wo) / pi, with the shading normal as the hit reports it
    (not turned towards the ray: a Lambertian seen from behind still evaluates against n_s); bounds 32 ulp of 1 / pi."""
    c = np.maximum(dot(wo, n_s), 0.0) / np.pi
    a = np.asarray(albedo, D)
    return dict(f=c[..., None] * a, pdf=c, f_bound=np.full(c.shape, TOL * a.max() / np.pi), pdf_bound=np.full(c.shape, TOL / np.pi))


# ------------------------------------------------------------------------------------------------- dielectric
def dielectric(win, n_s, ior):
    """The smooth dielectric of [dG06] at shading normal n_s for a ray that came from `win` (its direction is -win).
    Returns the mirror and the Snell direction, the probability of reflection - Schlick [S94] on cos(theta_i) from
    outside, on cos(theta_t) from inside, 1 beyond the critical angle - the eta it reports (ior from outside, 1 / ior
    from inside), cos(theta_t) and whether refraction exists."""
    d, n_s = -np.asarray(win, D), np.asarray(n_s, D)
    ior = f32(ior)
    front = dot(d, n_s) < 0
    n = np.where(front[..., None], n_s, -n_s)
    cos_i = -dot(d, n)
    k = np.where(front, 1.0 / ior, ior)                           # n_i / n_t
    sin2_t = k * k * (1.0 - cos_i * cos_i)
    tir = sin2_t > 1.0
    cos_t = np.sqrt(np.maximum(1.0 - sin2_t, 0.0))
    mirror = d + 2.0 * cos_i[..., None] * n
    snell = k[..., None] * d + (k * cos_i - cos_t)[..., None] * n
    r0 = ((1.0 - ior) / (1.0 + ior)) ** 2
    p_reflect = np.where(tir, 1.0, r0 + (1.0 - r0) * schlick_weight(np.where(front, cos_i, cos_t)))
    return dict(mirror=mirror, snell=snell, p_reflect=p_reflect, eta=np.where(front, ior, 1.0 / ior), cos_t=cos_t,
                cos_i=cos_i, tir=tir, front=front)


# ------------------------------------------------------------------------------------------------- lights
def one_sided_le(emit, n_light, wi):
    """A diffuse emitter radiates from the side its normal points to: Le = emit where n.wi < 0 (wi runs from the
    shaded point TO the light), 0 from the back."""
    return np.where((dot(n_light, wi) < 0)[..., None], np.asarray(emit, D), 0.0)


def sphere_light(p_from, centre, radius, q):
    """What the sphere-light sampler must report for a point q ON the sphere seen from p_from: wi, dist,
    G = |n.wi| / dist^2, the AREA-measure pdf it claims - 1 / (4 pi R^2) from inside; from outside the uniform-cone
    density 1 / (2 pi (1 - cos theta_max)), sin(theta_max) = R / d, times G - the light's outward normal at q, and
    for the outside case the cosine of q's polar angle about the centre -> p_from axis with the cap's limit: the
    sampler draws q's DIRECTION FROM THE CENTRE uniformly in a cap of half-angle theta_max about that axis (Q16), which
    is not the visible cap (half-angle acos(R / d)) and not uniform in solid angle from p_from."""
    p_from, centre, q = np.asarray(p_from, D), np.asarray(centre, D), np.asarray(q, D)
    radius = f32(radius)
    to_q = q - p_from
    dist = np.linalg.norm(to_q, axis=-1)
    wi = to_q / dist[..., None]
    n = unit(q - centre)
    G = np.abs(dot(n, wi)) / (dist * dist)
    d2 = dot(p_from - centre, p_from - centre)
    inside = d2 <= radius * radius
    with np.errstate(invalid="ignore", divide="ignore"):
        cos_max = np.sqrt(np.maximum(1.0 - radius * radius / d2, 0.0))
        pdf_out = G / (2.0 * np.pi * (1.0 - cos_max))
        axis = (p_from - centre) / np.sqrt(d2)[..., None]
    pdf = np.where(inside, 1.0 / (4.0 * np.pi * radius * radius), pdf_out)
    return dict(wi=wi, dist=dist, G=G, pdf=pdf, n=n, inside=inside, cos_max=cos_max, cos_cap=dot(n, axis), axis=axis)


def triangle_light(p_from, p0, p1, p2, q, normals=None):
    """For a point q on the triangle: barycentrics (u, v, w) with q = u p0 + v p1 + w p2, the distance of q from the
    plane, wi, dist, the light's normal at q (interpolated from vertex normals where the mesh has them, else the
    geometric one), G = |n.wi| / dist^2 with THAT normal, and the area pdf 1 / area."""
    p_from, q = np.asarray(p_from, D), np.asarray(q, D)
    p0, p1, p2 = (np.asarray(a, D) for a in (p0, p1, p2))
    e1, e2 = p1 - p0, p2 - p0
    nn = np.cross(e1, e2)
    area2 = np.linalg.norm(nn)
    n_geo = nn / area2
    rel = q - p0
    plane = dot(rel, n_geo)
    v = dot(np.cross(rel, e2), nn) / (area2 * area2)
    w = dot(np.cross(e1, rel), nn) / (area2 * area2)
    u = 1.0 - v - w
    if normals is not None:
        n0, n1, n2 = (np.asarray(a, D) for a in normals)
        n = unit(u[..., None] * n0 + v[..., None] * n1 + w[..., None] * n2)
    else:
        n = np.broadcast_to(n_geo, q.shape)
    to_q = q - p_from
    dist = np.linalg.norm(to_q, axis=-1)
    wi = to_q / dist[..., None]
    G = np.abs(dot(n, wi)) / (dist * dist)
    return dict(bary=np.stack([u, v, w], -1), plane=plane, wi=wi, dist=dist, n=n, G=G, pdf=np.full(dist.shape, 2.0 / area2),
                area=area2 / 2.0)


# ------------------------------------------------------------------------------------------------- quadrature
def sphere_grid(n_z, n_phi):
    """Midpoints of an equal-solid-angle (z, phi) grid over the sphere around +z: directions [n_z * n_phi, 3], weight."""
    z = (np.arange(n_z) + 0.5) / n_z * 2.0 - 1.0
    phi = (np.arange(n_phi) + 0.5) / n_phi * 2.0 * np.pi - np.pi
    Z, P = np.meshgrid(z, phi, indexing="ij")
    r = np.sqrt(1.0 - Z * Z)
    return np.stack([r * np.cos(P), r * np.sin(P), Z], -1).reshape(-1, 3), 4.0 * np.pi / (n_z * n_phi)


def integrate_sphere(fn, n0=64, rel=1e-4, n_max=2048):
    """Integral of fn(directions) over the sphere (midpoint rule in (z, phi)), the grid doubled until the result moves
    by less than `rel` relative (of the largest component); returns (value, the last change: the stated error)."""
    prev, n = None, n0
    while True:
        dirs, wgt = sphere_grid(n, 2 * n)
        val = np.asarray(fn(dirs)).sum(0) * wgt
        if prev is not None:
            err = np.abs(val - prev).max()
            if err <= rel * max(np.abs(val).max(), 1e-300) or n >= n_max:
                return val, err
        prev, n = val, n * 2
