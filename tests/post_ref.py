"""A float64 model of the post chain and of the two 8-bit decodes, written from the publications, and the rule by
which a backend's bytes are compared with it.  TEST INFRASTRUCTURE ONLY.

Plain numpy float64 with the published decimal constants; nothing here is float32 and nothing is imported from the
oracle.  The chain is  tone-mapping operator -> sRGB OETF -> quantiser:

  sRGB OETF      IEC 61966-2-1: 12.92 x below 0.0031308, 1.055 x^(1/2.4) - 0.055 from there on, x clamped to [0, 1]
  clamp          x clamped to [0, 1]
  AgX            the minimal AgX implementation (iolite-engine.com/blog_posts/minimal_agx_implementation, after
                 github.com/sobotka/AgX): inset matrix, log2 encoding between -12.47393 and 4.026069 EV, the 6th-order
                 polynomial of the default contrast, the identity look (slope 1, offset 0, power 1, saturation 1),
                 outset matrix, negative values to 0, the display's 2.2 power.  Its matrices are printed in GLSL's
                 column order: three numbers are one COLUMN
  Reinhard       Reinhard et al. 2002, eq. 4, on luminance: L_d = L (1 + L / L_w^2) / (1 + L), the colour scaled by
                 L_d / L, with L_w the largest positive non-NaN luminance of the frame
  ACES           Stephen Hill's fit (BakingLab ACES.hlsl): ACESInputMat, RRTAndODTFit, ACESOutputMat.  Its matrices
                 are printed in HLSL's row order: three numbers are one ROW
  quantiser      int(255.999 c), clamped to 0 ... 255

and the comparisons the reference states are part of the definition: a clamp is two comparisons, `v < lo` and
`hi < v`, which carry a NaN; Reinhard scales a colour only where `l_in > 0` and writes black otherwise; AgX's
`val < 0 -> 0`; a pixel with any NaN channel after the OETF is written as the marker (255, 0, 255).  The luminance is
the reference's, 0.212671 r + 0.715160 g + 0.072169 b.

DOMAIN.  The model answers for inputs whose float32 intermediates stay finite: |channel| <= 2^40, and beside them the
non-finite edge inputs (NaN, +inf in any channel).  Beyond that the float32 chain overflows where float64 does not:
ACES squares its input, so from about 1.8e19 on `v * v` is +inf in float32, `inf / inf` is NaN and the pixel becomes the
marker, where this model still says white.

THE RULE (`compare`).  A backend's bytes agree with the model when ALL of these hold:
  (a) no value differs by more than 1;
  (b) every value that differs has the model's q = 255.999 c within `delta` of an integer;
  (c) at most one value in a thousand differs, counted over the values whose q lies strictly inside (0, 255.999):
      saturated and black values never differ and would only dilute the share.  A cap, not a measurement.
`delta` is per operator: 4 x the float32 chain's worst deviation from this model in byte units, measured on the CPU
against the oracle's floats (POST_MEASURED in tests/test_post_known_answers.py), never against a kernel.
What 8 bits can show: a change of the model that moves c by much less than delta / 255.999 changes few bytes, all in
band, and passes - the last digit of an ACES constant (0.4329510 -> 0.43295) is such a change and is NOT seen.

The 8-bit decodes: `srgb_eotf8` is the sRGB EOTF of b / 255 (b / 255 / 12.92 up to 0.04045, ((x + 0.055) / 1.055)^2.4
above), `normal8` is normalize(((r, g) / 127.5 - 1) * scale, b / 127.5 - 1)."""
import numpy as np

LUMINANCE = (0.212671, 0.715160, 0.072169)

# every constant a perturbed model may replace (the mutants of test_post_known_answers.py); `post` reads no other
PUBLISHED = dict(
    oetf_threshold=0.0031308,
    quantiser=255.999,
    luminance=LUMINANCE,
    # AgX, columns as printed
    agx_inset_columns=((0.842479062253094, 0.0423282422610123, 0.0423756549057051),
                       (0.0784335999999992, 0.878468636469772, 0.0784336),
                       (0.0792237451477643, 0.0791661274605434, 0.879142973793104)),
    agx_outset_columns=((1.19687900512017, -0.0528968517574562, -0.0529716355144438),
                        (-0.0980208811401368, 1.15190312990417, -0.0980434501171241),
                        (-0.0990297440797205, -0.0989611768448433, 1.15107367264116)),
    agx_min_ev=-12.47393,
    agx_max_ev=4.026069,
    agx_contrast=(15.5, -40.14, 31.96, -6.868, 0.4298, 0.1191, -0.00232),     # x^6 ... x^0
    agx_power=2.2,
    # ACES, rows as printed
    aces_input_rows=((0.59719, 0.35458, 0.04823), (0.07600, 0.90834, 0.01566), (0.02840, 0.13383, 0.83777)),
    aces_output_rows=((1.60475, -0.53108, -0.07367), (-0.10208, 1.10813, -0.00605), (-0.00327, -0.07276, 1.07602)),
    aces_fit=(0.0245786, 0.000090537, 0.983729, 0.4329510, 0.238081),
    reinhard_white_power=2,
)

CLAMP, AGX, REINHARD, ACES = 0, 1, 2, 3
OPERATORS = {CLAMP: "clamp", AGX: "agx", REINHARD: "reinhard", ACES: "aces"}


def clamp(v, lo, hi):
    """`v < lo ? lo : hi < v ? hi : v`: a NaN fails both comparisons and is carried."""
    with np.errstate(invalid="ignore"):
        return np.where(v < lo, lo, np.where(hi < v, hi, v))


def luminance(rgb, k=PUBLISHED):
    w = k["luminance"]
    return rgb[..., 0] * w[0] + rgb[..., 1] * w[1] + rgb[..., 2] * w[2]


def _rows(m, v):
    """m v for a matrix given by its rows."""
    m = np.asarray(m, np.float64)
    return np.stack([m[i, 0] * v[..., 0] + m[i, 1] * v[..., 1] + m[i, 2] * v[..., 2] for i in range(3)], -1)


def srgb_oetf(x, k=PUBLISHED):
    x = clamp(x, 0.0, 1.0)
    with np.errstate(invalid="ignore"):
        return np.where(x < k["oetf_threshold"], 12.92 * x, 1.055 * np.power(x, 1 / 2.4) - 0.055)


def agx(v, k=PUBLISHED):
    with np.errstate(all="ignore"):
        v = _rows(np.transpose(k["agx_inset_columns"]), v)
        lo, hi = k["agx_min_ev"], k["agx_max_ev"]
        v = (clamp(np.log2(v), lo, hi) - lo) / (hi - lo)
        v = np.polyval(k["agx_contrast"], v)
        luma = v[..., 0] * 0.2126 + v[..., 1] * 0.7152 + v[..., 2] * 0.0722      # the look: slope 1, offset 0, power 1 ...
        v = luma[..., None] + 1.0 * (v - luma[..., None])                        # ... saturation 1
        v = _rows(np.transpose(k["agx_outset_columns"]), v)
        v = np.where(v < 0, 0.0, v)
        return np.power(v, k["agx_power"])


def aces(v, k=PUBLISHED):
    c1, c2, c3, c4, c5 = k["aces_fit"]
    with np.errstate(all="ignore"):
        v = _rows(k["aces_input_rows"], v)
        v = (v * (v + c1) - c2) / (v * (c3 * v + c4) + c5)
        return _rows(k["aces_output_rows"], v)


def largest_luminance(rgb, k=PUBLISHED):
    """The largest positive non-NaN luminance of the frame; 0 when there is none."""
    with np.errstate(invalid="ignore"):
        lum = luminance(rgb, k)
        lum = lum[lum > 0]
    return float(lum.max()) if lum.size else 0.0


def reinhard(v, k=PUBLISHED):
    with np.errstate(all="ignore"):
        lw = largest_luminance(v, k)
        lum = luminance(v, k)
        new = lum * (1 + lum / lw ** k["reinhard_white_power"]) / (1 + lum)
        return np.where((lum > 0)[..., None], v * (new / lum)[..., None], 0.0)


def post(rgb, tonemapper, k=PUBLISHED):
    """(q, rgb8) of an [H, W, 3] frame: q = 255.999 c per value in float64 (NaN where c is), rgb8 the bytes, the
    marker (255, 0, 255) on every pixel with a NaN channel."""
    v = np.asarray(rgb).astype(np.float64)
    assert v.ndim == 3 and v.shape[2] == 3 and tonemapper in OPERATORS
    if tonemapper == CLAMP:
        v = clamp(v, 0.0, 1.0)
    elif tonemapper == AGX:
        v = agx(v, k)
    elif tonemapper == REINHARD:
        v = reinhard(v, k)
    else:
        v = aces(v, k)
    q = k["quantiser"] * srgb_oetf(v, k)
    marker = np.isnan(q).any(-1)
    with np.errstate(invalid="ignore"):
        rgb8 = np.clip(np.trunc(np.where(np.isnan(q), 0.0, q)), 0, 255).astype(np.uint8)
    rgb8[marker] = (255, 0, 255)
    return q, rgb8


def compare(got, q, want, delta):
    """The rule on one frame: dict(failed = "" or the clauses that reject it, differing, share, worst_band, max_diff).
    `got`: a backend's bytes, `q`, `want`: the model's."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape == q.shape and got.dtype == np.uint8
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    differs = diff != 0
    with np.errstate(invalid="ignore"):
        inside = (q > 0) & (q < 255.999)
        band = np.abs(q - np.rint(q))[differs]               # NaN where the model has the marker: never in band
    share = differs.sum() / max(int(inside.sum()), 1)
    worst = float(np.max(np.where(np.isnan(band), np.inf, band))) if band.size else 0.0
    failed = "".join(c for c, bad in (("a", diff.max() > 1), ("b", worst > delta), ("c", share > 1e-3)) if bad)
    return dict(failed=failed, differing=int(differs.sum()), share=float(share), worst_band=worst,
                max_diff=int(diff.max()))


# ---------------------------------------------------------------------------------------------- the 8-bit decodes
def srgb_eotf8():
    """The 256 linear values of the sRGB bytes."""
    x = np.arange(256, dtype=np.float64) / 255
    return np.where(x <= 0.04045, x / 12.92, np.power((x + 0.055) / 1.055, 2.4))


def normal8(rgb8, scale):
    """(unit normal [..., 3], length of the vector before it is normalised) of a normal map's bytes; `scale` is taken
    as the float32 the decodes are handed."""
    v = np.asarray(rgb8).astype(np.float64) / 127.5 - 1
    s = float(np.float32(scale))
    v = v * np.array([s, s, 1.0])
    length = np.sqrt((v * v).sum(-1))
    return v / length[..., None], length
