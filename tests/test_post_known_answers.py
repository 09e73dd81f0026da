"""Known answers for the post chain and the 8-bit decodes: `oracle_post_rgb8`, the host library's
`tonemap_to_rgb8` and the GPU's `hip.post_rgb8` against tests/post_ref.py - float64 numpy written from the published
operators (IEC 61966-2-1, Hill's ACES fit, the minimal AgX, Reinhard's extended luminance operator), not from the three
restatements of the reference's float32 chain, which share one author and one expression tree.

The rule (post_ref.compare): (a) no value off by more than 1, (b) every differing value has the model's
q = 255.999 c within delta of an integer, (c) at most 1e-3 of the unsaturated values differ.  delta is 4 x the float32
chain's worst deviation from the model in byte units, per operator, measured on the oracle's floats
(`oracle_post_float`) over the three dense frames: POST_MEASURED below, recomputed by
test_post_measured_is_still_the_oracles_deviation.  test_the_rule_rejects_perturbed_models shows which clause sees
which wrong constant; a change of the model far below delta - the last digit of an ACES constant, 0.4329510 -> 0.43295 -
moves 2e-5 of the bytes, all in band, and is NOT seen: 8 bits cannot show it.

Beside the rule the GPU's bytes are the oracle's exactly, on 80 times as many distinct values as the one render of
test_post_chain_on_gpu_is_byte_exact; Reinhard's reduction is run where its grid-stride loop takes more than two
trips, with the maximum in every place that matters; the 8-bit decodes are run past their grid cap of 65 536 blocks.
Frames are at most 512 x 256 but for the 1021 x 517 reduction frames and the two decode calls of 2^24 + 1 items."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import post_ref as M
import vimg_amd
from vimg_amd import host

BACKENDS = [pytest.param("oracle", id="oracle"), pytest.param("host", id="host"),
            pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
DECODERS = [pytest.param("host", id="host"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
OPERATORS = list(M.OPERATORS)
U = 2.0 ** -24                     # unit roundoff of float32

# max |c_oracle - c_model| after the OETF over the three dense frames below (3 x 2^16 pixels), by operator, rounded up
# in the third digit.  Measured 2026-10-21 with
#   python -m pytest tests/test_post_known_answers.py -k post_measured -s
POST_MEASURED = {M.CLAMP: 1.45e-7, M.AGX: 6.97e-6, M.REINHARD: 2.36e-7, M.ACES: 7.93e-7}
DELTA = {tm: 4 * 255.999 * dev for tm, dev in POST_MEASURED.items()}


def post(kind, frame, tonemapper):
    """The bytes of one backend for an [H, W, 3] float32 numpy frame."""
    assert frame.dtype == np.float32
    if kind == "oracle":
        return O.post_rgb8(frame, tonemapper)
    if kind == "host":
        return vimg_amd.tonemap_to_rgb8(frame, tonemapper)
    from vimg_amd import hip
    out = hip.post_rgb8(frame, tonemapper)              # numpy in, numpy out
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == frame.shape
    return out


# ------------------------------------------------------------------------------------------------------ the frames
@functools.lru_cache(maxsize=None)
def dense_frames():
    """name -> [128, 512, 3] float32, 2^16 pixels each: a grey ramp 2^-20 ... 2^10, log-uniform colours 2^-14 ... 2^6,
    and those colours with 40 % of the channels zeroed."""
    n = 1 << 16
    rng = np.random.default_rng(20261021)
    ramp = np.repeat(np.exp2(np.linspace(-20.0, 10.0, n))[:, None], 3, 1)
    colours = np.exp2(rng.uniform(-14.0, 6.0, (n, 3)))
    sparse = np.where(rng.random((n, 3)) < 0.4, 0.0, colours)
    frames = {"ramp": ramp, "colours": colours, "sparse": sparse}
    return {k: np.ascontiguousarray(v.reshape(128, 512, 3), np.float32) for k, v in frames.items()}


EDGE_IN_DOMAIN = 18        # the first pixels of the edge frame: the model answers for them
FLT_MAX = float(np.finfo(np.float32).max)


@functools.lru_cache(maxsize=None)
def edge_frame():
    """One row: 0; -0; negatives in one and in all channels; denormals; NaN in each single channel; +inf in one and
    in three channels; ordinary colours beside them; 2^40 - then, past the model's domain, 1e19, 2e19, 1e30, FLT_MAX."""
    nan, inf = float("nan"), float("inf")
    px = [(0, 0, 0), (-0.0, -0.0, -0.0), (-0.5, 0.3, 0.2), (0.3, -0.5, 0.2), (0.3, 0.2, -7.0), (-1, -2, -3),
          (1e-40, 1e-40, 1e-40), (1.4e-45, 0, 1e-39), (nan, 0.5, 0.5), (0.5, nan, 0.5), (0.5, 0.5, nan),
          (inf, 0.5, 0.5), (0.5, inf, 0.5), (inf, inf, inf), (0.18, 0.18, 0.18), (0.9, 0.06, 0.35), (3.0, 7.0, 0.01),
          (2.0 ** 40,) * 3,
          (1e19,) * 3, (2e19,) * 3, (1e30,) * 3, (FLT_MAX,) * 3]
    assert len(px) == EDGE_IN_DOMAIN + 4
    return np.array(px, np.float32).reshape(1, len(px), 3)


REDUCTION_SHAPE = (517, 1021)          # 527 857 pixels: more than two trips of 1024 x 256 threads, n % 64 = 49
BRIGHT_AT = (0, 262143, 262144, 524288, 517 * 1021 - 1)


@functools.lru_cache(maxsize=None)
def reduction_base():
    """Colours up to 4 in every channel (largest luminance just below 4)."""
    rng = np.random.default_rng(517)
    return rng.uniform(0.0, 4.0, REDUCTION_SHAPE + (3,)).astype(np.float32)


def reduction_frame(pixels):
    """The base frame with `pixels` = ((flat index, (r, g, b)), ...) written into it."""
    f = reduction_base().copy()
    flat = f.reshape(-1, 3)
    for at, rgb in pixels:
        flat[at] = rgb
    return f


@functools.lru_cache(maxsize=None)
def model(name, tonemapper):
    """(q, bytes) of the model, computed once per frame and operator and shared by the backends."""
    if name in dense_frames():
        frame = dense_frames()[name]
    elif name == "edge":
        frame = edge_frame()
    elif name == "reduction base":
        frame = reduction_base()
    else:
        kind, at = name
        assert kind == "bright"
        frame = reduction_frame([(at, (50.0, 50.0, 50.0))])
    q, b = M.post(frame, tonemapper)
    q.setflags(write=False), b.setflags(write=False)
    return q, b


@functools.lru_cache(maxsize=None)
def oracle_bytes(name, tonemapper):
    frame = dense_frames()[name] if name in dense_frames() else edge_frame()
    b = O.post_rgb8(frame, tonemapper)
    b.setflags(write=False)
    return b


def agrees(got, q, want, tonemapper, label):
    r = M.compare(got, q, want, DELTA[tonemapper])
    print(f"{label}: {r['differing']} values differ (share {r['share']:.2e}), worst in-band distance "
          f"{r['worst_band']:.2e} of delta {DELTA[tonemapper]:.2e}, largest difference {r['max_diff']}")
    assert r["failed"] == "", (label, r)
    return r


# ------------------------------------------------------------------------------------- delta, and the rule's teeth
def measure_deviation(tonemapper):
    """max |c_oracle - c_model| over the dense frames, with the frame and value it is at."""
    worst = (0.0, None)
    for name, frame in dense_frames().items():
        q, _ = model(name, tonemapper)
        c = O.post_float(frame, tonemapper).astype(np.float64)
        assert not np.isnan(c).any() and not np.isnan(q).any()
        d = np.abs(c - q / 255.999)
        at = np.unravel_index(np.argmax(d), d.shape)
        if d[at] > worst[0]:
            worst = (float(d[at]), (name, frame[at[:2]].tolist()))
    return worst


def test_post_measured_is_still_the_oracles_deviation():
    """POST_MEASURED is the oracle's float chain against the model, not a number of its own: recomputed here, and
    the oracle's floats quantise to the oracle's bytes (the two entry points share one body)."""
    for tm in OPERATORS:
        dev, where = measure_deviation(tm)
        print(f"{M.OPERATORS[tm]}: max |c_oracle - c_model| = {dev:.4e} at {where}; recorded {POST_MEASURED[tm]:.3e}, "
              f"delta = {DELTA[tm]:.3e} byte units")
        assert dev <= POST_MEASURED[tm]
        assert dev >= POST_MEASURED[tm] / 2, "the recorded figure is stale: measure it again"
        for name, frame in dense_frames().items():
            c = O.post_float(frame, tm).astype(np.float64)
            assert np.array_equal(np.clip((255.999 * c).astype(np.int64), 0, 255), oracle_bytes(name, tm))


def _swap(key):
    return {key: tuple(zip(*M.PUBLISHED[key]))}


MUTANTS = {
    "OETF threshold 0.04045": dict(oetf_threshold=0.04045),
    "quantiser 255.0": dict(quantiser=255.0),
    "quantiser 256.0": dict(quantiser=256.0),
    "AgX without its 2.2 power": dict(agx_power=1.0),
    "AgX inset transposed": _swap("agx_inset_columns"),
    "AgX outset transposed": _swap("agx_outset_columns"),
    "ACES input matrix transposed": _swap("aces_input_rows"),
    "ACES output matrix transposed": _swap("aces_output_rows"),
    "Reinhard L / Lw": dict(reinhard_white_power=1),
    "Rec. 601 luminance": dict(luminance=(0.299, 0.587, 0.114)),
    "AgX contrast 40.14 -> 40.1": dict(agx_contrast=(15.5, -40.1, 31.96, -6.868, 0.4298, 0.1191, -0.00232)),
    "AgX max_ev 4.026069 -> 4.0": dict(agx_max_ev=4.0),
}
UNSEEN = {"ACES fit 0.4329510 -> 0.43295": dict(aces_fit=(0.0245786, 0.000090537, 0.983729, 0.43295, 0.238081))}


def _caught(change):
    """operator -> the clauses that reject the ORACLE's bytes when the model is perturbed by `change`."""
    k = dict(M.PUBLISHED, **change)
    caught, shares = {}, {}
    for tm in OPERATORS:
        clauses, share = set(), 0.0
        for name, frame in dense_frames().items():
            q, want = M.post(frame, tm, k)
            r = M.compare(oracle_bytes(name, tm), q, want, DELTA[tm])
            clauses |= set(r["failed"])
            share = max(share, r["share"])
        caught[M.OPERATORS[tm]], shares[M.OPERATORS[tm]] = "".join(sorted(clauses)), share
    return caught, shares


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_rule_rejects_perturbed_models(mutant):
    """Each wrong constant, put into the MODEL and held against the oracle's bytes on the dense frames, is rejected
    under at least one operator.  `256.0` for `255.999` moves only 1e-4 of the bytes, by 1: a cap on the share alone
    passes it, clause (b) does not - those bytes lie up to 1e-3 byte units from an edge, many deltas away."""
    caught, shares = _caught(MUTANTS[mutant])
    print(f"{mutant}: rejected by clause " + ", ".join(f"{op}: {c or '-'} (share {shares[op]:.1e})" for op, c in caught.items()))
    assert any(caught.values())
    if mutant == "quantiser 256.0":
        assert any("b" in caught[op] for op in ("clamp", "reinhard", "aces"))
        assert all("c" not in c for c in caught.values())           # the share alone does not see it


def test_a_last_digit_of_an_aces_constant_is_below_what_8_bits_show():
    """Printed, not claimed: the differing share and the clauses (none expected) for a change far below delta."""
    for name, change in UNSEEN.items():
        caught, shares = _caught(change)
        print(f"{name}: " + ", ".join(f"{op}: {c or '-'} (share {shares[op]:.1e})" for op, c in caught.items()))
        assert "a" not in caught["aces"] and "c" not in caught["aces"] and shares["aces"] < 1e-4


# ------------------------------------------------------------------------------------------------------ dense frames
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("tonemapper", OPERATORS)
@pytest.mark.parametrize("name", ["ramp", "colours", "sparse"])
def test_dense_frames_agree_with_the_model(name, tonemapper, backend):
    """3 x 2^16 pixels x four operators under the rule; the host library and the GPU give the oracle's bytes exactly
    (the existing contract, "byte-exact against its oracle restatement")."""
    frame = dense_frames()[name]
    got = post(backend, frame, tonemapper)
    q, want = model(name, tonemapper)
    agrees(got, q, want, tonemapper, f"{name} {M.OPERATORS[tonemapper]} {backend}")
    if backend != "oracle":
        same = got == oracle_bytes(name, tonemapper)
        assert same.all(), (int((~same).sum()), frame[np.nonzero(~same.all(-1))][:4].tolist())


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("tonemapper", OPERATORS)
def test_grey_ramps_are_monotone(tonemapper, backend):
    got = post(backend, dense_frames()["ramp"], tonemapper).reshape(-1, 3).astype(np.int32)
    assert np.all(np.diff(got, axis=0) >= 0)
    assert got[0].max() <= 1 and got[-1].min() >= 250            # from black to (almost) white


# -------------------------------------------------------------------------------------------------------- edge frame
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("tonemapper", OPERATORS)
def test_edge_inputs(tonemapper, backend):
    """Up to 2^40 every backend gives the model's bytes EXACTLY: by the model's own q none of these values is within
    4 delta of an edge between two bytes (the integers 1 ... 255: c is clamped to [0, 1], so 0 and 256 are none).
    Past the domain, ACES from 2e19 on: v * v overflows float32, inf / inf is NaN and the
    pixel is the marker, where the model says white (Q36); every other value there still follows the model."""
    frame = edge_frame()
    got = post(backend, frame, tonemapper)
    q, want = model("edge", tonemapper)
    k = EDGE_IN_DOMAIN
    with np.errstate(invalid="ignore"):
        inside = (q[:, :k] > 0) & (q[:, :k] < 255.999)
    margin = np.abs(q[:, :k] - np.clip(np.rint(q[:, :k]), 1, 255))[inside]      # the edges between bytes: 1 ... 255
    print(f"edge {M.OPERATORS[tonemapper]} {backend}: {int(inside.sum())} unsaturated values, nearest edge "
          f"{margin.min():.2e} byte units away (delta {DELTA[tonemapper]:.2e})")
    assert margin.min() > 4 * DELTA[tonemapper]
    assert np.array_equal(got[:, :k], want[:, :k]), (got[:, :k].tolist(), want[:, :k].tolist())
    if tonemapper != M.REINHARD:              # NaN in one channel: the marker (Reinhard: l_in > 0 fails, black)
        assert np.all(got[0, 8:11] == (255, 0, 255))
    else:
        assert np.all(got[0, 8:11] == 0)
    beyond_got, beyond_want = got[0, k:], want[0, k:]             # 1e19, 2e19, 1e30, FLT_MAX
    if tonemapper == M.ACES:
        assert np.all(beyond_want == 255)                         # the published form in float64: white
        assert np.all(beyond_got[0] == 255) and np.all(beyond_got[1:] == (255, 0, 255))
    else:
        assert np.array_equal(beyond_got, beyond_want)
    assert np.array_equal(got, oracle_bytes("edge", tonemapper))


# ------------------------------------------------------------------------------------ known answers without a model
@pytest.mark.parametrize("backend", BACKENDS)
def test_srgb_round_trip_returns_every_byte(backend):
    """Decode the 256 bytes with the sRGB table, post the result with the clamp operator: the bytes come back.  The
    nearest quantisation edge is 1.0e-3 byte units away (255.999 b / 255 against b), float32 error about 6e-5."""
    b = np.arange(256, dtype=np.uint8)
    if backend == "gpu":
        from vimg_amd import hip
        linear = hip.lut8_to_float(b, host.srgb8_lut())
    else:
        linear = host.srgb8_to_linear(b)
    frame = np.ascontiguousarray(np.repeat(linear[:, None], 3, 1).reshape(1, 256, 3))
    got = post(backend, frame, M.CLAMP)
    assert np.array_equal(got, np.repeat(b[:, None], 3, 1).reshape(1, 256, 3))


@pytest.mark.parametrize("backend", BACKENDS)
def test_reinhard_brightest_grey_pixel_is_white_and_dark_frames_are_black(backend):
    rng = np.random.default_rng(3)
    f = rng.uniform(0, 2, (64, 96, 3)).astype(np.float32)
    f[41, 17] = 9.5
    assert post(backend, f, M.REINHARD)[41, 17].tolist() == [255, 255, 255]
    assert not post(backend, np.zeros((33, 65, 3), np.float32), M.REINHARD).any()
    dark = -rng.uniform(0, 2, (33, 65, 3)).astype(np.float32)
    dark[::2] = 0
    dark[5, 5] = (1.0, -1.0, 1.0)            # luminance 0.285 - 0.715 < 0
    assert not post(backend, dark, M.REINHARD).any()


# ----------------------------------------------------------------------------------------------- Reinhard's reduction
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("at", BRIGHT_AT)
def test_reinhard_finds_the_maximum_wherever_it_is(at, backend):
    """One grey pixel of 50 in a frame of values up to 4, at the first pixel, the last of the first trip of the
    grid-stride loop, the first of the second and of the third, and the last (inside the partial last wave).  Missing
    it changes most of the frame: at least half of the bytes differ from the frame without it."""
    frame = reduction_frame([(at, (50.0, 50.0, 50.0))])
    got = post(backend, frame, M.REINHARD)
    q, want = model(("bright", at), M.REINHARD)
    agrees(got, q, want, M.REINHARD, f"bright pixel at {at} {backend}")
    assert np.array_equal(got, O.post_rgb8(frame, M.REINHARD))
    without = post(backend, reduction_base(), M.REINHARD)
    changed = (got != without).mean()
    print(f"bright pixel at {at} {backend}: {changed:.3f} of the bytes differ from the frame without it")
    assert changed >= 0.5


@pytest.mark.parametrize("backend", BACKENDS)
def test_reinhard_maximum_ignores_nan_negative_and_negative_luminance(backend):
    """A NaN pixel, a large negative pixel and a pixel of negative luminance with one large channel do not win the
    maximum: every other pixel keeps the bytes of the frame without them."""
    nan = float("nan")
    planted = [(100, (nan, 1.0, 1.0)), (262144 + 77, (-900.0, -900.0, -900.0)), (517 * 1021 - 3, (0.0, -100.0, 900.0)),
               (300000, (nan, nan, nan))]
    frame = reduction_frame(planted)
    got = post(backend, frame, M.REINHARD)
    q, want = M.post(frame, M.REINHARD)
    agrees(got, q, want, M.REINHARD, f"pixels that may not win {backend}")
    assert np.array_equal(got, O.post_rgb8(frame, M.REINHARD))
    without = post(backend, reduction_base(), M.REINHARD).reshape(-1, 3)
    keep = np.ones(len(without), bool)
    keep[[at for at, _ in planted]] = False
    assert np.array_equal(got.reshape(-1, 3)[keep], without[keep])
    assert not got.reshape(-1, 3)[~keep].any()                   # l_in > 0 fails: black, no marker


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("tonemapper", OPERATORS)
@pytest.mark.parametrize("h,w", [(1, 1), (1, 63), (1, 65), (257, 1)])
def test_small_frames(h, w, tonemapper, backend):
    """Frames smaller than a wave, one lane more than a wave, and one pixel more than a block."""
    rng = np.random.default_rng(h * 1000 + w)
    frame = np.exp2(rng.uniform(-8, 3, (h, w, 3))).astype(np.float32)
    got = post(backend, frame, tonemapper)
    q, want = M.post(frame, tonemapper)
    agrees(got, q, want, tonemapper, f"{h} x {w} {M.OPERATORS[tonemapper]} {backend}")
    assert np.array_equal(got, O.post_rgb8(frame, tonemapper))


@pytest.mark.parametrize("backend", BACKENDS)
def test_reinhard_on_denormal_luminances(backend):
    """The only positive luminances are denormal (against the oracle only: Lw^2 underflows, outside the model's
    domain).  A backend that flushed denormals would find no maximum, or no positive luminance."""
    f = np.zeros((40, 100, 3), np.float32)
    f[::3] = 1e-41
    f[7, 7] = 3e-39
    f[1::3] = -1.0
    want = O.post_rgb8(f, M.REINHARD)
    assert want[0, 0].tolist() != [0, 0, 0]
    assert np.array_equal(post(backend, f, M.REINHARD), want)


@pytest.mark.parametrize("backend", BACKENDS)
def test_reinhard_calls_do_not_see_each_others_maximum(backend):
    """A bright frame, then a dim one: the second answer is the dim frame's own (the device word of the maximum is
    reset by every call); and another operator between two Reinhard calls changes nothing."""
    rng = np.random.default_rng(9)
    dim = rng.uniform(0, 0.5, (100, 300, 3)).astype(np.float32)
    bright = dim * np.float32(400)
    first = post(backend, bright, M.REINHARD)
    second = post(backend, dim, M.REINHARD)
    q, want = M.post(dim, M.REINHARD)
    agrees(second, q, want, M.REINHARD, f"dim after bright {backend}")
    assert np.array_equal(second, O.post_rgb8(dim, M.REINHARD))
    assert np.array_equal(first, O.post_rgb8(bright, M.REINHARD))
    post(backend, bright, M.ACES)
    assert np.array_equal(post(backend, dim, M.REINHARD), second)


@pytest.mark.gpu
def test_binding_takes_numpy_and_tensors_and_refuses_a_view():
    """numpy in, numpy out; a CUDA tensor in, a CUDA tensor out with the same bytes; a non-contiguous CUDA view is
    refused by the shared tensor check before the library is called."""
    import torch
    from vimg_amd import hip
    frame = dense_frames()["colours"]
    t = torch.from_numpy(frame).cuda()
    out = hip.post_rgb8(t, 1)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8
    assert np.array_equal(out.cpu().numpy(), hip.post_rgb8(frame, 1))
    with pytest.raises(ValueError, match="post_rgb8 image: the tensor must be contiguous"):
        hip.post_rgb8(t.transpose(0, 1), 1)
    with pytest.raises(ValueError, match="post_rgb8 image: dtype must be float32"):
        hip.post_rgb8(t.double(), 1)


# ---------------------------------------------------------------------------------------------------- 8-bit decodes
def test_srgb_table_is_the_float64_eotf():
    """`vimg_host_srgb8_lut` against the float64 EOTF of b / 255.  Bound, from the expression
    pow((x / 255 + 0.055f) / 1.055f, 2.4f) in units of u = 2^-24 relative: x / 255 carries u; the sum of two
    positives max(u, u of the constant) + u = 2u; the quotient + u of 1.055f + u = 4u; the power multiplies that by
    2.4 (9.6u), the rounding of 2.4f adds 2.4 |ln t| u with t >= (11 / 255 + 0.055) / 1.055 = 0.093 (5.7u), powf
    itself is within 1 ulp = 2u: 17.3u = 1.03e-6 relative.  The linear branch (x / 255 / 12.92f) has 3u.
    Measured worst / bound: 0.34 (3.5e-7 relative, at byte 134)."""
    lut = host.srgb8_lut().astype(np.float64)
    ref = M.srgb_eotf8()
    assert lut[0] == 0 and ref[0] == 0 and lut[255] == 1.0
    rel = np.abs(lut[1:] - ref[1:]) / ref[1:]
    bound = (2.4 * 4 + 2.4 * abs(np.log((11 / 255 + 0.055) / 1.055)) + 2) * U
    print(f"sRGB table: worst relative error {rel.max():.3e} at byte {1 + int(np.argmax(rel))}, bound {bound:.3e}, "
          f"worst / bound {rel.max() / bound:.3f}")
    assert rel.max() <= bound
    assert np.all(np.diff(lut) > 0)


@functools.lru_cache(maxsize=None)
def shuffled_table():
    """256 distinct floats in no order: a gather that ignored its table, or read the sRGB one, fails."""
    rng = np.random.default_rng(256)
    t = rng.permutation(np.arange(256, dtype=np.float32) * np.float32(0.37) - np.float32(11.0))
    assert len(set(t.tolist())) == 256
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 99459, 65536 * 256 + 1])
def test_lut_gather_is_exact(n):
    """`hip.lut8_to_float` is lut[vals] bit for bit.  65 536 * 256 + 1 is the smallest n at which the grid-stride
    loop takes a second trip: its one element there has a value that occurs nowhere else, and so has the last
    element of the first trip."""
    from vimg_amd import hip
    lut = shuffled_table()
    rng = np.random.default_rng(n)
    vals = rng.integers(0, 254, n, dtype=np.uint8)
    vals[-1] = 255
    if n > 2:
        vals[-2] = 254
    if n > 65536 * 256:
        assert n - 2 == 16777215
    got = hip.lut8_to_float(vals, lut)
    assert got.shape == (n,) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), lut[vals].view(np.uint32))


@functools.lru_cache(maxsize=None)
def normal_bytes():
    """Every (r, g) with b in {0, 1, 126, 127, 128, 129, 254, 255}: 524 288 pixels."""
    r, g, b = np.meshgrid(np.arange(256), np.arange(256), [0, 1, 126, 127, 128, 129, 254, 255], indexing="ij")
    px = np.stack([r, g, b], -1).reshape(-1, 3).astype(np.uint8)
    px.setflags(write=False)
    return px


def decode_normals(kind, px, scale):
    if kind == "host":
        return host.rgb8_to_normal(px, scale)
    from vimg_amd import hip
    return hip.rgb8_to_normal(px, scale)


@pytest.mark.parametrize("backend", DECODERS)
@pytest.mark.parametrize("scale", [0.0, 0.7, 1.0, 25.0])
def test_normal_decode_is_the_float64_normal(scale, backend):
    """normalize(((r, g) / 127.5 - 1) * scale, b / 127.5 - 1) in float64, on every (r, g) at eight b.  Bound per
    component, in u = 2^-24: a component c = b / 127.5f - 1 carries an ABSOLUTE error of 1.5u (the quotient, below 2,
    is rounded to u; the subtraction is exact between 0.5 and 2 and rounds to u / 2 elsewhere) - relative to c this is
    unbounded at bytes 127 and 128, where the subtraction cancels; times `scale` and its rounding, 2.5u * scale for x
    and y.  The error vector, at most sqrt(3) * 2.5u * max(1, scale) long, turns the normalised vector by its length
    over the length |v| of the unnormalised one.  The normalisation itself (three squares, two sums, a root, a
    reciprocal, a product) is a common relative factor of at most 5u: the decoded normal's length is 1 to 5u.
    The GPU's bits are the host library's."""
    px = normal_bytes()
    got = decode_normals(backend, px, scale).astype(np.float64)
    ref, length = M.normal8(px, scale)
    bound = (np.sqrt(3.0) * 2.5 * max(1.0, scale) / length + 5) * U
    err = np.abs(got - ref).max(-1)
    unit = np.abs(np.sqrt((got * got).sum(-1)) - 1)
    at = int(np.argmax(err / bound))
    print(f"normal decode, scale {scale} {backend}: worst error {err.max():.2e}, worst error / bound "
          f"{(err / bound).max():.3f} at bytes {px[at].tolist()}; length off by at most {unit.max():.2e} "
          f"({unit.max() / (5 * U):.2f} of 5u)")
    assert np.all(err <= bound)
    assert unit.max() <= 5 * U
    if backend == "gpu":
        assert np.array_equal(got.astype(np.float32).view(np.uint32), host.rgb8_to_normal(px, scale).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 257])
def test_normal_decode_of_a_few_pixels_is_the_host_librarys(n):
    from vimg_amd import hip
    px = np.random.default_rng(n).integers(0, 256, (n, 3), dtype=np.uint8)
    got = hip.rgb8_to_normal(px, 0.7)
    assert got.shape == (n, 3)
    assert np.array_equal(got.view(np.uint32), host.rgb8_to_normal(px, 0.7).view(np.uint32))


@pytest.mark.gpu
def test_normal_decode_takes_a_second_grid_stride_trip():
    """65 536 * 256 + 1 pixels: one more than the capped grid covers in one trip.  Compared with the host library on
    the last 512 pixels (both sides of the trip's end) and on every 4099th pixel."""
    from vimg_amd import hip
    n = 65536 * 256 + 1
    px = np.random.default_rng(24).integers(0, 256, (n, 3), dtype=np.uint8)
    px[-1] = (3, 250, 77)
    got = hip.rgb8_to_normal(px, 0.7)
    assert got.shape == (n, 3)
    for part in (slice(n - 512, n), slice(0, n, 4099)):
        assert np.array_equal(got[part].view(np.uint32), host.rgb8_to_normal(px[part], 0.7).view(np.uint32))
