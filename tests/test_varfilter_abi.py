"""The variance-guided filter library at its boundary, without a GPU: include/vimg_varfilter.h against its ctypes
mirror, the exports of libvimg_varfilter.so, every argument error of its two calls, and the numpy restatement of the
contract (tests/varfilter_ref.py) pinned on its own - among the pins the inequalities the filter was built for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import atrous_ref as A
import varfilter_ref as R
from abi_layout import c_layout, ctypes_layout
from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # VIMG_E_INVALID
F = np.float32
EXPORTS = ["vimg_varfilter_atrous", "vimg_varfilter_defaults", "vimg_varfilter_last_error", "vimg_varfilter_variance",
           "vimg_varfilter_workspace"]


def _defaults():
    p = abi.VarFilterParams()
    abi.varfilter_lib().vimg_varfilter_defaults(C.byref(p))
    return p


def default_kw():
    p = _defaults()
    return {k: getattr(p, k) for k, _ in abi.VarFilterParams._fields_ if k != "struct_size"}


def atrous_default_kw():
    p = abi.AtrousParams()
    abi.filter_lib().vimg_filter_atrous_defaults(C.byref(p))
    return {k: getattr(p, k) for k, _ in abi.AtrousParams._fields_ if k != "struct_size"}


# ---- 1. header and ctypes ------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_structs(tmp_path):
    structs = {"VimgVarFilterFrames": abi.VarFilterFrames, "VimgVarFilterParams": abi.VarFilterParams}
    got = c_layout(tmp_path, ["vimg_varfilter.h"], structs, 'printf("codes %d %d\\n", VIMG_OK, VIMG_E_INVALID);')
    assert got.pop("codes 0") == str(INVALID)
    assert got == ctypes_layout(structs)
    assert C.sizeof(abi.VarFilterFrames) == 64 and C.sizeof(abi.VarFilterParams) == 28
    assert abi.VarFilterFrames().struct_size == 64 and abi.VarFilterParams().struct_size == 28
    # the shared eight fields, where frame_lib.h's check_head and hip.FrameCall expect them
    shared = [(f, getattr(abi.VarFilterFrames, f).offset) for f, _ in abi.FilterFrames._fields_]
    assert shared == [(f, getattr(abi.FilterFrames, f).offset) for f, _ in abi.FilterFrames._fields_]
    assert [o for _, o in shared[:8]] == [0, 4, 8, 12, 16, 24, 32, 40] and abi.VarFilterFrames.variance.offset == 56


def test_the_workspace_is_64_bytes_per_pixel_and_the_defaults_are_valid():
    lib = abi.varfilter_lib()
    for w, h in ((1, 1), (3, 5), (1800, 800), (32768, 32768), (0, 7)):
        assert lib.vimg_varfilter_workspace(w, h) == 64 * w * h
        assert lib.vimg_varfilter_workspace(w, h) == abi.filter_lib().vimg_filter_atrous_workspace(w, h)
    p = _defaults()
    assert p.struct_size == C.sizeof(abi.VarFilterParams) and 1 <= p.iterations <= 12
    assert p.sigma_luminance > 0 and 0 < p.sigma_normal < np.inf and 0 < p.sigma_plane < np.inf
    assert 0 < p.albedo_floor < 1 and np.frexp(p.albedo_floor)[0] == 0.5       # a power of two: x / f * f is exact
    assert 0 < p.variance_floor < np.inf
    # ... and pass the call's own checks: with them the call gets as far as the launch
    import torch
    if not torch.cuda.is_available():
        rc, msg = _call(**_good_call())
        assert rc == -2 and "launch failed" in msg, (rc, msg)          # VIMG_E_DEVICE, no silent success


def test_the_library_exports_the_five_declared_names_and_leaves_the_other_libraries_alone():
    assert sorted(abi.VARFILTER_SYMBOLS) == EXPORTS
    abi.varfilter_lib()                    # loads on a machine without a GPU
    lib = os.path.join(ROOT, "v-img_amd", "lib", "libvimg_varfilter.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    have = sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("vimg_"))
    assert have == EXPORTS
    for kernel in ("pack", "estimate", "iteration", "unpack", "variance"):
        assert any(f"varfilter_{kernel}_kernel" in l for l in nm.splitlines()), kernel
    # the shared host skeleton (frames/frame_lib.h) is internal: no error slot and no helper of it is a dynamic symbol
    assert not [l for l in nm.splitlines() if any(w in l for w in ("g_error", "vimg_frames", "4fail", "last_errorEv", "check_"))]
    header = open(os.path.join(ROOT, "include", "vimg_varfilter.h")).read()
    for name in abi.VARFILTER_SYMBOLS:
        assert name + "(" in header
    for other in (abi.HIP_SYMBOLS, abi.HIP_TEST_SYMBOLS, abi.FILTER_SYMBOLS, abi.TEMPORAL_SYMBOLS):
        assert not set(abi.VARFILTER_SYMBOLS) & set(other)
    assert "varfilter" not in open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read()
    # it links the HIP runtime and none of the project's libraries
    needed = subprocess.run(["readelf", "-d", lib], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libvimg" not in needed.replace("libvimg_varfilter", "")


def test_the_module_and_the_source_directory_of_the_same_name_do_not_collide():
    import vimg_amd.varfilter as vf
    assert vf.__file__.endswith("varfilter.py") and callable(vf.atrous) and callable(vf.variance)
    assert not [f for f in os.listdir(os.path.join(abi.PKG_DIR, "varfilter")) if f.endswith(".py")]


# ---- 2. argument errors, found before anything is enqueued -------------------------------------------------------
def _good_call():
    """Arguments vimg_varfilter_atrous accepts up to the launch (the pointers are never read on the host)."""
    frames = abi.VarFilterFrames(width=8, height=4, color=0x1000, normal=0x2000, position=0x3000, depth=0x4000, albedo=0x5000,
                                 variance=0x7000)
    return dict(frames=frames, params=_defaults(), out=0x6000, out_variance=0x8000, workspace=0x10000, nbytes=64 * 8 * 4)


def _call(frames, params, out, out_variance, workspace, nbytes):
    lib = abi.varfilter_lib()
    rc = lib.vimg_varfilter_atrous(None if frames is None else C.byref(frames), None if params is None else C.byref(params),
                                   C.c_void_p(out), C.c_void_p(out_variance), C.c_void_p(workspace), nbytes, None)
    return rc, lib.vimg_varfilter_last_error().decode()


def _edit(**kw):
    a = _good_call()
    for k, v in kw.items():
        if k in a:
            a[k] = v
        elif k in dict(abi.VarFilterFrames._fields_):
            setattr(a["frames"], k, v)
        else:
            setattr(a["params"], k, v)
    return a


NAN, INF = float("nan"), float("inf")
ERRORS = [
    (dict(frames=None), "null frames"), (dict(params=None), "null params"),
    (dict(color=None), "null color frame"), (dict(normal=None), "null normal frame"),
    (dict(position=None), "null position frame"), (dict(depth=None), "null depth frame"),
    (dict(out=None), "null output"), (dict(workspace=None), "null workspace"),
    (dict(struct_size=63), "frames.struct_size 63 is below the struct's 64"),
    (dict(width=0), "width and height must be 1..32768"), (dict(height=0), "width and height must be 1..32768"),
    (dict(width=32769, nbytes=2 ** 40), "width and height must be 1..32768"),
    (dict(height=32769, nbytes=2 ** 40), "width and height must be 1..32768"),
    (dict(iterations=0), "iterations must be 1..12"), (dict(iterations=13), "iterations must be 1..12"),
    (dict(sigma_luminance=0.0), "sigma_luminance must be > 0"), (dict(sigma_luminance=-1.0), "sigma_luminance must be > 0"),
    (dict(sigma_luminance=NAN), "sigma_luminance must be > 0"),
    (dict(sigma_normal=0.0), "sigma_normal must be > 0"), (dict(sigma_normal=-2.0), "sigma_normal must be > 0"),
    (dict(sigma_normal=NAN), "sigma_normal must be > 0"), (dict(sigma_normal=INF), "sigma_normal must be > 0 and finite"),
    (dict(sigma_plane=0.0), "sigma_plane must be > 0"), (dict(sigma_plane=-0.5), "sigma_plane must be > 0"),
    (dict(sigma_plane=NAN), "sigma_plane must be > 0"), (dict(sigma_plane=INF), "sigma_plane must be > 0 and finite"),
    (dict(albedo_floor=0.0), "albedo_floor must be > 0"), (dict(albedo_floor=-0.25), "albedo_floor must be > 0"),
    (dict(albedo_floor=NAN), "albedo_floor must be > 0"), (dict(albedo_floor=INF), "albedo_floor must be > 0 and finite"),
    (dict(variance_floor=0.0), "variance_floor must be > 0"), (dict(variance_floor=-1e-8), "variance_floor must be > 0"),
    (dict(variance_floor=NAN), "variance_floor must be > 0"), (dict(variance_floor=INF), "variance_floor must be > 0 and finite"),
    (dict(nbytes=64 * 8 * 4 - 1), "the workspace has 2047 bytes, 8 x 4 needs 2048"),
    (dict(workspace=0x10008), "the workspace must be 16-byte aligned"),
]


@pytest.mark.parametrize("edit,sentence", ERRORS, ids=[f"{'-'.join(e)}-{i}" for i, (e, _) in enumerate(ERRORS)])
def test_argument_errors_are_invalid_with_their_sentence_and_need_no_device(edit, sentence):
    rc, msg = _call(**_edit(**edit))
    assert rc == INVALID and msg.startswith("varfilter: ") and sentence in msg, (rc, msg)


def test_params_struct_size_and_what_may_be_null_or_infinite():
    a = _good_call()
    a["params"].struct_size = 27
    rc, msg = _call(**a)
    assert rc == INVALID and "params.struct_size 27 is below the struct's 28" in msg
    rc, msg2 = _call(**_edit(iterations=99))
    assert rc == INVALID and msg2 != msg and "99" in msg2
    # sigma_luminance may be +inf; albedo, variance and out_variance may be NULL: the call passes every argument check
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(sigma_luminance=INF), dict(albedo=None), dict(variance=None), dict(out_variance=None)):
            rc, msg = _call(**_edit(**ok))
            assert rc == -2 and "launch failed" in msg, (ok, rc, msg)


VARIANCE_ERRORS = [
    (dict(count=None), "null count"), (dict(batches=None), "null batches"), (dict(m2=None), "null m2"),
    (dict(out=None), "null output variance"),
    (dict(width=0), "width and height must be 1..32768, not 0 x 4"), (dict(height=0), "width and height must be 1..32768, not 8 x 0"),
    (dict(width=32769), "width and height must be 1..32768"), (dict(height=32769), "width and height must be 1..32768"),
]


@pytest.mark.parametrize("edit,sentence", VARIANCE_ERRORS, ids=[next(iter(e)) + str(i) for i, (e, _) in enumerate(VARIANCE_ERRORS)])
def test_argument_errors_of_the_variance_call(edit, sentence):
    a = dict(width=8, height=4, count=0x1000, batches=0x2000, m2=0x3000, out=0x4000) | edit
    lib = abi.varfilter_lib()
    rc = lib.vimg_varfilter_variance(a["width"], a["height"], C.c_void_p(a["count"]), C.c_void_p(a["batches"]), C.c_void_p(a["m2"]),
                                     C.c_void_p(a["out"]), None)
    msg = lib.vimg_varfilter_last_error().decode()
    assert rc == INVALID and msg.startswith("varfilter: ") and sentence in msg, (rc, msg)


# ---- 3. the restatement, pinned on its own -----------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def shadowed():
    return R.shadowed_frame(64, 96)


def _guides(s):
    return s["normal"], s["position"], s["depth"], s["albedo"]


def test_zero_variance_moves_no_pixel_further_than_the_floor_allows(shadowed):
    """variance = 0 everywhere: den = variance_floor, so a tap takes part only when dL^2 < floor, |dL| < sqrt(floor).
    The result is a convex mean of colours whose demodulated luminance is within sqrt(floor) of the pixel's own, so its
    luminance moves by less than sqrt(floor) = 1e-4 at floor 1e-8 (plus rounding) - and the variance stays 0."""
    s = shadowed
    rng = np.random.default_rng(2)
    color, _ = R.noisy_mean(s, 16, 4, rng)
    p = dict(default_kw(), sigma_luminance=8.0, variance_floor=1e-8, iterations=5)
    out, out_v = R.atrous(color, *_guides(s), variance=np.zeros(s["hit"].shape, F), **p)
    a = np.where(s["albedo"] > F(p["albedo_floor"]), s["albedo"], F(p["albedo_floor"]))
    dl = np.abs(R.lum(out.astype(np.float64) / a) - R.lum(color.astype(np.float64) / a))[s["hit"]]
    rel = (np.abs(out.astype(np.float64) - color) / np.abs(color))[s["hit"]]
    print(f"largest luminance move {dl.max():.3e}, largest relative change {rel.max():.3e}")
    assert dl.max() < 5 * 1e-4 * 1.001            # five iterations, each within sqrt(floor)
    assert np.array_equal(out_v, np.zeros_like(out_v))
    assert np.array_equal(_bits(out[~s["hit"]]), _bits(color[~s["hit"]]))


def test_a_frame_without_live_pixels_comes_back_bit_for_bit():
    rng = np.random.default_rng(5)
    h, w = 13, 21
    zero = np.zeros((h, w, 3), F)
    anyf = rng.gamma(2.0, 0.5, (h, w, 3)).astype(F)
    var = rng.gamma(2.0, 0.5, (h, w)).astype(F)
    for albedo in (None, zero, rng.uniform(0.1, 0.9, (h, w, 3)).astype(F)):
        for depth in (zero, np.full((h, w, 3), np.nan, F), np.full((h, w, 3), -1, F)):
            out, out_v = R.atrous(anyf, zero, zero, depth, albedo, var, **default_kw())
            if albedo is None or not albedo.any():      # a floor that is a power of two: x / f * f is exact
                assert np.array_equal(_bits(out), _bits(anyf))
            else:
                assert np.allclose(out, anyf, rtol=2e-7, atol=0)
            assert np.array_equal(out_v, np.zeros((h, w), F))          # V is 0 for a pixel that is not live


@pytest.mark.parametrize("with_variance", [False, True])
def test_a_nan_colour_reaches_no_neighbour(with_variance):
    """A NaN colour makes every S it enters NaN, and a non-finite luminance is no tap of the estimate: the pixel stays
    NaN (its centre tap) and no other pixel becomes NaN."""
    h, w = 24, 24
    rng = np.random.default_rng(7)
    color = (0.5 * rng.gamma(8.0, 1 / 8, (h, w, 1)) * np.ones(3)).astype(F)
    color[11, 13, 1] = np.nan
    normal = np.zeros((h, w, 3), F)
    normal[..., 2] = 1
    yy, xx = np.mgrid[0:h, 0:w]
    position = np.stack([xx, yy, np.zeros_like(xx)], -1).astype(F)
    depth = np.full((h, w, 3), 10, F)
    var = np.full((h, w), 0.25 / 8, F) if with_variance else None
    out, out_v = R.atrous(color, normal, position, depth, None, var, **default_kw())
    assert np.isnan(out[11, 13, 1]) and np.isnan(out).sum() == 1
    rest = np.ones((h, w), bool)
    rest[10:13, 12:15] = False               # the pixel and the eight that its NaN variance reaches through the prefilter
    assert np.isfinite(out_v[rest]).all()
    assert np.abs(out[rest] - 0.5).max() < np.abs(color[rest] - 0.5).max()


def test_the_filtered_variance_is_not_above_the_input_on_the_flat_noisy_part(shadowed):
    """V' = sum w^2 V / (sum w)^2 <= max V over the taps; where the variance is one value, every pixel's falls."""
    s = shadowed
    rng = np.random.default_rng(3)
    color, var = R.noisy_mean(s, 64, 8, rng)
    flat = np.full(s["hit"].shape, np.nanmedian(var[s["hit"]]), F)
    out, out_v = R.atrous(color, *_guides(s), variance=flat, **default_kw())
    live = s["hit"]
    assert np.isfinite(out_v).all() and (out_v[live] <= flat[live]).all()
    assert np.median(out_v[live]) < 0.1 * flat[live][0]
    assert np.array_equal(out_v[~live], np.zeros_like(out_v[~live]))


COUNTS = [(4, 1), (4, 2), (16, 4), (64, 8), (512, 8)]


@pytest.mark.parametrize("n,K", COUNTS, ids=[f"{n}spp-K{K}" for n, K in COUNTS])
def test_nearer_the_clean_frame_than_the_fixed_filter_and_than_the_noisy_frame(shadowed, n, K):
    """The shadowed synthetic frame (a shadow edge no guide knows about) at n samples in K batches: the restatement at
    the library's defaults is strictly nearer the clean frame than atrous_ref.atrous at the a-trous defaults, and than
    the noisy frame.  e = mean((x - clean)^2 / (clean^2 + 0.01)) over the hit pixels."""
    s = shadowed
    color, var = R.noisy_mean(s, n, K, np.random.default_rng(100 + n + K))
    fixed = A.atrous(color, *_guides(s), **atrous_default_kw())
    guided, _ = R.atrous(color, *_guides(s), variance=None if K < 2 else var, **default_kw())
    e = {k: R.rel_error(v, s["clean"], s["hit"]) for k, v in dict(noisy=color, fixed=fixed, guided=guided).items()}
    print(f"n {n} K {K}: " + ", ".join(f"{k} {v:.5f}" for k, v in e.items()))
    assert e["guided"] < e["fixed"] and e["guided"] < e["noisy"], e


def test_on_a_frame_of_mixed_counts_both_parts_are_nearer(shadowed):
    """The upper 40 rows at 512 samples (K = 8), the lower rows at 8 (K = 2): one setting serves both."""
    s = shadowed
    h, w = s["hit"].shape
    top = np.arange(h)[:, None] < 40
    n = np.where(top, 512, 8) * np.ones((h, w), int)
    K = np.where(top, 8, 2) * np.ones((h, w), int)
    color, var = R.noisy_mean(s, n, K, np.random.default_rng(9))
    fixed = A.atrous(color, *_guides(s), **atrous_default_kw())
    guided, _ = R.atrous(color, *_guides(s), variance=var, **default_kw())
    for name, rows in (("converged", top & s["hit"]), ("noisy", ~top & s["hit"])):
        e = {k: R.rel_error(v, s["clean"], rows) for k, v in dict(noisy=color, fixed=fixed, guided=guided).items()}
        print(f"{name} rows: " + ", ".join(f"{k} {v:.5f}" for k, v in e.items()))
        assert e["guided"] < e["fixed"] and e["guided"] < e["noisy"], (name, e)


def test_the_variance_formula_is_the_errors_text():
    """vimg_hip.h: err = K < 2 ? +inf : sqrt((M2 < 0 ? 0 : M2) / float(K - 1) / float(N)) / (fabs(Y(S) / float(N)) + 1e-3f)."""
    N = np.array([[0, 4, 4, 8, 12, 7, 0, 3, 4000000000]], np.uint32)
    K = np.array([[0, 0, 1, 2, 3, 2, 2, 5, 4000000000]], np.uint32)
    M2 = np.array([[0.0, 1.0, 2.0, 0.75, 1e-3, -0.5, 1.0, np.nan, 3.0]], F)
    V = R.variance(N, K, M2)
    assert V.dtype == F and V.shape == N.shape
    assert np.isnan(V[0, [0, 1, 2, 6, 7]]).all()                   # K = 0, K = 0, K = 1, N = 0, a NaN M2
    assert V[0, 3] == F(0.75) / F(1) / F(8) and V[0, 4] == F(1e-3) / F(2) / F(12) and V[0, 5] == 0
    assert V[0, 8] == F(3.0) / F(3999999999) / F(4000000000)       # uint32, not int32
    assert not R.known(V[0, [0, 1, 2, 6, 7]]).any() and R.known(V[0, [3, 4, 5, 8]]).all()
    # against the error's own text, with sums whose luminance is the mean
    S = np.array([[[0.4 * n, 0.5 * n, 0.6 * n] for n in N[0].astype(np.float64)]], F)
    with np.errstate(all="ignore"):
        m = R.lum(S) / N.astype(F)
        err_text = np.where(K < 2, F(np.inf), np.sqrt(np.where(M2 < 0, F(0), M2) / (K.astype(np.int64) - 1).astype(F) / N.astype(F))
                            / (np.abs(m) + F(1e-3))).astype(F)
        from_v = (np.sqrt(V) / (np.abs(m) + F(1e-3))).astype(F)
    ok = (K >= 2) & (N > 0) & ~np.isnan(M2)
    assert np.array_equal(_bits(from_v[ok]), _bits(err_text[ok]))
    assert np.array_equal(R.known(np.array([0.0, -0.0, 1.0, np.inf, -1.0, np.nan, -np.inf], F)),
                          [True, True, True, False, False, False, False])
