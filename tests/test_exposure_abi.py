"""The auto-exposure at its boundary, without a GPU: include/vimg_exposure.h against its ctypes mirror, the exports of
libvimg_exposure.so and of libvimg_hip.so, every argument error of vimg_exposure_adapt with its whole sentence, and the
numpy restatement of its contract (tests/exposure_ref.py) pinned on its own against cases worked out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exposure_ref as R
from abi_layout import c_layout, ctypes_layout
from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # VIMG_E_INVALID
F = np.float32
EXPORTS = ["vimg_exposure_adapt", "vimg_exposure_defaults", "vimg_exposure_last_error"]


def _defaults():
    p = abi.ExposureParams()
    abi.exposure_lib().vimg_exposure_defaults(C.byref(p))
    return p


def _exports(name):
    lib = os.path.join(ROOT, "v-img_amd", "lib", f"libvimg_{name}.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    return nm, sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("vimg_"))


# ---- 1. header and ctypes ------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_structs(tmp_path):
    structs = {"VimgExposureFrames": abi.ExposureFrames, "VimgExposureParams": abi.ExposureParams}
    got = c_layout(tmp_path, ["vimg_exposure.h"], structs,
                   'printf("codes %d %d\\n", VIMG_OK, VIMG_E_INVALID);'
                   'printf("limits %u %u %u %u\\n", VIMG_EXPOSURE_MAX_EXTENT, VIMG_EXPOSURE_BINS, VIMG_EXPOSURE_STATE_BYTES,'
                   ' VIMG_EXPOSURE_MAX_WORKGROUPS);')
    assert got.pop("codes 0") == str(INVALID)
    assert got.pop("limits 32768 256 1040") == str(abi.EXPOSURE_MAX_WORKGROUPS)
    assert (abi.EXPOSURE_BINS, abi.EXPOSURE_STATE_BYTES) == (256, 1040) == (R.BINS, R.STATE_BYTES)
    assert got == ctypes_layout(structs)
    assert C.sizeof(abi.ExposureFrames) == 32 and C.sizeof(abi.ExposureParams) == 32
    assert abi.ExposureFrames().struct_size == 32 and abi.ExposureParams().struct_size == 32
    assert [(f, getattr(abi.ExposureFrames, f).offset) for f, _ in abi.ExposureFrames._fields_] == \
        [("struct_size", 0), ("width", 4), ("height", 8), ("reserved", 12), ("color", 16), ("depth", 24)]
    assert [(f, getattr(abi.ExposureParams, f).offset) for f, _ in abi.ExposureParams._fields_] == \
        [("struct_size", 0), ("low_permille", 4), ("high_permille", 8), ("key", 12), ("min_exposure", 16), ("max_exposure", 20),
         ("rate_brighten", 24), ("rate_darken", 28)]
    # the state: the header's offsets, the mirror's and the restatement's
    assert C.sizeof(abi.ExposureState) == 1040
    want = [("hist", 0), ("exposure", 1024), ("frames", 1028), ("metered", 1032), ("counted", 1036)]
    assert [(f, getattr(abi.ExposureState, f).offset) for f, _ in abi.ExposureState._fields_] == want
    assert [(f, R.STATE.fields[f][1]) for f in R.STATE.names] == want


def test_the_defaults_are_the_headers_and_valid():
    p = _defaults()
    assert p.struct_size == C.sizeof(abi.ExposureParams)
    got = {k: getattr(p, k) for k, _ in abi.ExposureParams._fields_ if k != "struct_size"}
    assert got == {k: (v if isinstance(v, int) else float(F(v))) for k, v in R.DEFAULTS.items()}
    assert (p.low_permille, p.high_permille, p.min_exposure, p.max_exposure, p.rate_brighten, p.rate_darken) == (500, 950, 1 / 64, 64, 0.25, 0.5)
    assert p.rate_darken > p.rate_brighten          # the exposure falls faster than it rises
    # ... and pass the call's own checks: with them the call gets as far as the launch
    import torch
    if not torch.cuda.is_available():
        rc, msg = _call(**_good_call())
        assert rc == -2 and "launch failed" in msg, (rc, msg)          # VIMG_E_DEVICE, no silent success


def test_the_library_exports_the_three_declared_names_and_libvimg_hip_gains_nothing():
    assert sorted(abi.EXPOSURE_SYMBOLS) == EXPORTS
    assert "exposure" not in abi._LIBRARIES and "exposure" in abi._LATER_LIBRARIES
    assert not set(abi._LIBRARIES) & set(abi._LATER_LIBRARIES)
    lib = abi.exposure_lib()
    assert lib is abi.exposure_lib() and callable(lib.vimg_exposure_adapt)
    nm, have = _exports("exposure")
    assert have == EXPORTS
    for kernel in ("meter", "resolve", "apply"):
        assert any(f"exposure_{kernel}_kernel" in l for l in nm.splitlines()), kernel
    # the shared host skeleton (frames/frame_lib.h) is internal: no error slot and no helper of it is a dynamic symbol
    assert not [l for l in nm.splitlines() if any(w in l for w in ("g_error", "vimg_frames", "4fail", "last_errorEv", "check_", "overlaps"))]
    header = open(os.path.join(ROOT, "include", "vimg_exposure.h")).read()
    for name in abi.EXPOSURE_SYMBOLS:
        assert name + "(" in header
    # libvimg_hip.so exports its golden list, and no library shares a name with this one
    hip = open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read().split()
    assert _exports("hip")[1] == sorted(hip) and "exposure" not in " ".join(hip)
    for table in (abi.HIP_SYMBOLS, abi.HIP_TEST_SYMBOLS, abi.HOST_SYMBOLS, abi.DESPECKLE_SYMBOLS, abi.FILTER_SYMBOLS, abi.TEMPORAL_SYMBOLS):
        assert not set(abi.EXPOSURE_SYMBOLS) & set(table)
    # it links the HIP runtime and none of the project's libraries
    path = os.path.join(ROOT, "v-img_amd", "lib", "libvimg_exposure.so")
    needed = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libvimg" not in needed.replace("libvimg_exposure", "")


def test_the_module_and_the_source_directory_of_the_same_name_do_not_collide():
    import vimg_amd.exposure as ex
    assert ex.__file__.endswith("exposure.py") and callable(ex.adapt) and callable(ex.params) and callable(ex.read)
    assert not [f for f in os.listdir(os.path.join(abi.PKG_DIR, "exposure")) if f.endswith(".py")]
    # lum stays ONE definition: the unit includes frames/guides.h and defines none of its own
    unit = open(os.path.join(abi.PKG_DIR, "exposure", "exposure.hip")).read()
    assert '#include "../frames/guides.h"' in unit and '#include "../frames/frame_lib.h"' in unit
    assert "float lum(" not in unit and "0.212671" not in unit and " lum(" in unit


def test_params_takes_two_integer_fields_and_refuses_what_does_not_fit():
    import vimg_amd.exposure as ex
    d, p = _defaults(), ex.params()
    assert all(getattr(p, k) == getattr(d, k) for k, _ in abi.ExposureParams._fields_)
    p = ex.params(low_permille=100, high_permille=900, key=0.25, rate_darken=1)
    assert (p.low_permille, p.high_permille, p.key, p.rate_darken, p.rate_brighten) == (100, 900, 0.25, 1.0, d.rate_brighten)
    for kw, sentence in ((dict(low_permille=-1), "exposure: low_permille must be 0..high_permille - 1, not -1"),
                         (dict(high_permille=2 ** 32), "exposure: high_permille must be low_permille + 1..1000, not 4294967296")):
        with pytest.raises(ValueError) as e:
            ex.params(**kw)
        assert str(e.value) == sentence
    with pytest.raises(TypeError, match=r"exposure: unknown parameters \['gain'\]"):
        ex.params(gain=1.0)


def test_the_previews_refuse_an_exposure_they_cannot_use():
    from vimg_amd import preview
    assert preview.exposure_kw(None, "x") is None and preview.exposure_kw(False, "x") is None
    assert preview.exposure_kw(True, "x") == {} and preview.exposure_kw(dict(key=0.3), "x") == dict(key=0.3)
    with pytest.raises(ValueError, match="preview: exposure must be None, a bool or a dict"):
        preview.exposure_kw(3, "preview")
    with pytest.raises(TypeError, match="exposure: unknown parameters"):
        preview.exposure_kw(dict(radius=3), "preview")
    frame = object()
    assert preview.expose(frame, None) is frame          # None: no call, no import of the library's module even


# ---- 2. argument errors, found before anything is enqueued -------------------------------------------------------
W, H = 8, 4
FRAME, STATE = 12 * W * H, 1040


def _good_call():
    """Arguments vimg_exposure_adapt accepts up to the launch (the pointers are never read on the host)."""
    frames = abi.ExposureFrames(width=W, height=H, color=0x1000, depth=0x2000)
    return dict(frames=frames, params=_defaults(), state=0x4000, out=0x6000)


def _call(frames, params, state, out):
    lib = abi.exposure_lib()
    rc = lib.vimg_exposure_adapt(None if frames is None else C.byref(frames), None if params is None else C.byref(params),
                                 C.c_void_p(state), C.c_void_p(out), None)
    return rc, lib.vimg_exposure_last_error().decode()


def _edit(**kw):
    a = _good_call()
    for k, v in kw.items():
        if k in a:
            a[k] = v
        elif k in dict(abi.ExposureFrames._fields_):
            setattr(a["frames"], k, v)
        else:
            setattr(a["params"], k, v)
    return a


NAN, INF = float("nan"), float("inf")
ERRORS = [
    (dict(frames=None), "null frames"), (dict(params=None), "null params"),
    (dict(struct_size=31), "frames.struct_size 31 is below the struct's 32"),
    (dict(width=0), "width and height must be 1..32768, not 0 x 4"), (dict(height=0), "width and height must be 1..32768, not 8 x 0"),
    (dict(width=32769), "width and height must be 1..32768, not 32769 x 4"),
    (dict(height=32769), "width and height must be 1..32768, not 8 x 32769"),
    (dict(color=None), "null color frame"), (dict(state=None), "null state"),
    (dict(state=0x4008), "the state must be 16-byte aligned"), (dict(state=0x4004), "the state must be 16-byte aligned"),
    (dict(low_permille=950), "the permilles must be 0 <= low < high <= 1000, not 950 and 950"),
    (dict(low_permille=951), "the permilles must be 0 <= low < high <= 1000, not 951 and 950"),
    (dict(high_permille=1001), "the permilles must be 0 <= low < high <= 1000, not 500 and 1001"),
    (dict(low_permille=0, high_permille=0), "the permilles must be 0 <= low < high <= 1000, not 0 and 0"),
    (dict(key=0.0), "key must be > 0 and finite, not 0"), (dict(key=-1.0), "key must be > 0 and finite, not -1"),
    (dict(key=NAN), "key must be > 0 and finite, not nan"), (dict(key=INF), "key must be > 0 and finite, not inf"),
    (dict(min_exposure=0.0), "min_exposure must be > 0 and finite, not 0"), (dict(min_exposure=NAN), "min_exposure must be > 0 and finite, not nan"),
    (dict(min_exposure=INF), "min_exposure must be > 0 and finite, not inf"),
    (dict(max_exposure=-2.0), "max_exposure must be > 0 and finite, not -2"), (dict(max_exposure=NAN), "max_exposure must be > 0 and finite, not nan"),
    (dict(max_exposure=INF), "max_exposure must be > 0 and finite, not inf"),
    (dict(min_exposure=2.0, max_exposure=1.0), "min_exposure 2 is above max_exposure 1"),
    (dict(rate_brighten=0.0), "rate_brighten must be > 0 and finite, not 0"), (dict(rate_brighten=NAN), "rate_brighten must be > 0 and finite, not nan"),
    (dict(rate_brighten=INF), "rate_brighten must be > 0 and finite, not inf"), (dict(rate_brighten=1.5), "rate_brighten must be at most 1, not 1.5"),
    (dict(rate_darken=-0.5), "rate_darken must be > 0 and finite, not -0.5"), (dict(rate_darken=NAN), "rate_darken must be > 0 and finite, not nan"),
    (dict(rate_darken=INF), "rate_darken must be > 0 and finite, not inf"), (dict(rate_darken=1.25), "rate_darken must be at most 1, not 1.25"),
    # each forbidden overlap: the last byte of one buffer on the first of the other, and the other way round
    (dict(out=0x1000 + 12), "the output overlaps the color frame without being it"),
    (dict(out=0x1000 - FRAME + 1), "the output overlaps the color frame without being it"),
    (dict(out=0x2000), "the output overlaps the depth frame"), (dict(out=0x2000 + FRAME - 1), "the output overlaps the depth frame"),
    (dict(out=0x2000 - FRAME + 1), "the output overlaps the depth frame"),
    (dict(out=0x4000 + STATE - 1), "the output overlaps the state"), (dict(out=0x4000 - FRAME + 1), "the output overlaps the state"),
    (dict(state=0x1000 + FRAME - 16), "the state overlaps the color frame"), (dict(state=0x1000 - STATE + 16, out=None), "the state overlaps the color frame"),
    (dict(state=0x2000 + FRAME - 16), "the state overlaps the depth frame"), (dict(state=0x2000 - STATE + 16, out=None), "the state overlaps the depth frame"),
]


@pytest.mark.parametrize("edit,sentence", ERRORS, ids=[f"{'-'.join(e)}-{i}" for i, (e, _) in enumerate(ERRORS)])
def test_argument_errors_are_invalid_with_their_sentence_and_need_no_device(edit, sentence):
    rc, msg = _call(**_edit(**edit))
    assert rc == INVALID and msg == "exposure: " + sentence, (rc, msg)


def test_the_checks_come_in_a_fixed_order():
    """Two faults at once: the one that comes first - the structs, the extent, the colour frame, the state and its
    alignment, the permilles, key, min, max, their order, the two rates, the overlaps - is reported."""
    order = [dict(struct_size=31), dict(width=0), dict(color=None), dict(state=None), dict(low_permille=999), dict(key=NAN),
             dict(min_exposure=NAN), dict(max_exposure=NAN), dict(rate_brighten=NAN), dict(rate_darken=NAN), dict(out=0x2000)]
    sentences = ["frames.struct_size", "width and height", "null color frame", "null state", "the permilles must be", "key must be",
                 "min_exposure must be", "max_exposure must be", "rate_brighten must be", "rate_darken must be", "overlaps the depth frame"]
    for i in range(len(order) - 1):
        rc, msg = _call(**_edit(**order[i], **order[i + 1]))
        assert rc == INVALID and sentences[i] in msg, (i, msg)
    rc, msg = _call(**_edit(state=0x4008, low_permille=999))
    assert rc == INVALID and "16-byte aligned" in msg
    rc, msg = _call(**_edit(min_exposure=2.0, max_exposure=1.0, rate_brighten=NAN))
    assert rc == INVALID and "is above max_exposure" in msg


def test_params_struct_size_and_what_may_be_null_or_touch():
    a = _good_call()
    a["params"].struct_size = 31
    rc, msg = _call(**a)
    assert rc == INVALID and msg == "exposure: params.struct_size 31 is below the struct's 32"
    # the depth frame and the output may be NULL, the output may be the colour frame, buffers may touch end to start, and
    # the ends of every range are inside it: the call passes every argument check
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(depth=None), dict(out=None), dict(out=0x1000), dict(out=0x2000 - FRAME), dict(out=0x2000 + FRAME),
                   dict(state=0x1000 + FRAME), dict(out=0x4000 + STATE), dict(depth=None, out=0x2000),
                   dict(low_permille=0, high_permille=1000), dict(low_permille=999, high_permille=1000),
                   dict(min_exposure=1.0, max_exposure=1.0), dict(rate_brighten=1.0, rate_darken=1.0)):
            rc, msg = _call(**_edit(**ok))
            assert rc == -2 and "launch failed" in msg, (ok, rc, msg)


# ---- 3. the restatement, pinned on its own against hand-computed cases ---------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _grey(L, h=4, w=4):
    """[h, w, 3] whose luminance is L to a rounding: green alone, g = L / 0.715160."""
    c = np.zeros((h, w, 3), F)
    c[..., 1] = F(L) / F(0.715160)
    return c


def test_the_bins_of_the_ends_of_the_range_and_of_what_is_not_a_luminance():
    lo, hi = F(2.0 ** -16), F(2.0 ** 16)
    L = np.array([lo, np.nextafter(lo, F(0)), hi, np.nextafter(hi, F(0)), 1e-42, 0, -1, np.nan, np.inf, 1, np.nextafter(F(1), F(0)),
                  1.125, 3e38, -np.inf], F)
    k, counted = R.bin_of(L)
    #                     2^-16  below  2^16  below  denormal  0  -1  NaN  inf  1    below 1  1.125  huge  -inf
    assert k.tolist()[:5] == [0, 0, 255, 255, 0] and k.tolist()[9:13] == [128, 127, 129, 255]
    assert counted.tolist() == [True, True, True, True, True, False, False, False, False, True, True, True, True, False]
    assert L[4] > 0 and L[4] < np.finfo(F).tiny          # it IS a denormal
    # a whole octave in eight equal steps of the mantissa
    assert R.bin_of(np.array([2, 2.25, 2.5, 2.75, 3, 3.25, 3.5, 3.75, 4], F))[0].tolist() == list(range(136, 145))


def test_every_edge_falls_in_its_own_bin_and_the_float_below_it_in_the_one_before():
    edges = np.array([R.edge(b) for b in range(257)], F)
    assert edges[0] == F(2.0 ** -16) and edges[256] == F(2.0 ** 16) and edges[128] == 1 and (np.diff(edges) > 0).all()
    assert R.bin_of(edges[:256])[0].tolist() == list(range(256))
    assert R.bin_of(np.nextafter(edges[1:], F(0)))[0].tolist() == list(range(256))
    # eight per octave: every eighth edge doubles
    assert (edges[8:] == F(2) * edges[:-8]).all()


@pytest.mark.parametrize("L", [2.0 ** -15.5, 0.01, 0.18, 1.0, 1.0624, 7.3, 900.0, 2.0 ** 15.9])
def test_a_constant_frame_meters_within_one_bin_width_of_its_luminance(L):
    color = _grey(L)
    state = R.adapt(color)[1]
    s = R.read(state)
    k = int(R.bin_of(R.luminance(color))[0][0, 0])
    width = float(R.edge(k + 1)) - float(R.edge(k))
    # every rank of the window is in bin k: m = k exactly, f = 0 and metered is the bin's start
    assert s["metered"] == float(R.edge(k)) and abs(s["metered"] - L) <= width and width <= L / 8
    assert s["counted"] == 16 and s["frames"] == 1
    assert s["exposure"] == float(R.target_of(R.edge(k), 0.18, 1 / 64, 64))
    assert not R.fields(state)["hist"].any()


def test_the_window_by_hand():
    """10 pixels in bin 100, 10 in bin 108, low 250, high 750: T 20, lo 5, hi 15 - five ranks of each bin, S = 5 * 100 +
    5 * 108, m = 104: half an octave above edge(100) on the piecewise-linear scale."""
    hist = np.zeros(256, np.uint32)
    hist[100], hist[108] = 10, 10
    assert R.window(hist, 250, 750) == (20, 5, 15, 1040)
    assert R.metered_of(1040, 10) == R.edge(104)
    # m = 103.5: halfway between two edges
    assert R.window(hist, 300, 700) == (20, 6, 14, 4 * 100 + 4 * 108)
    hist[100] = 11
    T, lo, hi, S = R.window(hist, 0, 1000)
    assert (T, lo, hi, S) == (21, 0, 21, 1100 + 1080)
    m = F(2180) / F(21)
    assert R.metered_of(S, 21) == R.edge(103) + (m - F(103)) * (R.edge(104) - R.edge(103))
    # integer division: T 21, 500 and 950 permille -> ranks 10 .. 18
    assert R.window(hist, 500, 950)[1:3] == (10, 19)
    # the clamps are comparisons
    assert R.target_of(F(1e-4), 0.18, 1 / 64, 64) == 64 and R.target_of(F(1e4), 0.18, 1 / 64, 64) == F(1 / 64)
    assert R.target_of(F(0.5), 0.18, 1 / 64, 64) == F(0.18) / F(0.5)


def test_one_pixel_a_thousand_times_brighter_moves_the_target_by_less_than_one_percent():
    """130 x 67 log-uniform luminances: 8710 counted pixels, a window of 3 920 ranks (the defaults' 450 permille).  One
    pixel moved up the ranks shifts the window by at most one rank: S changes by at most 255 over at least 3 900 ranks, under
    0.07 of a bin, and a bin is at most log2(1.125) = 0.17 octave wide: 0.012 octave, under 1 %.  The same edit, made to the
    brightest pixel, moves 1 / max luminance, Reinhard's scale, a thousandfold."""
    rng = np.random.default_rng(7)
    color = _grey(1, 67, 130) * (F(2) ** rng.uniform(-6, 6, (67, 130, 1)).astype(F))
    base = R.target(color)
    assert R.window(R.meter(color), 500, 950)[2] - R.window(R.meter(color), 500, 950)[1] >= 3900
    lum = R.luminance(color)
    worst = 0.0
    for y, x in ((0, 0), (33, 65), (66, 129), tuple(np.unravel_index(np.argmin(lum), lum.shape)), tuple(np.unravel_index(np.argmax(lum), lum.shape))):
        edited = color.copy()
        edited[y, x] *= F(1000)
        moved = R.target(edited)
        worst = max(worst, abs(float(moved) / float(base) - 1))
    assert 0 < worst < 0.01, worst
    # the brightest pixel times 1000: 1 / max falls a thousandfold, E* by under 1 %
    y, x = np.unravel_index(np.argmax(lum), lum.shape)
    edited = color.copy()
    edited[y, x] *= F(1000)
    assert float(lum.max()) / float(R.luminance(edited).max()) == pytest.approx(1e-3, rel=1e-3)
    assert abs(float(R.target(edited)) / float(base) - 1) < 0.01


def test_nothing_metered_leaves_the_scalars_alone_and_a_fresh_state_scales_by_one():
    color = _grey(0.53)
    out, state = R.adapt(color, key=0.25)
    before = R.read(state)
    assert before["frames"] == 1 and before["exposure"] == 0.5 and np.array_equal(out, color * F(0.5))
    for black in (np.zeros((4, 4, 3), F), np.full((4, 4, 3), np.nan, F), np.full((4, 4, 3), -1, F), np.full((4, 4, 3), np.inf, F)):
        out, after = R.adapt(black, state=state, key=0.25)
        assert R.read(after) == dict(before, counted=0)
        assert np.array_equal(after[:1036], state[:1036])
        assert np.array_equal(_bits(out), _bits((black * F(0.5)).astype(F)))          # still scaled by the exposure it had
    # a depth frame of misses alone: the same
    out, after = R.adapt(color, np.zeros((4, 4, 3), F), state=state, key=0.25)
    assert R.read(after) == dict(before, counted=0)
    # a fresh state: exposure reads 1, the frame comes back as it is, the bytes stay zero
    out, after = R.adapt(black, key=0.25)
    assert R.read(after) == dict(exposure=1.0, frames=0, metered=0.0, counted=0) and not after.any()
    assert np.array_equal(_bits(out), _bits(black))
    # hi == lo: one counted pixel and a window of under one rank
    one = np.zeros((4, 4, 3), F)
    one[0, 0] = 1
    after = R.adapt(one, state=state, key=0.25)[1]
    assert R.read(after) == dict(before, counted=1)
    assert R.read(R.adapt(one, state=state, key=0.25, low_permille=0, high_permille=1000)[1])["frames"] == 2


def test_the_exposure_moves_toward_its_target_by_the_stated_rates():
    """key 0.25: a frame of luminance 0.53 meters as its bin's start 0.5 and has E* = 0.5, one of 0.13 meters as 0.125 and
    has E* = 2, all exact in float32."""
    kw = dict(key=0.25, rate_brighten=0.25, rate_darken=0.5)
    state = R.adapt(_grey(0.53), **kw)[1]
    assert R.read(state)["exposure"] == 0.5                      # the first frame takes its target
    state = R.adapt(_grey(0.13), state=state, **kw)[1]
    assert R.read(state)["exposure"] == 0.5 + (2 - 0.5) * 0.25     # brighter: a quarter of the way
    state = R.adapt(_grey(0.13), state=state, **kw)[1]
    assert R.read(state)["exposure"] == 0.875 + (2 - 0.875) * 0.25
    E = R.read(state)["exposure"]
    state = R.adapt(_grey(0.53), state=state, **kw)[1]
    assert R.read(state)["exposure"] == E + (0.5 - E) * 0.5        # darker: half the way
    assert R.read(state)["frames"] == 4 and R.read(state)["metered"] == 0.5
