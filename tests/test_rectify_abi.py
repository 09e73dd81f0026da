"""The history clamp at its boundary, without a GPU: include/vimg_rectify.h against its ctypes mirror, the exports of
libvimg_rectify.so and of the other libraries, every argument error of vimg_rectify_clamp with its whole sentence, and
the numpy restatement of its contract (tests/rectify_ref.py) pinned on its own against cases worked out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rectify_ref as R
from abi_layout import c_layout, ctypes_layout
from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # VIMG_E_INVALID
F = np.float32
EXPORTS = ["vimg_rectify_clamp", "vimg_rectify_defaults", "vimg_rectify_last_error", "vimg_rectify_workspace"]
OTHERS = {"filter": (abi.FILTER_SYMBOLS,), "temporal": (abi.TEMPORAL_SYMBOLS,), "varfilter": (abi.VARFILTER_SYMBOLS,),
          "moments": (abi.MOMENTS_SYMBOLS,), "infill": (abi.INFILL_SYMBOLS,), "wtemporal": (abi.WTEMPORAL_SYMBOLS,),
          "antilag": (abi.ANTILAG_SYMBOLS,), "motion": (abi.MOTION_SYMBOLS,), "despeckle": (abi.DESPECKLE_SYMBOLS,),
          "exposure": (abi.EXPOSURE_SYMBOLS,), "demand": (abi.DEMAND_SYMBOLS,), "host": (abi.HOST_SYMBOLS,)}


def _defaults():
    p = abi.RectifyParams()
    abi.rectify_lib().vimg_rectify_defaults(C.byref(p))
    return p


def _exports(name):
    lib = os.path.join(ROOT, "v-img_amd", "lib", f"libvimg_{name}.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    return nm, sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("vimg_"))


# ---- 1. header and ctypes ------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_structs(tmp_path):
    structs = {"VimgRectifyFrames": abi.RectifyFrames, "VimgRectifyParams": abi.RectifyParams}
    got = c_layout(tmp_path, ["vimg_rectify.h"], structs,
                   'printf("codes %d %d\\n", VIMG_OK, VIMG_E_INVALID);'
                   'printf("what %u %u %u %u\\n", VIMG_RECTIFY_KEPT, VIMG_RECTIFY_CLAMPED, VIMG_RECTIFY_FEW_TAPS, VIMG_RECTIFY_NOT_LIVE);'
                   'printf("limits %u %u %u\\n", VIMG_RECTIFY_MAX_EXTENT, VIMG_RECTIFY_MAX_RADIUS, VIMG_RECTIFY_HISTORY_PER_PIXEL);')
    assert got.pop("codes 0") == str(INVALID)
    assert got.pop("what 0 1 2") == "3" and got.pop("limits 32768 3") == "48"
    assert (abi.RECTIFY_KEPT, abi.RECTIFY_CLAMPED, abi.RECTIFY_FEW_TAPS, abi.RECTIFY_NOT_LIVE) == (0, 1, 2, 3) \
        == (R.KEPT, R.CLAMPED, R.FEW_TAPS, R.NOT_LIVE)
    assert abi.RECTIFY_MAX_RADIUS == 3 and abi.TEMPORAL_HISTORY_PER_PIXEL == 48
    assert got == ctypes_layout(structs)
    assert C.sizeof(abi.RectifyFrames) == 40 and C.sizeof(abi.RectifyParams) == 36
    assert abi.RectifyFrames().struct_size == 40 and abi.RectifyParams().struct_size == 36
    assert [(f, getattr(abi.RectifyFrames, f).offset) for f, _ in abi.RectifyFrames._fields_] == \
        [("struct_size", 0), ("width", 4), ("height", 8), ("reserved", 12), ("slow", 16), ("fast", 24), ("albedo", 32)]
    assert [f for f, _ in abi.RectifyParams._fields_] == ["struct_size", "radius", "min_taps", "reserved", "k", "cut", "sigma_normal",
                                                         "sigma_plane", "albedo_floor"]


def test_the_workspace_is_nothing_and_the_defaults_are_valid():
    lib = abi.rectify_lib()
    for w, h in ((1, 1), (3, 5), (1800, 800), (32768, 32768), (0, 7), (0, 0)):
        assert lib.vimg_rectify_workspace(w, h) == 0
    p = _defaults()
    assert p.struct_size == C.sizeof(abi.RectifyParams) and p.reserved == 0
    assert 1 <= p.radius <= 3 and 1 <= p.min_taps <= (2 * p.radius + 1) ** 2
    assert 0 <= p.k and 0 <= p.cut <= 1
    # the sigmas and the floor are the a-trous filter's
    q = abi.AtrousParams()
    abi.filter_lib().vimg_filter_atrous_defaults(C.byref(q))
    assert (p.sigma_normal, p.sigma_plane, p.albedo_floor) == (q.sigma_normal, q.sigma_plane, q.albedo_floor)
    # the header names them
    header = open(os.path.join(ROOT, "include", "vimg_rectify.h")).read()
    assert f"radius {p.radius}, min_taps {p.min_taps}, k {p.k:g}, cut {p.cut:g}, sigma_normal 0.5, sigma_plane 0.005" in header
    # ... and they pass the call's own checks: with them the call gets as far as the launch
    import torch
    if not torch.cuda.is_available():
        rc, msg = _call(**_good_call())
        assert rc == -2 and "launch failed" in msg, (rc, msg)          # VIMG_E_DEVICE, no silent success


def test_the_library_exports_the_four_declared_names_and_leaves_the_other_libraries_alone():
    assert sorted(abi.RECTIFY_SYMBOLS) == EXPORTS
    assert "rectify" not in abi._LIBRARIES and "rectify" in abi._LATER_LIBRARIES
    assert not set(abi._LIBRARIES) & set(abi._LATER_LIBRARIES)
    lib = abi.rectify_lib()
    assert lib is abi.rectify_lib() and callable(lib.vimg_rectify_clamp)
    nm, have = _exports("rectify")
    assert have == EXPORTS
    assert any("rectify_clamp_kernel" in l for l in nm.splitlines())
    # the shared host skeleton (frames/frame_lib.h) is internal: no error slot and no helper of it is a dynamic symbol
    assert not [l for l in nm.splitlines() if any(w in l for w in ("g_error", "vimg_frames", "4fail", "last_errorEv", "check_", "overlaps"))]
    header = open(os.path.join(ROOT, "include", "vimg_rectify.h")).read()
    for name in abi.RECTIFY_SYMBOLS:
        assert name + "(" in header
    # the other libraries export what they exported - their symbol tables, and libvimg_hip.so its golden list - and share
    # no name with this one
    for name, tables in OTHERS.items():
        want = sorted(s for t in tables for s in t)
        assert _exports(name)[1] == want, name
        assert not set(abi.RECTIFY_SYMBOLS) & set(want)
    hip = open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read().split()
    assert _exports("hip")[1] == sorted(hip) and "rectify" not in " ".join(hip)
    assert not set(abi.RECTIFY_SYMBOLS) & (set(abi.HIP_SYMBOLS) | set(abi.HIP_TEST_SYMBOLS))
    # it links the HIP runtime and none of the project's libraries
    path = os.path.join(ROOT, "v-img_amd", "lib", "libvimg_rectify.so")
    needed = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libvimg" not in needed.replace("libvimg_rectify", "")


def test_the_module_and_the_source_directory_of_the_same_name_do_not_collide():
    import vimg_amd.rectify as rc
    assert rc.__file__.endswith("rectify.py") and callable(rc.clamp) and callable(rc.params) and rc.workspace(640, 480) == 0
    assert not [f for f in os.listdir(os.path.join(abi.PKG_DIR, "rectify")) if f.endswith(".py")]
    # guide_score and floored stay ONE definition: the unit includes frames/guides.h and defines neither
    unit = open(os.path.join(abi.PKG_DIR, "rectify", "rectify.hip")).read()
    assert '#include "../frames/guides.h"' in unit and '#include "../frames/frame_lib.h"' in unit
    for name in ("guide_score(const", "float floored("):
        assert name not in unit


def test_params_takes_two_integer_fields_and_refuses_what_does_not_fit():
    import vimg_amd.rectify as rc
    d, p = _defaults(), rc.params()
    assert all(getattr(p, k) == getattr(d, k) for k, _ in abi.RectifyParams._fields_)
    p = rc.params(radius=3, min_taps=9, k=float("inf"), cut=1, sigma_plane=0.25)
    assert (p.radius, p.min_taps, p.k, p.cut, p.sigma_plane, p.sigma_normal) == (3, 9, np.inf, 1.0, 0.25, d.sigma_normal)
    for kw, sentence in ((dict(radius=-1), "rectify: radius must be 1..3, not -1"),
                         (dict(min_taps=-1), "rectify: min_taps must be 1..(2 radius + 1)^2, not -1"),
                         (dict(min_taps=2 ** 32), "rectify: min_taps must be 1..(2 radius + 1)^2, not 4294967296")):
        with pytest.raises(ValueError) as e:
            rc.params(**kw)
        assert str(e.value) == sentence
    with pytest.raises(TypeError, match=r"rectify: unknown parameters \['gain'\]"):
        rc.params(gain=1.0)


def test_the_preview_refuses_a_rectify_it_cannot_use():
    from vimg_amd import preview
    assert preview.rectify_kw(None, "x") is None and preview.rectify_kw(False, "x") is None
    assert preview.rectify_kw(True, "x") == (preview.FAST_HISTORY, {})
    assert preview.rectify_kw(dict(fast_history=2, k=3), "x") == (2.0, dict(k=3))
    with pytest.raises(ValueError, match="preview: rectify must be None, a bool or a dict"):
        preview.rectify_kw(3, "preview")
    with pytest.raises(TypeError, match="rectify: unknown parameters"):
        preview.rectify_kw(dict(max_history=3), "preview")
    for bad in (0, 0.5, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="preview: rectify's fast_history must be >= 1 and finite"):
            preview.rectify_kw(dict(fast_history=bad), "preview")


# ---- 2. argument errors, found before anything is enqueued -------------------------------------------------------
W, H = 8, 4
FRAME, CODES, HIST = 12 * W * H, W * H, 48 * W * H


def _good_call():
    """Arguments vimg_rectify_clamp accepts up to the launch (the pointers are never read on the host)."""
    frames = abi.RectifyFrames(width=W, height=H, slow=0x10000, fast=0x20000, albedo=0x30000)
    return dict(frames=frames, params=_defaults(), out=0x40000, code=0x50000, workspace=None, nbytes=0)


def _call(frames, params, out, code, workspace, nbytes):
    lib = abi.rectify_lib()
    rc = lib.vimg_rectify_clamp(None if frames is None else C.byref(frames), None if params is None else C.byref(params),
                                C.c_void_p(out), C.c_void_p(code), C.c_void_p(workspace), nbytes, None)
    return rc, lib.vimg_rectify_last_error().decode()


def _edit(**kw):
    a = _good_call()
    for k, v in kw.items():
        if k in a:
            a[k] = v
        elif k in dict(abi.RectifyFrames._fields_):
            setattr(a["frames"], k, v)
        else:
            setattr(a["params"], k, v)
    return a


NAN, INF = float("nan"), float("inf")
ERRORS = [
    # check_head's, in its order
    (dict(frames=None), "null frames"), (dict(params=None), "null params"),
    (dict(struct_size=39), "frames.struct_size 39 is below the struct's 40"),
    (dict(width=0), "width and height must be 1..32768, not 0 x 4"), (dict(height=0), "width and height must be 1..32768, not 8 x 0"),
    (dict(width=32769), "width and height must be 1..32768, not 32769 x 4"),
    (dict(height=32769), "width and height must be 1..32768, not 8 x 32769"),
    (dict(slow=None), "null slow history"), (dict(fast=None), "null fast history"),
    # alignment
    (dict(slow=0x10008), "the slow history must be 16-byte aligned"), (dict(fast=0x20004), "the fast history must be 16-byte aligned"),
    (dict(albedo=0x30002), "the albedo frame must be 4-byte aligned"), (dict(out=0x40001), "the output must be 4-byte aligned"),
    # the parameters
    (dict(radius=0), "radius must be 1..3, not 0"), (dict(radius=4), "radius must be 1..3, not 4"),
    (dict(radius=1, min_taps=0), "min_taps must be 1..9, not 0"), (dict(radius=1, min_taps=10), "min_taps must be 1..9, not 10"),
    (dict(radius=2, min_taps=26), "min_taps must be 1..25, not 26"), (dict(radius=3, min_taps=50), "min_taps must be 1..49, not 50"),
    (dict(k=-0.5), "k must be >= 0 (it may be +inf), not -0.5"), (dict(k=NAN), "k must be >= 0 (it may be +inf), not nan"),
    (dict(k=-INF), "k must be >= 0 (it may be +inf), not -inf"),
    (dict(cut=-0.25), "cut must be 0..1, not -0.25"), (dict(cut=1.5), "cut must be 0..1, not 1.5"), (dict(cut=NAN), "cut must be 0..1, not nan"),
    (dict(sigma_normal=0.0), "sigma_normal must be > 0 and finite, not 0"), (dict(sigma_normal=-2.0), "sigma_normal must be > 0 and finite, not -2"),
    (dict(sigma_normal=NAN), "sigma_normal must be > 0 and finite, not nan"), (dict(sigma_normal=INF), "sigma_normal must be > 0 and finite, not inf"),
    (dict(sigma_plane=0.0), "sigma_plane must be > 0 and finite, not 0"), (dict(sigma_plane=-0.5), "sigma_plane must be > 0 and finite, not -0.5"),
    (dict(sigma_plane=NAN), "sigma_plane must be > 0 and finite, not nan"), (dict(sigma_plane=INF), "sigma_plane must be > 0 and finite, not inf"),
    (dict(albedo_floor=0.0), "albedo_floor must be > 0 and finite, not 0"), (dict(albedo_floor=-0.25), "albedo_floor must be > 0 and finite, not -0.25"),
    (dict(albedo_floor=NAN), "albedo_floor must be > 0 and finite, not nan"), (dict(albedo_floor=INF), "albedo_floor must be > 0 and finite, not inf"),
    # each forbidden overlap: the last byte of one buffer on the first of the other, and the other way round
    (dict(fast=0x10000), "the slow history overlaps the fast history"),
    (dict(fast=0x10000 + HIST - 16), "the slow history overlaps the fast history"),
    (dict(fast=0x10000 - HIST + 16), "the slow history overlaps the fast history"),
    (dict(albedo=0x10000 + HIST - 4), "the slow history overlaps the albedo frame"),
    (dict(albedo=0x10000 - FRAME + 4), "the slow history overlaps the albedo frame"),
    (dict(out=0x10000 + HIST - 4), "the output overlaps the slow history"), (dict(out=0x10000 - FRAME + 4), "the output overlaps the slow history"),
    (dict(out=0x20000), "the output overlaps the fast history"), (dict(out=0x20000 + HIST - 4), "the output overlaps the fast history"),
    (dict(out=0x30000 + 4), "the output overlaps the albedo frame"), (dict(out=0x30000 - FRAME + 4), "the output overlaps the albedo frame"),
    (dict(code=0x10000 + HIST - 1), "the output codes overlap the slow history"), (dict(code=0x10000 - CODES + 1), "the output codes overlap the slow history"),
    (dict(code=0x20000 + 7), "the output codes overlap the fast history"),
    (dict(code=0x30000 + FRAME - 1), "the output codes overlap the albedo frame"),
    (dict(code=0x40000 + FRAME - 1), "the output overlaps the output codes"), (dict(code=0x40000 - CODES + 1), "the output overlaps the output codes"),
]


@pytest.mark.parametrize("edit,sentence", ERRORS, ids=[f"{'-'.join(e)}-{i}" for i, (e, _) in enumerate(ERRORS)])
def test_argument_errors_are_invalid_with_their_sentence_and_need_no_device(edit, sentence):
    rc, msg = _call(**_edit(**edit))
    assert rc == INVALID and msg == "rectify: " + sentence, (rc, msg)


def test_the_checks_come_in_a_fixed_order():
    """Two faults at once: the one that comes first - check_head's order, the alignments, then radius, min_taps, k, cut, the
    two sigmas, the floor, the overlaps - is reported."""
    order = [dict(struct_size=39), dict(width=0), dict(fast=None), dict(slow=0x10004), dict(albedo=0x30001), dict(out=0x40002),
             dict(radius=9), dict(min_taps=0), dict(k=NAN), dict(cut=2.0), dict(sigma_normal=NAN), dict(sigma_plane=NAN),
             dict(albedo_floor=NAN), dict(code=0x10000)]
    sentences = ["frames.struct_size", "width and height", "null fast history", "the slow history must be", "the albedo frame must be",
                 "the output must be", "radius must be", "min_taps must be", "k must be", "cut must be", "sigma_normal must be",
                 "sigma_plane must be", "albedo_floor must be", "overlap the slow history"]
    for i in range(len(order) - 1):
        rc, msg = _call(**_edit(**order[i], **order[i + 1]))
        assert rc == INVALID and sentences[i] in msg, (i, msg)


def test_params_struct_size_and_what_may_be_null_or_touch():
    a = _good_call()
    a["params"].struct_size = 35
    rc, msg = _call(**a)
    assert rc == INVALID and msg == "rectify: params.struct_size 35 is below the struct's 36"
    # albedo, both outputs and the workspace may be NULL, a workspace that is given is not looked at, k may be +inf or 0,
    # and buffers may touch end to start: the call passes every argument check
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(albedo=None), dict(code=None), dict(out=None), dict(out=None, code=None), dict(workspace=0x10000, nbytes=64),
                   dict(k=INF), dict(k=0.0), dict(cut=0.0), dict(cut=1.0), dict(radius=3, min_taps=49), dict(radius=1, min_taps=9),
                   dict(fast=0x10000 + HIST), dict(fast=0x10000 - HIST), dict(out=0x10000 + HIST), dict(code=0x40000 + FRAME),
                   dict(albedo=0x10000 - FRAME)):
            rc, msg = _call(**_edit(**ok))
            assert rc == -2 and "launch failed" in msg, (ok, rc, msg)


# ---- 3. the restatement, pinned on its own against hand-computed cases ---------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# sigma_plane 0.125 at depth 8: the plane term's denominator is (0.125 * 8)^2 = 1
KW = dict(radius=1, min_taps=4, k=2, cut=0.5, sigma_normal=0.5, sigma_plane=0.125, albedo_floor=1 / 64)


def test_k_infinite_changes_no_bit():
    """On the synthetic histories - noise, a stale quarter, misses, NaN and inf colours - and on a constant fast history,
    where every variance is 0 and the bound is inf * 0 = NaN."""
    for slow, fast, albedo in (R.synthetic_histories(13, 21), R.flat_histories(6, 7, slow_rgb=9.0) + (None,)):
        for alb in (albedo, None):
            for radius in (1, 2, 3):
                plane, rgb, code = R.clamp(slow, fast, alb, **dict(KW, radius=radius, k=np.inf, min_taps=1))
                assert np.array_equal(_bits(plane), _bits(slow[0])) and np.array_equal(_bits(rgb), _bits(slow[0][..., :3]))
                assert not (code == R.CLAMPED).any() and (code == R.KEPT).any()


@pytest.mark.parametrize("with_albedo", [False, True])
def test_a_constant_fast_history_pulls_every_accepted_pixel_to_exactly_its_mean(with_albedo):
    """Fast colour 0.25 a~ everywhere, so F = 0.25 exactly (a~ a power of two), s1 = 0.25 m, s2 = 0.0625 m, mean = 0.25,
    v = 0, the bounds are 0.25 whatever k: a slow pixel at 0.5 a~ becomes exactly 0.25 a~, one at 0.25 a~ is kept."""
    h, w = 6, 7
    slow, fast = R.flat_histories(h, w)
    albedo = None
    a = np.ones((h, w, 3), F)
    if with_albedo:
        yy, xx = np.mgrid[0:h, 0:w]
        albedo = np.where(((xx + yy) % 2 == 0)[..., None], F(0.5), F(0.001)) * np.ones(3, F)     # the dark squares are floored
        a = np.where(albedo > F(1 / 64), albedo, F(1 / 64))
    fast[0, ..., :3] = F(0.25) * a
    slow[0, ..., :3] = F(0.5) * a
    slow[0, 2, 3, :3] = F(0.25) * a[2, 3]
    plane, rgb, code = R.clamp(slow, fast, albedo, **dict(KW, k=3))
    corners = np.zeros((h, w), bool)
    corners[::h - 1, ::w - 1] = True                    # four taps with the centre: min_taps 4 is just met
    want = np.ones((h, w), np.uint8)
    want[2, 3] = 0
    assert np.array_equal(code, want)
    assert np.array_equal(_bits(rgb), _bits((F(0.25) * a).astype(F))) and np.array_equal(_bits(plane[..., :3]), _bits(rgb))
    # the length: Ls 16, Lf 4, cut 0.5 -> 10 where clamped
    assert np.array_equal(plane[..., 3], np.where(want == 1, F(10), F(16)))
    # with min_taps 5 the corners are left alone
    plane, rgb, code = R.clamp(slow, fast, albedo, **dict(KW, k=3, min_taps=5))
    assert (code[corners] == R.FEW_TAPS).all() and np.array_equal(_bits(plane[corners]), _bits(slow[0][corners]))


def test_the_bounds_are_the_mean_and_k_deviations_of_the_window_centre_included():
    """3 x 3, coplanar, fast green 1..9 in tap order: at the centre m = 9, s1 = 45, s2 = 285, mean = 5, v = 285 / 9 - 25,
    w = k sqrt(v): a slow 100 comes down to mean + w, a slow 0 up to mean - w, a slow 5 stays; the other channels are
    constant 0: bounds 0 +- 0, not moved."""
    slow, fast = R.flat_histories(3, 3, slow_rgb=0.0, fast_rgb=0.0)
    fast[0, ..., 1] = np.arange(1, 10, dtype=F).reshape(3, 3)
    v = F(285) / F(9) - F(5) * F(5)
    wd = F(1.5) * np.sqrt(v)
    for H_, want_g, want_code in ((100, F(5) + wd, 1), (0, F(5) - wd, 1), (5, F(5), 0), (F(5) + wd, F(5) + wd, 0)):
        slow[0, 1, 1, 1] = H_
        plane, rgb, code = R.clamp(slow, fast, None, **dict(KW, k=1.5, min_taps=9))
        assert code[1, 1] == want_code and np.array_equal(_bits(rgb[1, 1]), _bits(np.array([0, want_g, 0], F)))
        assert (code[[0, 0, 2, 2, 0, 1, 1, 2], [0, 2, 0, 2, 1, 0, 2, 1]] == R.FEW_TAPS).all()       # six or four taps, under 9
    # (without the centre the mean would be 5 all the same, but the variance 260 / 8 - 25 = 7.5: the centre is in)
    assert float(v) == pytest.approx(285 / 9 - 25, rel=1e-5) and abs(float(v) - 7.5) > 0.5


def test_a_tap_behind_a_normal_or_a_plane_edge_is_not_accepted():
    """The column right of the centre holds a fast colour of 100, but faces +x (1 - n.n = 1, s_n = 2) or stands one unit
    off the centre's plane (s_p = 1, and S < 1 fails): the centre's box is the six pixels at 1, and a slow 1 is kept;
    without the edge the 100s are in the box, the bounds are wide, and a slow 50 is kept."""
    for edge in ("normal", "plane", None):
        slow, fast = R.flat_histories(5, 5, slow_rgb=1.0, fast_rgb=1.0)
        fast[0, :, 3, :3] = 100
        slow[0, 2, 2, :3] = 50
        if edge == "normal":
            slow[1, :, 3, :3] = (1, 0, 0)
        elif edge == "plane":
            slow[2, :, 3, 2] += F(1)
        plane, rgb, code = R.clamp(slow, fast, None, **KW)
        if edge is None:
            assert code[2, 2] == R.KEPT and np.array_equal(_bits(rgb[2, 2]), _bits(slow[0, 2, 2, :3]))
        else:
            assert code[2, 2] == R.CLAMPED and np.array_equal(rgb[2, 2], np.ones(3, F))
            # the column itself accepts its own three (at the ends: two) pixels only: fewer than min_taps, untouched
            assert (code[:, 3] == R.FEW_TAPS).all() and np.array_equal(_bits(plane[:, 3]), _bits(slow[0][:, 3]))


def test_few_taps_misses_and_pixels_without_a_slow_history_are_untouched():
    slow, fast = R.flat_histories(4, 5, slow_rgb=7.0, fast_rgb=1.0)
    slow[1, 0, 0, 3] = 0             # a miss
    slow[1, 0, 1, 3] = np.nan        # a NaN depth
    slow[0, 3, 4, 3] = 0             # no slow history
    fast[0, 2, 0:3, 3] = 0           # three pixels without a fast history
    plane, rgb, code = R.clamp(slow, fast, None, **dict(KW, min_taps=6))
    assert code[0, 0] == code[0, 1] == code[3, 4] == R.NOT_LIVE
    # (3, 1): six cells inside the image, three of them without a fast history: m = 3
    assert code[3, 1] == R.FEW_TAPS and code[1, 3] == R.CLAMPED
    keep = code != R.CLAMPED
    assert np.array_equal(_bits(plane[keep]), _bits(slow[0][keep])) and np.array_equal(_bits(rgb[keep]), _bits(slow[0][..., :3][keep]))
    # a pixel without a fast history of its own is clamped by its neighbours' and keeps its length
    assert code[2, 1] == R.CLAMPED and plane[2, 1, 3] == 16 and np.array_equal(rgb[2, 1], np.ones(3, F))
    # a miss is no tap: (1, 1) has nine cells, a miss, a NaN depth and three without a fast history: four are left
    assert code[1, 1] == R.FEW_TAPS
    assert R.clamp(slow, fast, None, **dict(KW, min_taps=4))[2][1, 1] == R.CLAMPED
    assert R.clamp(slow, fast, None, **dict(KW, min_taps=5))[2][1, 1] == R.FEW_TAPS


@pytest.mark.parametrize("cut,want", [(0.0, 16.0), (0.5, 10.0), (1.0, 4.0)])
def test_the_length_rule(cut, want):
    slow, fast = R.flat_histories(5, 5, slow_rgb=7.0, fast_rgb=1.0)
    fast[0, 2, 2, 3] = 20            # a fast history longer than the slow one: the length stays
    fast[0, 1, 1, 3] = 16            # as long: stays
    slow[0, 3, 3, :3] = 1            # not moved: every bit stays
    plane, rgb, code = R.clamp(slow, fast, None, **dict(KW, cut=cut))
    assert code[3, 3] == R.KEPT and np.array_equal(_bits(plane[3, 3]), _bits(slow[0, 3, 3]))
    assert code[2, 2] == code[1, 1] == code[0, 4] == R.CLAMPED
    assert plane[2, 2, 3] == 16 and plane[1, 1, 3] == 16 and plane[0, 4, 3] == F(want) and plane[2, 3, 3] == F(want)


def test_a_nan_or_infinite_fast_colour_poisons_only_the_boxes_it_enters_and_those_pixels_are_kept():
    for bad in (np.nan, np.inf, -np.inf):
        slow, fast = R.flat_histories(7, 7, slow_rgb=7.0, fast_rgb=1.0)
        fast[0, 3, 3, 1] = bad
        plane, rgb, code = R.clamp(slow, fast, None, **KW)
        box = np.zeros((7, 7), bool)
        box[2:5, 2:5] = True
        # green is poisoned in the box, red and blue still move: clamped, with green kept as it was
        assert (code == R.CLAMPED).all()
        assert np.array_equal(rgb[box], np.tile(np.array([1, 7, 1], F), (9, 1))) and np.array_equal(rgb[~box], np.ones((40, 3), F))
        slow[0, ..., 0] = slow[0, ..., 2] = 1
        plane, rgb, code = R.clamp(slow, fast, None, **KW)
        assert (code[box] == R.KEPT).all() and (code[~box] == R.CLAMPED).all()
        assert np.array_equal(_bits(plane[box]), _bits(slow[0][box]))
