"""The anti-lag library at its boundary, without a GPU: include/vimg_antilag.h against its ctypes mirror, the exports of
libvimg_antilag.so and of the other libraries, every argument error of vimg_antilag_rescale with its whole sentence,
and the numpy restatement of its contract (tests/antilag_ref.py) pinned on its own against cases worked out by hand
and two statistical ones with fixed seeds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import antilag_ref as R
import temporal_ref as TR
from abi_layout import c_layout, ctypes_layout
from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # VIMG_E_INVALID
F = np.float32
EXPORTS = ["vimg_antilag_defaults", "vimg_antilag_last_error", "vimg_antilag_rescale", "vimg_antilag_workspace_bytes"]
# the other libraries' vimg_* exports, as they were before this one: the symbol tables their own ABI tests pin
OTHERS = {"filter": (abi.FILTER_SYMBOLS,), "temporal": (abi.TEMPORAL_SYMBOLS,), "varfilter": (abi.VARFILTER_SYMBOLS,),
          "moments": (abi.MOMENTS_SYMBOLS,), "infill": (abi.INFILL_SYMBOLS,), "wtemporal": (abi.WTEMPORAL_SYMBOLS,),
          "host": (abi.HOST_SYMBOLS,)}
TEMPORAL_SIGMAS = dict(sigma_normal=0.1, sigma_plane=0.00005)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _defaults():
    p = abi.AntilagParams()
    abi.antilag_lib().vimg_antilag_defaults(C.byref(p))
    return p


def _exports(name):
    lib = os.path.join(ROOT, "v-img_amd", "lib", f"libvimg_{name}.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    return nm, sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("vimg_"))


# ---- 1. header and ctypes ------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_structs(tmp_path):
    structs = {"VimgAntilagFrames": abi.AntilagFrames, "VimgAntilagParams": abi.AntilagParams}
    got = c_layout(tmp_path, ["vimg_antilag.h"], structs,
                   'printf("limits %u %u %u\\n", VIMG_ANTILAG_MAX_EXTENT, VIMG_ANTILAG_MAX_RADIUS, VIMG_ANTILAG_HISTORY_PER_PIXEL);'
                   'printf("workspace %u\\n", VIMG_ANTILAG_WORKSPACE_PER_PIXEL);')
    assert got.pop("limits 32768 8") == "48" == str(abi.TEMPORAL_HISTORY_PER_PIXEL)
    assert got.pop("workspace") == "8" == str(abi.ANTILAG_WORKSPACE_PER_PIXEL) and abi.ANTILAG_MAX_RADIUS == 8
    assert got == ctypes_layout(structs)
    assert C.sizeof(abi.AntilagFrames) == 48 and C.sizeof(abi.AntilagParams) == 28
    assert abi.AntilagFrames().struct_size == 48 and abi.AntilagParams().struct_size == 28
    # the shared eight fields, where frame_lib.h's check_head and hip.FrameCall expect them, and nothing after them
    shared = ("struct_size", "width", "height", "reserved", "color", "normal", "position", "depth")
    assert [f for f, _ in abi.AntilagFrames._fields_] == list(shared)
    assert [got[f"VimgAntilagFrames.{f}"] for f in shared] == ["0", "4", "8", "12", "16", "24", "32", "40"]
    assert [getattr(abi.AntilagFrames, f).offset for f in shared] == [getattr(abi.TemporalFrames, f).offset for f in shared]
    assert [f for f, _ in abi.AntilagParams._fields_] == ["struct_size", "radius", "t_low", "t_high", "min_matches", "sigma_normal",
                                                          "sigma_plane"]


def test_the_workspace_is_8_bytes_per_pixel_and_the_defaults_are_valid():
    lib = abi.antilag_lib()
    for w, h in ((1, 1), (3, 5), (1800, 800), (32768, 32768), (0, 7), (0, 0)):
        assert lib.vimg_antilag_workspace_bytes(w, h) == 8 * w * h
    p, q = _defaults(), abi.TemporalParams()
    abi.temporal_lib().vimg_temporal_defaults(C.byref(q))
    assert p.struct_size == C.sizeof(abi.AntilagParams) and 1 <= p.radius <= 8
    assert 0 < p.t_low < p.t_high < np.inf and 2 <= p.min_matches < np.inf
    assert (p.sigma_normal, p.sigma_plane) == (q.sigma_normal, q.sigma_plane)          # the same-surface test of vimg_temporal.h
    # the restatement's defaults are the library's
    assert R.DEFAULTS == {k: pytest.approx(getattr(p, k)) for k, _ in abi.AntilagParams._fields_ if k != "struct_size"}
    # ... and the call takes them.  Its pointers are made up, so it is only made where no device could follow them:
    # there it passes every argument check and fails at the launch
    import torch
    if not torch.cuda.is_available():
        rc, msg = _call(**_good_call())
        assert rc == -2 and "launch failed" in msg, (rc, msg)          # VIMG_E_DEVICE, no silent success


def test_the_library_exports_the_four_declared_names_and_leaves_the_other_libraries_alone():
    assert sorted(abi.ANTILAG_SYMBOLS) == EXPORTS
    abi.antilag_lib()                    # loads on a machine without a GPU
    nm, have = _exports("antilag")
    assert have == EXPORTS
    for kernel in ("pair", "scale"):
        assert any(f"antilag_{kernel}_kernel" in l for l in nm.splitlines()), kernel
    # the shared host skeleton (frames/frame_lib.h) is internal: no error slot and no helper of it is a dynamic symbol
    assert not [l for l in nm.splitlines() if any(w in l for w in ("g_error", "vimg_frames", "4fail", "last_errorEv", "check_", "overlaps"))]
    header = open(os.path.join(ROOT, "include", "vimg_antilag.h")).read()
    for name in abi.ANTILAG_SYMBOLS:
        assert name + "(" in header
    # the other seven libraries export what they exported: their symbol tables, and libvimg_hip.so its golden list
    for name, tables in OTHERS.items():
        want = sorted(s for t in tables for s in t)
        assert _exports(name)[1] == want, name
        assert not set(abi.ANTILAG_SYMBOLS) & set(want)
    hip = open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read().split()
    assert _exports("hip")[1] == sorted(hip) and "antilag" not in " ".join(hip)
    assert sorted(abi._LIBRARIES) == sorted(["antilag", "hip", *OTHERS])
    # it links the HIP runtime and none of the project's libraries
    lib = os.path.join(ROOT, "v-img_amd", "lib", "libvimg_antilag.so")
    needed = subprocess.run(["readelf", "-d", lib], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libvimg" not in needed.replace("libvimg_antilag", "")


def test_the_module_and_the_source_directory_of_the_same_name_do_not_collide():
    import vimg_amd.antilag as al
    assert al.__file__.endswith("antilag.py") and callable(al.rescale) and callable(al.antilag_params)
    assert not [f for f in os.listdir(os.path.join(abi.PKG_DIR, "antilag")) if f.endswith(".py")]
    p = al.antilag_params(radius=2, t_low=2.5)
    assert (p.radius, p.t_low, p.t_high) == (2, 2.5, _defaults().t_high)
    with pytest.raises(TypeError, match="antilag: unknown parameters"):
        al._params(None, dict(max_history=3).items())
    with pytest.raises(ValueError, match="antilag: radius must be 1..8"):
        al.antilag_params(radius=-1)


# ---- 2. argument errors, found before anything is enqueued -------------------------------------------------------
W, H = 8, 4
FRAME, PLANE, HIST, WORK = 12 * W * H, 4 * W * H, 48 * W * H, 8 * W * H


def _good_call():
    """Arguments vimg_antilag_rescale accepts up to the launch (the device pointers are never read on the host)."""
    frames = abi.AntilagFrames(width=W, height=H, color=0x1000, normal=0x2000, position=0x3000, depth=0x4000)
    return dict(frames=frames, matrix=TR.IDENTITY.tolist(), history=0x10000, params=_defaults(), workspace=0x20000, nbytes=WORK,
                scale=0x6000)


def _call(frames, matrix, history, params, workspace, nbytes, scale):
    lib = abi.antilag_lib()
    m = None if matrix is None else (abi.f32 * 12)(*matrix)
    rc = lib.vimg_antilag_rescale(None if frames is None else C.byref(frames), m, C.c_void_p(history),
                                  None if params is None else C.byref(params), C.c_void_p(workspace), nbytes, C.c_void_p(scale),
                                  None)
    return rc, lib.vimg_antilag_last_error().decode()


def _edit(**kw):
    a = _good_call()
    for k, v in kw.items():
        if k.startswith("m") and k[1:].isdigit():
            a["matrix"][int(k[1:])] = v
        elif k in a:
            a[k] = v
        elif k in dict(abi.AntilagFrames._fields_):
            setattr(a["frames"], k, v)
        else:
            assert k in dict(abi.AntilagParams._fields_), k
            setattr(a["params"], k, v)
    return a


NAN, INF = float("nan"), float("inf")
ERRORS = [
    # check_head's, in its order
    (dict(frames=None), "antilag: null frames"), (dict(params=None), "antilag: null params"),
    (dict(struct_size=47), "antilag: frames.struct_size 47 is below the struct's 48"),
    (dict(width=0), "antilag: width and height must be 1..32768, not 0 x 4"),
    (dict(height=0), "antilag: width and height must be 1..32768, not 8 x 0"),
    (dict(width=32769), "antilag: width and height must be 1..32768, not 32769 x 4"),
    (dict(height=32769), "antilag: width and height must be 1..32768, not 8 x 32769"),
    (dict(color=None), "antilag: null color frame"), (dict(normal=None), "antilag: null normal frame"),
    (dict(position=None), "antilag: null position frame"), (dict(depth=None), "antilag: null depth frame"),
    # each parameter's range
    (dict(radius=0), "antilag: radius must be 1..8, not 0"), (dict(radius=9), "antilag: radius must be 1..8, not 9"),
    (dict(t_low=0.0), "antilag: t_low must be > 0 and finite, not 0"),
    (dict(t_low=-1.0), "antilag: t_low must be > 0 and finite, not -1"),
    (dict(t_low=NAN), "antilag: t_low must be > 0 and finite, not nan"),
    (dict(t_low=INF), "antilag: t_low must be > 0 and finite, not inf"),
    (dict(t_low=3.0, t_high=3.0), "antilag: t_high must be > 3 and finite, not 3"),
    (dict(t_low=3.0, t_high=2.5), "antilag: t_high must be > 3 and finite, not 2.5"),
    (dict(t_low=1.5, t_high=1.25), "antilag: t_high must be > 1.5 and finite, not 1.25"),
    (dict(t_low=3.0, t_high=NAN), "antilag: t_high must be > 3 and finite, not nan"),
    (dict(t_low=3.0, t_high=INF), "antilag: t_high must be > 3 and finite, not inf"),
    (dict(min_matches=1.5), "antilag: min_matches must be >= 2 and finite, not 1.5"),
    (dict(min_matches=NAN), "antilag: min_matches must be >= 2 and finite, not nan"),
    (dict(min_matches=INF), "antilag: min_matches must be >= 2 and finite, not inf"),
    (dict(sigma_normal=0.0), "antilag: sigma_normal must be > 0 and finite, not 0"),
    (dict(sigma_normal=NAN), "antilag: sigma_normal must be > 0 and finite, not nan"),
    (dict(sigma_normal=INF), "antilag: sigma_normal must be > 0 and finite, not inf"),
    (dict(sigma_plane=-0.5), "antilag: sigma_plane must be > 0 and finite, not -0.5"),
    (dict(sigma_plane=NAN), "antilag: sigma_plane must be > 0 and finite, not nan"),
    (dict(sigma_plane=INF), "antilag: sigma_plane must be > 0 and finite, not inf"),
    # the matrix, the history, the workspace, the scale output
    (dict(matrix=None), "antilag: null world-to-pixel matrix"),
    (dict(m0=NAN), "antilag: world-to-pixel entry 0 is not finite (nan)"),
    (dict(m7=INF), "antilag: world-to-pixel entry 7 is not finite (inf)"),
    (dict(m11=-INF), "antilag: world-to-pixel entry 11 is not finite (-inf)"),
    (dict(history=None), "antilag: null history"),
    (dict(history=0x10008), "antilag: the history must be 16-byte aligned"),
    (dict(workspace=None), "antilag: null workspace"),
    (dict(nbytes=WORK - 1), "antilag: the workspace has 255 bytes, 8 x 4 needs 256"),
    (dict(workspace=0x20008), "antilag: the workspace must be 16-byte aligned"),
    (dict(scale=0x6002), "antilag: the scale output must be 4-byte aligned"),
    # each forbidden overlap: the last bytes of one buffer on the first of the other, and the other way round
    (dict(history=0x1000), "antilag: the history overlaps the color frame"),
    (dict(history=0x1000 + FRAME - 16), "antilag: the history overlaps the color frame"),
    (dict(history=0x2000 - HIST + 16, color=0x40000), "antilag: the history overlaps the normal frame"),
    (dict(history=0x3000, color=0x40000, normal=0x41000), "antilag: the history overlaps the position frame"),
    (dict(history=0x4000 + FRAME - 16), "antilag: the history overlaps the depth frame"),
    (dict(workspace=0x10000 + HIST - 16), "antilag: the workspace overlaps the history"),
    (dict(workspace=0x10000 - WORK + 16), "antilag: the workspace overlaps the history"),
    (dict(workspace=0x1000 + FRAME - 16), "antilag: the workspace overlaps the color frame"),
    (dict(workspace=0x2000 - WORK + 16, color=0x40000), "antilag: the workspace overlaps the normal frame"),
    (dict(workspace=0x3000), "antilag: the workspace overlaps the position frame"),
    (dict(workspace=0x4000 + FRAME - 16), "antilag: the workspace overlaps the depth frame"),
    (dict(scale=0x10000 + HIST - 4), "antilag: the scale output overlaps the history"),
    (dict(scale=0x10000 - PLANE + 4), "antilag: the scale output overlaps the history"),
    (dict(scale=0x1000), "antilag: the scale output overlaps the color frame"),
    (dict(scale=0x2000 + FRAME - 4), "antilag: the scale output overlaps the normal frame"),
    (dict(scale=0x3000 - PLANE + 4), "antilag: the scale output overlaps the position frame"),
    (dict(scale=0x4000 + 4), "antilag: the scale output overlaps the depth frame"),
    (dict(scale=0x20000 + WORK - 4), "antilag: the scale output overlaps the workspace"),
    (dict(scale=0x20000 - PLANE + 4), "antilag: the scale output overlaps the workspace"),
]


@pytest.mark.parametrize("edit,sentence", ERRORS, ids=[f"{'-'.join(e)}-{i}" for i, (e, _) in enumerate(ERRORS)])
def test_argument_errors_are_invalid_with_their_whole_sentence_and_need_no_device(edit, sentence):
    rc, msg = _call(**_edit(**edit))
    assert rc == INVALID and msg == sentence, (rc, msg)


def test_the_checks_come_in_a_fixed_order():
    """Two faults at once: the one that comes first - check_head's order, each parameter, the matrix, the history, the
    workspace, the scale output, the overlaps - is reported."""
    order = [dict(struct_size=47), dict(width=0), dict(depth=None), dict(radius=0), dict(t_low=NAN), dict(t_high=1.0),
             dict(min_matches=0.0), dict(sigma_normal=NAN), dict(sigma_plane=NAN), dict(matrix=None), dict(history=None),
             dict(workspace=None), dict(scale=0x6001), dict(history=0x4000)]
    sentences = ["frames.struct_size", "width and height", "null depth frame", "radius must be", "t_low must be", "t_high must be",
                 "min_matches must be", "sigma_normal must be", "sigma_plane must be", "null world-to-pixel matrix", "null history",
                 "null workspace", "the scale output must be", "the history overlaps the depth frame"]
    for i in range(len(order) - 1):
        for j in range(i + 1, len(order)):
            if set(order[i]) & set(order[j]):
                continue
            rc, msg = _call(**_edit(**order[i], **order[j]))
            assert rc == INVALID and sentences[i] in msg, (i, j, msg)
    # within the groups: a non-finite entry after a null matrix, alignment after null, size before alignment, and the
    # overlaps in the order history, workspace, scale output
    for first, second, says in ((dict(m3=NAN), dict(history=0x10004), "entry 3"), (dict(history=0x10004), dict(nbytes=1), "the history must be"),
                                (dict(nbytes=1), dict(workspace=0x20004), "the workspace has"),
                                (dict(workspace=0x20004), dict(scale=0x6001), "the workspace must be"),
                                (dict(history=0x1000), dict(workspace=0x2000), "the history overlaps the color"),
                                (dict(workspace=0x2000), dict(scale=0x3000), "the workspace overlaps the normal"),
                                (dict(workspace=0x10000), dict(scale=0x10000), "the workspace overlaps the history")):
        rc, msg = _call(**_edit(**first, **second))
        assert rc == INVALID and says in msg, (first, second, msg)


def test_params_struct_size_the_slot_of_its_own_and_what_is_not_an_error():
    a = _good_call()
    a["params"].struct_size = 27
    rc, msg = _call(**a)
    assert rc == INVALID and msg == "antilag: params.struct_size 27 is below the struct's 28"
    # the last-error slot is this library's: a failure of libvimg_temporal leaves it alone, and the other way round
    import test_temporal_abi as TA
    tmp, lag = abi.temporal_lib(), abi.antilag_lib()
    fail_a = lambda: _call(**_edit(min_matches=0.25))
    fail_t = lambda: TA._call(**TA._edit(sigma_plane=-3.0))
    for first, second in ((fail_a, fail_t), (fail_t, fail_a)):
        assert first()[0] == INVALID and second()[0] == INVALID
        assert lag.vimg_antilag_last_error().decode() == "antilag: min_matches must be >= 2 and finite, not 0.25"
        assert tmp.vimg_temporal_last_error().decode() == "temporal: sigma_plane must be > 0 and finite, not -3"
    # no scale output, buffers that touch end to start, the extreme radii: all pass every argument check (and only
    # then need a device)
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(scale=None), dict(workspace=0x10000 + HIST), dict(scale=0x10000 - PLANE), dict(history=0x4000 + FRAME),
                   dict(radius=1), dict(radius=8), dict(min_matches=2.0)):
            rc, msg = _call(**_edit(**ok))
            assert rc == -2 and "launch failed" in msg, (ok, rc, msg)          # VIMG_E_DEVICE, no silent success


# ---- 3. the restatement, pinned on its own -----------------------------------------------------------------------
def history_of(frames, length=8.0, planes=3):
    """The history a first accumulate of ``frames`` leaves (tests/temporal_ref.py), its live lengths set to ``length``;
    with ``planes`` = 4 a plane M of made-up moments follows."""
    hist = TR.accumulate(frames["color"], frames["normal"], frames["position"], frames["depth"], None, None, max_history=32,
                         current_weight=1, **TEMPORAL_SIGMAS)
    hist[0, ..., 3] = np.where(hist[0, ..., 3] > 0, F(length), hist[0, ..., 3])
    if planes == 4:
        h, w = hist.shape[1:3]
        m = np.arange(h * w * 4, dtype=F).reshape(1, h, w, 4) / F(7)
        hist = np.concatenate([hist, m], axis=0)
    return hist


def grey_case(h, w, history_grey=1.0, sigma=0.0, left=1.0, seed=1):
    """The flat wall: history ``history_grey``; current = history times ``left`` on the left half (columns < w // 2),
    plus Gaussian noise of ``sigma``."""
    hist = history_of(TR.flat_frames(h, w, history_grey))
    cur = TR.flat_frames(h, w, history_grey)
    cur["color"][:, : w // 2] *= F(left)
    if sigma:
        cur["color"] += np.random.default_rng(seed).normal(0.0, sigma, size=(h, w, 1)).astype(F)
    return cur, hist


def _rescale(cur, hist, matrix=TR.IDENTITY, **kw):
    return R.rescale(cur["color"], cur["normal"], cur["position"], cur["depth"], hist, matrix, **kw)


@pytest.mark.parametrize("shift", [0.0, 2.0, -3.0], ids=["identity", "right2", "left3"])
def test_an_unchanged_constant_picture_keeps_every_length_and_every_byte(shift):
    cur, hist = grey_case(9, 13, 0.625)
    cur["position"][..., 0] -= F(shift)          # the camera moved: what pixel x now shows, pixel x - shift showed
    out, s = _rescale(cur, hist, TR.shift_matrix(shift))
    assert np.array_equal(s, np.ones((9, 13), F)) and np.array_equal(_bits(out), _bits(hist))
    d, v = R.pairs(cur["color"], cur["normal"], cur["position"], cur["depth"], hist, TR.shift_matrix(shift), **R.DEFAULTS)
    assert not d.any() and v.sum() == 9 * (13 - abs(int(shift)))          # the columns that left the picture have no pair


@pytest.mark.parametrize("radius", [1, 3])
def test_a_noise_free_change_drops_inside_keeps_outside_and_ramps_between(radius):
    """The left half changed colour, no noise: a window wholly inside it has var = 0, t2 = x / 0 = inf, s = 0; a window
    wholly outside has 0 / 0 = NaN, s = 1; a window across the edge has a variance and lands anywhere in [0, 1]."""
    h, w = 11, 20
    cur, hist = grey_case(h, w, 0.5, left=0.25)
    out, s = _rescale(cur, hist, radius=radius, min_matches=2)
    x = np.arange(w)
    assert (s[:, x < w // 2 - radius] == 0).all() and (s[:, x >= w // 2 + radius] == 1).all()
    assert ((s >= 0) & (s <= 1)).all()
    assert np.array_equal(out[0, ..., 3], hist[0, ..., 3] * s)
    keep = np.ones(hist.shape, bool)
    keep[0, ..., 3] = False
    assert np.array_equal(_bits(out)[keep], _bits(hist)[keep])          # only the lengths were written


def test_surfaces_that_left_the_picture_or_became_hidden_are_no_pairs():
    """tests/temporal_ref.py's sequence: the camera moves right, the wall 1 px and the box 2 px per frame to the left.  A
    history pixel of frame i - 1 is a pair in frame i exactly when it was hit, still projects inside the picture and
    the current pixel there shows the same surface - not the box, when the history pixel is wall."""
    seq = TR.synthetic_sequence(16, 32, frames=3)
    for i in (1, 2):
        old, cur = seq[i - 1], seq[i]
        hist = history_of(old)
        d, v = R.pairs(cur["color"], cur["normal"], cur["position"], cur["depth"], hist, cur["matrix"], **R.DEFAULTS)
        yy, xx = np.mgrid[0:16, 0:32]
        to = xx - np.where(old["box"], 2, 1)                            # where the history pixel's surface is now
        inside = to >= 0
        same = inside & old["hit"] & (cur["box"][yy, np.where(inside, to, 0)] == old["box"])
        assert np.array_equal(v == 1, same)
        assert (v[~old["hit"]] == 0).all() and (v[:, 0] == 0).all()      # misses; the column that left
        hidden = old["hit"] & ~old["box"] & inside & cur["box"][yy, np.where(inside, to, 0)]
        assert hidden.any() and (v[hidden] == 0).all()                  # wall the box now covers
        assert (d[v == 0] == 0).all()


def test_min_matches_and_the_nan_rules():
    h, w = 5, 5
    cur, hist = grey_case(h, w, 0.5, left=0.0)
    cur["color"][...] = F(0.25)                                        # everything changed, noise-free: drop ...
    out, s = _rescale(cur, hist, radius=1, min_matches=4)
    assert (s == 0).all() and (out[0, ..., 3] == 0).all()
    # ... unless the window has too few pairs: a corner's 2 x 2 window has 4, an edge's 6, the inside 9
    out, s = _rescale(cur, hist, radius=1, min_matches=5)
    corner = np.zeros((h, w), bool)
    corner[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    assert (s[corner] == 1).all() and (s[~corner] == 0).all()
    out, s = _rescale(cur, hist, radius=1, min_matches=9.5)
    assert (s == 1).all() and np.array_equal(_bits(out), _bits(hist))
    # a NaN colour, a NaN history colour, a NaN normal, a NaN position, a dead current pixel: no pair each
    for where, plane in (("color", None), ("normal", None), ("position", None), ("depth", None), (None, 0), (None, 1), (None, 2)):
        cur, hist = grey_case(h, w, 0.5)
        cur["color"][...] = F(0.25)
        if where == "depth":
            cur["depth"][2, 2] = 0
        elif where:
            cur[where][2, 2, 0] = np.nan
        else:
            hist[plane, 2, 2, 0] = np.nan
        d, v = R.pairs(cur["color"], cur["normal"], cur["position"], cur["depth"], hist, TR.IDENTITY, **R.DEFAULTS)
        assert v[2, 2] == 0 and d[2, 2] == 0 and v.sum() == h * w - 1, (where, plane)
        out, s = _rescale(cur, hist, radius=1, min_matches=2)
        assert np.isfinite(s).all() and (s == 0).all()                  # the other eight pairs of each window still say "drop"
    # a pixel without history is no pair, is not written, and has the scale of its window all the same
    cur, hist = grey_case(h, w, 0.5)
    hist[0, 1, 1, 3], hist[0, 3, 3, 3] = 0, np.nan
    out, s = _rescale(cur, hist, radius=1, min_matches=2)
    assert (s == 1).all() and np.array_equal(_bits(out), _bits(hist))
    # +inf in the current colour: d is inf, d - d is NaN: no pair
    cur["color"][0, 0, 1] = np.inf
    d, v = R.pairs(cur["color"], cur["normal"], cur["position"], cur["depth"], hist, TR.IDENTITY, **R.DEFAULTS)
    assert v[0, 0] == 0 and d[0, 0] == 0


def test_the_ramp_by_hand_on_one_by_two():
    """1 x 2, radius 1, min_matches 2: d = (1, 3) times lum's weight sum g = lum(1, 1, 1), both windows hold both pairs.
    sd = 4 g, sq = 10 g^2, c = 2: m = 2 g, var = (10 g^2 - 8 g^2) / 1 = 2 g^2, t2 = 4 g^2 / (g^2) = 4 up to rounding - between
    t_low = 1 and t_high = 3: s = (9 - t2) / 8."""
    cur, hist = grey_case(1, 2, 0.0)
    hist[0, ..., :3] = 0
    cur["color"][0, 0], cur["color"][0, 1] = 1, 3
    out, s = _rescale(cur, hist, radius=1, min_matches=2, t_low=1, t_high=3)
    kr, kg, kb = F(0.212671), F(0.715160), F(0.072169)
    d0, d1 = ((kr + kg) + kb) - F(0), ((F(3) * kr + F(3) * kg) + F(3) * kb) - F(0)
    sd, sq, c = (F(0) + d0) + d1, (F(0) + d0 * d0) + d1 * d1, F(2)
    m = sd / c
    var = (sq - sd * m) / (c - F(1))
    t2 = (m * m) / (var / c)
    want = (F(9) - t2) / (F(9) - F(1))
    assert abs(float(t2) - 4.0) < 1e-5 and np.array_equal(_bits(s), _bits(np.full((1, 2), want, F)))
    assert np.array_equal(_bits(out[0, ..., 3]), _bits(F(8) * s))


# ---- 4. two statistical cases with caps: the seeds are fixed, the figures are the restatement's ----------------------
NOISY = dict(radius=4, t_low=3.0, t_high=6.0, min_matches=8.0)


@pytest.mark.parametrize("size", [(64, 64), (9, 130)], ids=["64x64", "130x9"])
def test_noise_alone_touches_at_most_two_percent_of_the_pixels(size):
    """History 1.0 grey, current = history + N(0, 0.5): the share of pixels with s < 1 is the false-alarm rate of a
    two-sided test at t = 3 with up to 80 degrees of freedom, a few tenths of a percent.  Seed 1: 15 of 4096 at 64 x 64
    (0.37 %), 4 of 1170 at 130 x 9 (0.34 %)."""
    h, w = size
    cur, hist = grey_case(h, w, 1.0, sigma=0.5, seed=1)
    out, s = _rescale(cur, hist, **NOISY)
    share = float((s < 1).mean())
    print(f"{w} x {h}: {int((s < 1).sum())} of {h * w} pixels have s < 1 ({share:.4%})")
    assert share <= 0.02


@pytest.mark.parametrize("size", [(64, 64), (9, 130)], ids=["64x64", "130x9"])
def test_a_halved_left_half_is_dropped_under_the_same_noise(size):
    """... and with the current picture halved on the left half, at least 95 % of the pixels more than `radius` inside it
    have s == 0: the mean difference is 0.5 = 1 sigma, 9 standard errors of a full window's 81 pairs (6.7 of the 45 a window at the picture's top or
    bottom row has).  Seed 1: 99.55 % at 64 x 64, 97.45 % at 130 x 9."""
    h, w = size
    cur, hist = grey_case(h, w, 1.0, sigma=0.5, left=0.5, seed=1)
    out, s = _rescale(cur, hist, **NOISY)
    inside = s[:, : w // 2 - NOISY["radius"]]
    share = float((inside == 0).mean())
    print(f"{w} x {h}: {share:.4%} of the {inside.size} pixels more than {NOISY['radius']} inside the changed half have s == 0")
    assert share >= 0.95
