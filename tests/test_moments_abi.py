"""The moments library at its boundary, without a GPU: include/vimg_moments.h against its ctypes mirror, the exports of
libvimg_moments.so, every argument error of vimg_moments_accumulate with its whole sentence, and the numpy restatement
of its contract (tests/moments_ref.py) pinned on its own: planes 0..2 against tests/temporal_ref.py bit for bit, plane
M against closed forms, and its variance against the spread of the accumulated luminance itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import moments_ref as R
import temporal_ref as T
from abi_layout import c_layout, ctypes_layout
from test_temporal import EXPLICIT, matrices, random_case
from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # VIMG_E_INVALID
F = np.float32
EXPORTS = ["vimg_moments_accumulate", "vimg_moments_defaults", "vimg_moments_history_bytes", "vimg_moments_last_error"]
PARAMS = dict(max_history=32, current_weight=1, sigma_normal=0.1, sigma_plane=0.01, min_history=4)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _defaults():
    p = abi.MomentsParams()
    abi.moments_lib().vimg_moments_defaults(C.byref(p))
    return p


# ---- 1. header and ctypes ------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_structs(tmp_path):
    structs = {"VimgMomentsFrames": abi.MomentsFrames, "VimgMomentsParams": abi.MomentsParams}
    got = c_layout(tmp_path, ["vimg_moments.h"], structs, 'printf("per_pixel %u\\n", VIMG_MOMENTS_HISTORY_PER_PIXEL);')
    assert got.pop("per_pixel") == "64" == str(abi.MOMENTS_HISTORY_PER_PIXEL)
    assert got == ctypes_layout(structs)
    assert C.sizeof(abi.MomentsFrames) == 56 and C.sizeof(abi.MomentsParams) == 28
    assert abi.MomentsFrames().struct_size == 56 and abi.MomentsParams().struct_size == 28
    # the shared eight fields, where frame_lib.h's check_head and hip.FrameCall expect them, then the variance frame
    shared = [(f, getattr(abi.MomentsFrames, f).offset) for f, _ in abi.TemporalFrames._fields_]
    assert shared == [(f, getattr(abi.TemporalFrames, f).offset) for f, _ in abi.TemporalFrames._fields_]
    assert [o for _, o in shared] == [0, 4, 8, 12, 16, 24, 32, 40] and abi.MomentsFrames.variance.offset == 48
    # the first four floats are VimgTemporalParams's, then min_history
    assert [(f, getattr(abi.MomentsParams, f).offset) for f, _ in abi.TemporalParams._fields_] == \
        [(f, getattr(abi.TemporalParams, f).offset) for f, _ in abi.TemporalParams._fields_]
    assert abi.MomentsParams._fields_[-1][0] == "min_history" and abi.MomentsParams.min_history.offset == 24
    # the ABIs this library leaves closed
    assert C.sizeof(abi.RenderParams) == 20 and C.sizeof(abi.TemporalFrames) == 48 and abi.TEMPORAL_HISTORY_PER_PIXEL == 48


def test_a_history_is_64_bytes_per_pixel_and_the_defaults_are_the_temporal_ones_and_min_history_4():
    lib = abi.moments_lib()
    for w, h in ((1, 1), (3, 5), (1800, 800), (32768, 32768), (0, 7)):
        assert lib.vimg_moments_history_bytes(w, h) == 64 * w * h
    p, t = _defaults(), abi.TemporalParams()
    abi.temporal_lib().vimg_temporal_defaults(C.byref(t))
    assert p.struct_size == C.sizeof(abi.MomentsParams) == 28 and p.reserved == 0
    for name in ("max_history", "current_weight", "sigma_normal", "sigma_plane"):
        assert getattr(p, name) == getattr(t, name), name
    assert p.min_history == 4
    # ... and the call takes them.  Its pointers are made up, so it is only made where no device could follow them:
    # there it passes every argument check and fails at the launch
    import torch
    if not torch.cuda.is_available():
        rc, msg = _call(**_good_call())
        assert rc == -2 and msg.startswith("moments: launch failed"), (rc, msg)          # VIMG_E_DEVICE, no silent success


def test_the_library_exports_the_declared_names_and_its_kernel_and_leaves_the_other_libraries_alone():
    """Five exports: the four functions of the header - nothing else vimg_* - and the kernel moments_accumulate_kernel."""
    assert sorted(abi.MOMENTS_SYMBOLS) == EXPORTS
    abi.moments_lib()                    # loads on a machine without a GPU
    lib = os.path.join(ROOT, "v-img_amd", "lib", "libvimg_moments.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    have = sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("vimg_"))
    assert have == EXPORTS
    kernels = [l.split()[-1] for l in nm.splitlines() if "_kernel" in l and "__device_stub__" not in l]
    assert len(kernels) == 1 and "25moments_accumulate_kernelE" in kernels[0], kernels          # one kernel, one launch
    # the shared host skeleton (frames/frame_lib.h) is internal: no error slot and no helper of it is a dynamic symbol
    assert not [l for l in nm.splitlines() if any(w in l for w in ("g_error", "vimg_frames", "4fail", "last_errorEv", "check_"))]
    header = open(os.path.join(ROOT, "include", "vimg_moments.h")).read()
    for name in abi.MOMENTS_SYMBOLS:
        assert name + "(" in header
    for other in (abi.HIP_SYMBOLS, abi.HIP_TEST_SYMBOLS, abi.FILTER_SYMBOLS, abi.TEMPORAL_SYMBOLS, abi.VARFILTER_SYMBOLS):
        assert not set(abi.MOMENTS_SYMBOLS) & set(other)
    assert "moments" not in open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read()
    # it links the HIP runtime and none of the project's libraries
    needed = subprocess.run(["readelf", "-d", lib], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libvimg" not in needed.replace("libvimg_moments", "")


def test_the_module_and_the_source_directory_of_the_same_name_do_not_collide():
    import vimg_amd.moments as mom
    assert mom.__file__.endswith("moments.py") and callable(mom.accumulate) and callable(mom.params)
    assert not [f for f in os.listdir(os.path.join(abi.PKG_DIR, "moments")) if f.endswith(".py")]


# ---- 2. argument errors, found before anything is enqueued -------------------------------------------------------
W, H = 8, 4
HIST, FRAME, PLANE = 64 * W * H, 12 * W * H, 4 * W * H


def _good_call():
    """Arguments vimg_moments_accumulate accepts up to the launch (the device pointers are never read on the host)."""
    frames = abi.MomentsFrames(width=W, height=H, color=0x1000, normal=0x2000, position=0x3000, depth=0x4000, variance=0x5000)
    return dict(frames=frames, prev=0x10000, matrix=T.IDENTITY.tolist(), params=_defaults(), next=0x20000, out=0x6000,
                out_variance=0x7000)


def _call(frames, prev, matrix, params, next, out, out_variance):
    lib = abi.moments_lib()
    m = None if matrix is None else (abi.f32 * 12)(*matrix)
    rc = lib.vimg_moments_accumulate(None if frames is None else C.byref(frames), C.c_void_p(prev), m,
                                     None if params is None else C.byref(params), C.c_void_p(next), C.c_void_p(out),
                                     C.c_void_p(out_variance), None)
    return rc, lib.vimg_moments_last_error().decode()


def _edit(**kw):
    a = _good_call()
    for k, v in kw.items():
        if k.startswith("m") and k[1:].isdigit():
            a["matrix"][int(k[1:])] = v
        elif k in a:
            a[k] = v
        elif k in dict(abi.MomentsFrames._fields_):
            setattr(a["frames"], k, v)
        else:
            setattr(a["params"], k, v)
    return a


NAN, INF = float("nan"), float("inf")
ERRORS = [
    # vimg_temporal_accumulate's, under the prefix "moments:" and with the 64-byte history
    (dict(frames=None), "null frames"), (dict(params=None), "null params"), (dict(next=None), "null next history"),
    (dict(color=None), "null color frame"), (dict(normal=None), "null normal frame"),
    (dict(position=None), "null position frame"), (dict(depth=None), "null depth frame"),
    (dict(struct_size=55), "frames.struct_size 55 is below the struct's 56"),
    (dict(width=0), "width and height must be 1..32768, not 0 x 4"), (dict(height=0), "width and height must be 1..32768, not 8 x 0"),
    (dict(width=32769), "width and height must be 1..32768, not 32769 x 4"),
    (dict(height=32769), "width and height must be 1..32768, not 8 x 32769"),
    (dict(max_history=0.5), "max_history must be >= 1 and finite, not 0.5"), (dict(max_history=NAN), "max_history must be >= 1 and finite, not nan"),
    (dict(max_history=INF), "max_history must be >= 1 and finite, not inf"), (dict(max_history=-2.0), "max_history must be >= 1 and finite, not -2"),
    (dict(current_weight=0.0), "current_weight must be >= 1 and finite, not 0"),
    (dict(current_weight=NAN), "current_weight must be >= 1 and finite, not nan"),
    (dict(current_weight=INF), "current_weight must be >= 1 and finite, not inf"),
    (dict(sigma_normal=0.0), "sigma_normal must be > 0 and finite, not 0"), (dict(sigma_normal=-1.0), "sigma_normal must be > 0 and finite, not -1"),
    (dict(sigma_normal=NAN), "sigma_normal must be > 0 and finite, not nan"), (dict(sigma_normal=INF), "sigma_normal must be > 0 and finite, not inf"),
    (dict(sigma_plane=0.0), "sigma_plane must be > 0 and finite, not 0"), (dict(sigma_plane=-0.5), "sigma_plane must be > 0 and finite, not -0.5"),
    (dict(sigma_plane=NAN), "sigma_plane must be > 0 and finite, not nan"), (dict(sigma_plane=INF), "sigma_plane must be > 0 and finite, not inf"),
    (dict(next=0x20008), "the next history must be 16-byte aligned"),
    (dict(prev=0x10004), "the previous history must be 16-byte aligned"),
    (dict(matrix=None), "a previous history needs its world-to-pixel matrix"),
    (dict(m0=NAN), "world-to-pixel entry 0 is not finite (nan)"), (dict(m7=INF), "world-to-pixel entry 7 is not finite (inf)"),
    (dict(m11=-INF), "world-to-pixel entry 11 is not finite (-inf)"),
    (dict(prev=None, m5=NAN), "world-to-pixel entry 5 is not finite (nan)"),
    (dict(next=0x10000 + HIST - 16), "the next history overlaps the previous one"),
    (dict(next=0x10000 - HIST + 16), "the next history overlaps the previous one"),
    (dict(next=0x1000), "the next history overlaps the color frame"),
    (dict(next=0x4000 - HIST + 16, out=None, out_variance=None, color=0x100000, normal=0x200000, position=0x300000, variance=None),
     "the next history overlaps the depth frame"),
    (dict(out=0x10000 + HIST - 4), "the output overlaps the previous history"),
    (dict(out=0x20000 - 8), "the output overlaps the next history"),
    (dict(out=0x1004), "the output overlaps the color frame without being it"),
    (dict(out=0x2000), "the output overlaps the normal frame"), (dict(out=0x3000 - 4), "the output overlaps the position frame"),
    (dict(out=0x4000 + FRAME - 4), "the output overlaps the depth frame"),
    # this library's own
    (dict(min_history=0.5), "min_history must be >= 1 and finite, not 0.5"), (dict(min_history=-1.0), "min_history must be >= 1 and finite, not -1"),
    (dict(min_history=NAN), "min_history must be >= 1 and finite, not nan"), (dict(min_history=INF), "min_history must be >= 1 and finite, not inf"),
    (dict(min_history=33.0), "min_history 33 is above max_history 32"),
    (dict(max_history=2.0), "min_history 4 is above max_history 2"),
    (dict(next=0x5000 - HIST + 16, out=None, out_variance=None, color=0x100000, normal=0x200000, position=0x300000, depth=0x400000),
     "the next history overlaps the variance frame"),
    (dict(out=0x5000 - FRAME + 4, depth=0x400000), "the output overlaps the variance frame"),
    (dict(out_variance=0x10000 + HIST - 4), "the output variance overlaps the previous history"),
    (dict(out_variance=0x10000 - PLANE + 4), "the output variance overlaps the previous history"),
    (dict(out_variance=0x20000 + 3 * HIST // 4), "the output variance overlaps the next history"),
    (dict(out_variance=0x1000 + FRAME - 4), "the output variance overlaps the color frame"),
    (dict(out_variance=0x2000), "the output variance overlaps the normal frame"),
    (dict(out_variance=0x3000 - 4), "the output variance overlaps the position frame"),
    (dict(out_variance=0x4000 + 8), "the output variance overlaps the depth frame"),
    (dict(out_variance=0x6000 + FRAME - 4), "the output variance overlaps the output"),
    (dict(out_variance=0x1000, out=0x1000), "the output variance overlaps the color frame"),
    (dict(out_variance=0x5004), "the output variance overlaps the variance frame without being it"),
    (dict(out_variance=0x5000 - PLANE + 4), "the output variance overlaps the variance frame without being it"),
]


@pytest.mark.parametrize("edit,sentence", ERRORS, ids=[f"{'-'.join(e)}-{i}" for i, (e, _) in enumerate(ERRORS)])
def test_argument_errors_are_invalid_with_their_whole_sentence_and_need_no_device(edit, sentence):
    rc, msg = _call(**_edit(**edit))
    assert rc == INVALID and msg == "moments: " + sentence, (rc, msg)


def test_the_shared_sentences_are_the_temporal_librarys_under_another_prefix():
    """Each of vimg_temporal_accumulate's recorded errors (tests/test_temporal_abi.py), made on both libraries with the
    same edit where the edit means the same in both: the sentence differs in the prefix alone."""
    import test_temporal_abi as TA

    def means_the_same(edit):      # not the edits whose numbers rest on the 48-byte history, the 48-byte struct or the output
        return "struct_size" not in edit and "out" not in edit and ("next" not in edit or edit["next"] in (None, 0x20008, 0x1000))
    n = 0
    for edit, _ in TA.ERRORS:
        if not means_the_same(edit):
            continue
        rc_t, msg_t = TA._call(**TA._edit(**edit))
        rc_m, msg_m = _call(**_edit(**edit))
        assert rc_t == rc_m == INVALID and msg_t.startswith("temporal: ") and msg_m == "moments: " + msg_t[len("temporal: "):], (edit, msg_t, msg_m)
        n += 1
    assert n >= 30


def test_params_struct_size_the_error_slot_and_what_is_not_an_error():
    a = _good_call()
    a["params"].struct_size = 27
    rc, msg = _call(**a)
    assert rc == INVALID and msg == "moments: params.struct_size 27 is below the struct's 28"
    # an error slot of its own: a failure of the temporal library leaves this library's sentence alone, and the reverse
    import test_temporal_abi as TA
    assert TA._call(**TA._edit(max_history=0.25))[0] == INVALID
    assert abi.moments_lib().vimg_moments_last_error().decode() == msg
    assert _call(**_edit(min_history=0.25)) == (INVALID, "moments: min_history must be >= 1 and finite, not 0.25")
    assert abi.temporal_lib().vimg_temporal_last_error().decode() == "temporal: max_history must be >= 1 and finite, not 0.25"
    # no history and no matrix, no outputs, no variance frame, outputs that are the frames they may be, history right
    # behind history, min_history at max_history: all pass every argument check (and only then need a device)
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(prev=None, matrix=None), dict(out=None), dict(out_variance=None), dict(variance=None), dict(out=0x1000),
                   dict(out_variance=0x5000), dict(out_variance=0x5004, variance=None),
                   dict(next=0x10000 + HIST), dict(max_history=1.0, min_history=1.0, current_weight=7.0), dict(min_history=32.0)):
            rc, msg = _call(**_edit(**ok))
            assert rc == -2 and msg.startswith("moments: launch failed"), (ok, rc, msg)          # VIMG_E_DEVICE, no silent success


# ---- 3. the restatement, pinned on its own -----------------------------------------------------------------------
def extended_case(w, h, seed=0):
    """test_temporal.random_case with a plane M in the history (positive first moments, second moments above and, for
    some pixels, below their square; a V the contract never reads) and a variance frame that holds known values, 0, NaN,
    negative values and +inf."""
    f, prev3 = random_case(w, h, seed)
    rng = np.random.default_rng(31 * h + w + seed)
    prev = np.zeros((4, h, w, 4), F)
    prev[:3] = prev3
    m1 = rng.gamma(4.0, 0.25, (h, w))
    prev[3, ..., 0] = m1
    prev[3, ..., 1] = m1 * m1 * rng.uniform(0.9, 1.6, (h, w))
    prev[3, ..., 2] = rng.gamma(2.0, 0.01, (h, w))
    var = rng.gamma(2.0, 0.02, (h, w)).astype(F)
    flat = var.reshape(-1)
    if flat.size >= 15:
        for i, bad in enumerate((np.nan, -0.5, np.inf, 0.0, -np.inf)):
            flat[(i * 7 + 3) % 15::11] = bad
    return f, prev, var


def test_planes_0_to_2_and_rgb_are_the_temporal_restatement_bit_for_bit():
    w, h = 67, 5
    f, prev, var = extended_case(w, h)
    kw = dict(EXPLICIT, min_history=3.0)
    for name, m in matrices(w, h).items():
        want = T.accumulate(f["color"], f["normal"], f["position"], f["depth"], prev[:3], m, **EXPLICIT)
        for v in (var, None):
            got = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], v, prev, m, **kw)
            assert got.shape == (4, h, w, 4) and got.dtype == F
            assert np.array_equal(_bits(got[:3]), _bits(want)), name
            assert (got[3, ..., 3] == 0).all()
        # ... and the three kinds of pixel are all there, with V known for some of the blended ones and not for others
        got = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], var, prev, m, **kw)
        L, V = got[0, ..., 3], got[3, ..., 2]
        assert (L == 0).any() and (L == 1).any() and (L > 1).any()
        assert (V[L == 0] == 0).all()
        assert np.isnan(V[(L > 1) & (L < 3)]).all() and R.known(V[L >= 3]).any()
    want = T.accumulate(f["color"], f["normal"], f["position"], f["depth"], None, None, **EXPLICIT)
    got = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], var, None, None, **kw)
    assert np.array_equal(_bits(got[:3]), _bits(want))


def test_without_history_V_is_the_known_variance_itself_and_nan_without_one():
    w, h = 67, 5
    f, prev, var = extended_case(w, h)
    empty = prev.copy()
    empty[0, ..., 3] = 0                          # a history nobody can tap is no history either
    for p, m in ((None, None), (empty, T.IDENTITY)):
        got = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], var, p, m, **PARAMS)
        L, V = got[0, ..., 3], got[3, ..., 2]
        assert set(np.unique(L)) == {0.0, 1.0}
        vk = R.known(var)
        assert vk.any() and (~vk).any() and (var[~vk] < 0).any() and np.isinf(var[~vk]).any()
        live = L == 1
        assert np.array_equal(_bits(V[live & vk]), _bits(var[live & vk]))          # V == v exactly
        assert np.array_equal(_bits(V[live & ~vk]), np.full((live & ~vk).sum(), 0x7FC00000, np.uint32))
        assert (V[~live] == 0).all()
        # the first moment is the luminance, the second its square and the correction, which is 0 at current_weight 1
        Lc = R.lum(f["color"])
        assert np.array_equal(_bits(got[3, ..., 0]), _bits(Lc))
        ok = ~np.isnan(Lc)
        assert np.array_equal(_bits(got[3, ..., 1][ok & ~vk]), _bits((Lc * Lc)[ok & ~vk]))
        none = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], None, p, m, **PARAMS)
        assert np.isnan(none[3, ..., 2][live]).all() and (none[3, ..., 2][~live] == 0).all()
        assert np.array_equal(_bits(none[:3]), _bits(got[:3]))


def _static(h, w, frames, rng, mean=2.0, sigma=0.7, **kw):
    """Static grey pixels under the identity with iid Gaussian luminance: the histories after each frame."""
    f = T.flat_frames(h, w, 0)
    hist, out = None, []
    for _ in range(frames):
        c = (rng.normal(mean, sigma, (h, w, 1)) * np.ones(3)).astype(F)
        hist = R.accumulate(c, f["normal"], f["position"], f["depth"], None, hist, T.IDENTITY, **dict(PARAMS, **kw))
        out.append(hist)
    return out


def test_a_history_shorter_than_min_history_has_no_variance():
    hists = _static(4, 6, 7, np.random.default_rng(5), min_history=5)
    for i, hist in enumerate(hists, start=1):
        assert (hist[0, ..., 3] == i).all()
        V = hist[3, ..., 2]
        if i < 5:
            assert np.array_equal(_bits(V), np.full(V.shape, 0x7FC00000, np.uint32)), i
        else:
            assert R.known(V).all() and (V > 0).all(), i
    # the moments are the plain means of luminance and of its square while the length is below the cap
    assert np.isfinite(hists[-1][3, ..., :2]).all() and (hists[-1][3, ..., 1] >= hists[-1][3, ..., 0] ** 2).all()


def test_at_current_weight_1_the_correction_adds_exactly_zero_and_at_k_it_adds_v_times_k_minus_1():
    w, h = 67, 5
    f, prev, var = extended_case(w, h)
    var = np.where(R.known(var), var, F(0.02)).astype(F)         # every value known: the correction is taken everywhere
    m = matrices(w, h)["half_pixel"]
    a = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], var, None, None, **PARAMS)
    b = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], None, None, None, **PARAMS)
    assert np.array_equal(_bits(a[3, ..., :2]), _bits(b[3, ..., :2]))          # x2 + v 0 == x2, bit for bit
    a = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], var, prev, m, **PARAMS)
    b = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], None, prev, m, **PARAMS)
    assert np.array_equal(_bits(a[3, ..., :2]), _bits(b[3, ..., :2]))
    Lc = R.lum(f["color"])
    k3 = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], var, None, None, **dict(PARAMS, current_weight=3))
    ok = ~np.isnan(Lc)
    assert np.array_equal(_bits(k3[3, ..., 1][ok]), _bits((Lc * Lc + var * F(2))[ok]))
    assert (k3[3, ..., 1][ok & (var > 0)] > (Lc * Lc)[ok & (var > 0)]).all() and (var == 0).any()


def test_a_hand_computed_blend_of_the_moments():
    """A history of length 3 with moments (0.5, 0.375) and a frame of luminance 1 with known variance 0.0625: N = 4,
    a = 1 / 4, u u = 9 / 16, a a = 1 / 16, sh = 1 / 8."""
    h, w = 3, 4
    f = T.flat_frames(h, w, 0)
    prev = np.zeros((4, h, w, 4), F)
    prev[:3] = T.accumulate(np.full((h, w, 3), 0.5, F), f["normal"], f["position"], f["depth"], None, None, **EXPLICIT)
    prev[0, ..., 3] = 3
    prev[3, ..., 0], prev[3, ..., 1] = 0.5, 0.375
    grey = np.full((h, w, 3), 1, F)
    Lc = R.lum(grey)[0, 0]
    var = np.full((h, w), 0.0625, F)
    for v, vc in ((var, 0.0625), (None, None)):
        out = R.accumulate(grey, f["normal"], f["position"], f["depth"], v, prev, T.IDENTITY, **PARAMS)
        m1 = F(0.5) + (Lc - F(0.5)) * F(0.25)
        m2 = F(0.375) + (Lc * Lc - F(0.375)) * F(0.25)
        sc = m2 - m1 * m1
        Vh = F(0.125) / F(3)                        # sh = 0.375 - 0.25, over len = 3
        want = F(0.5625) * Vh + F(0.0625) * (F(vc) if vc is not None else sc / F(1))
        assert (out[0, ..., 3] == 4).all()
        assert (out[3, ..., 0] == m1).all() and (out[3, ..., 1] == m2).all() and (out[3, ..., 2] == want).all()
    short = R.accumulate(grey, f["normal"], f["position"], f["depth"], var, prev, T.IDENTITY, **dict(PARAMS, min_history=4.5))
    assert np.isnan(short[3, ..., 2]).all() and np.array_equal(_bits(short[3, ..., :2]), _bits(out[3, ..., :2]))


def test_the_variance_is_the_spread_of_the_accumulated_luminance():
    """20 000 static pixels under the identity, iid Gaussian luminance (mean 2, sigma 0.7), grey, current_weight 1, no
    variance frame: mean(V) / var(Y(A)) over the pixels lies in [0.6, 1.7] at frames 4, 5, 8, 16 and 32 for max_history
    32, and at frame 32 for max_history 8.  A float64 simulation of the recursion gives 0.69 (N = 4) .. 0.97 (N = 32)
    and, at the cap, 1.56; the standard error of the mean ratio is about 0.005."""
    h, w = 100, 200
    for cap, at in ((32, (4, 5, 8, 16, 32)), (8, (32,))):
        hists = _static(h, w, 32, np.random.default_rng(1000 + cap), max_history=cap)
        for n in at:
            hist = hists[n - 1]
            assert (hist[0, ..., 3] == min(n, cap)).all()
            V = hist[3, ..., 2].astype(np.float64)
            assert np.isfinite(V).all()
            ratio = V.mean() / R.lum(hist[0, ..., :3]).astype(np.float64).var()
            print(f"max_history {cap}, frame {n}: mean(V) / var(Y(A)) = {ratio:.3f}")
            assert 0.6 <= ratio <= 1.7, (cap, n, ratio)
        for n in (1, 2, 3):
            assert np.isnan(hists[n - 1][3, ..., 2]).all()
