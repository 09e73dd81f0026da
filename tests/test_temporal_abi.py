"""The temporal library at its boundary, without a GPU: include/vimg_temporal.h against its ctypes mirror, the exports
of libvimg_temporal.so, every argument error of vimg_temporal_accumulate, the numpy restatement of its contract
(tests/temporal_ref.py) pinned on its own, and temporal.world_to_pixel against a float64 restatement of the
reference camera's generate_ray."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import temporal_ref as R
from abi_layout import c_layout, ctypes_layout
from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # VIMG_E_INVALID
F = np.float32
PARAMS = dict(max_history=32, current_weight=1, sigma_normal=0.1, sigma_plane=0.01)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. header and ctypes ------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_structs(tmp_path):
    structs = {"VimgTemporalFrames": abi.TemporalFrames, "VimgTemporalParams": abi.TemporalParams}
    got = c_layout(tmp_path, ["vimg_temporal.h"], structs, 'printf("per_pixel %u\\n", VIMG_TEMPORAL_HISTORY_PER_PIXEL);')
    assert got.pop("per_pixel") == "48" == str(abi.TEMPORAL_HISTORY_PER_PIXEL)
    assert got == ctypes_layout(structs)
    assert C.sizeof(abi.TemporalFrames) == 48 and C.sizeof(abi.TemporalParams) == 24
    assert abi.TemporalFrames().struct_size == 48


def test_a_history_is_48_bytes_per_pixel_and_the_defaults_are_valid():
    lib = abi.temporal_lib()
    for w, h in ((1, 1), (3, 5), (1800, 800), (32768, 32768), (0, 7)):
        assert lib.vimg_temporal_history_bytes(w, h) == 48 * w * h
    p = abi.TemporalParams()
    lib.vimg_temporal_defaults(C.byref(p))
    assert p.struct_size == C.sizeof(abi.TemporalParams) == 24 and p.reserved == 0
    assert 1 <= p.max_history < np.inf and p.current_weight == 1
    assert 0 < p.sigma_normal < np.inf and 0 < p.sigma_plane < np.inf
    # ... and the call takes them.  Its pointers are made up, so it is only made where no device could follow them:
    # there it passes every argument check and fails at the launch
    import torch
    if not torch.cuda.is_available():
        a = _good_call()
        a["params"] = p
        rc, msg = _call(**a)
        assert rc == -2 and "launch failed" in msg, (rc, msg)


def test_the_library_exports_the_four_declared_names_and_leaves_the_other_two_alone():
    assert sorted(abi.TEMPORAL_SYMBOLS) == ["vimg_temporal_accumulate", "vimg_temporal_defaults", "vimg_temporal_history_bytes",
                                            "vimg_temporal_last_error"]
    abi.temporal_lib()                    # loads on a machine without a GPU
    lib = os.path.join(ROOT, "v-img_amd", "lib", "libvimg_temporal.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    have = sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("vimg_"))
    assert have == sorted(abi.TEMPORAL_SYMBOLS)
    assert any("temporal_accumulate_kernel" in l for l in nm.splitlines())       # ... and its kernel is in it
    # the shared host skeleton (frames/frame_lib.h) is internal: no error slot and no helper of it is a dynamic symbol,
    # so the dynamic linker cannot merge this library's error slot with the other frame library's
    assert not [l for l in nm.splitlines() if any(w in l for w in ("g_error", "vimg_frames", "4fail", "last_errorEv", "check_"))]
    header = open(os.path.join(ROOT, "include", "vimg_temporal.h")).read()
    for name in abi.TEMPORAL_SYMBOLS:
        assert name + "(" in header
    assert not set(abi.TEMPORAL_SYMBOLS) & (set(abi.HIP_SYMBOLS) | set(abi.FILTER_SYMBOLS))
    assert "temporal" not in open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read()
    # it links the HIP runtime and nothing of the other two libraries
    needed = subprocess.run(["readelf", "-d", lib], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libvimg" not in needed.replace("libvimg_temporal", "")


def test_the_module_and_the_source_directory_of_the_same_name_do_not_collide():
    import vimg_amd.temporal as tmp
    assert tmp.__file__.endswith("temporal.py") and callable(tmp.accumulate)
    assert not [f for f in os.listdir(os.path.join(abi.PKG_DIR, "temporal")) if f.endswith(".py")]


# ---- 2. argument errors, found before anything is enqueued -------------------------------------------------------
def _good_call():
    """Arguments vimg_temporal_accumulate accepts up to the launch (the device pointers are never read on the host)."""
    frames = abi.TemporalFrames(width=8, height=4, color=0x1000, normal=0x2000, position=0x3000, depth=0x4000)
    params = abi.TemporalParams()
    abi.temporal_lib().vimg_temporal_defaults(C.byref(params))
    return dict(frames=frames, prev=0x10000, matrix=R.IDENTITY.tolist(), params=params, next=0x20000, out=0x6000)


def _call(frames, prev, matrix, params, next, out):
    lib = abi.temporal_lib()
    m = None if matrix is None else (abi.f32 * 12)(*matrix)
    rc = lib.vimg_temporal_accumulate(None if frames is None else C.byref(frames), C.c_void_p(prev), m,
                                      None if params is None else C.byref(params), C.c_void_p(next), C.c_void_p(out), None)
    return rc, lib.vimg_temporal_last_error().decode()


def _edit(**kw):
    a = _good_call()
    for k, v in kw.items():
        if k.startswith("m") and k[1:].isdigit():
            a["matrix"][int(k[1:])] = v
        elif k in a:
            a[k] = v
        elif k in dict(abi.TemporalFrames._fields_):
            setattr(a["frames"], k, v)
        else:
            setattr(a["params"], k, v)
    return a


NAN, INF = float("nan"), float("inf")
ERRORS = [
    (dict(frames=None), "null frames"), (dict(params=None), "null params"), (dict(next=None), "null next history"),
    (dict(color=None), "null color frame"), (dict(normal=None), "null normal frame"),
    (dict(position=None), "null position frame"), (dict(depth=None), "null depth frame"),
    (dict(struct_size=47), "frames.struct_size 47 is below"),
    (dict(width=0), "width and height must be 1..32768"), (dict(height=0), "width and height must be 1..32768"),
    (dict(width=32769), "width and height must be 1..32768"), (dict(height=32769), "width and height must be 1..32768"),
    (dict(max_history=0.5), "max_history must be >= 1 and finite"), (dict(max_history=NAN), "max_history must be >= 1 and finite"),
    (dict(max_history=INF), "max_history must be >= 1 and finite"), (dict(max_history=-2.0), "max_history must be >= 1 and finite"),
    (dict(current_weight=0.0), "current_weight must be >= 1 and finite"), (dict(current_weight=NAN), "current_weight must be >= 1 and finite"),
    (dict(current_weight=INF), "current_weight must be >= 1 and finite"),
    (dict(sigma_normal=0.0), "sigma_normal must be > 0 and finite"), (dict(sigma_normal=-1.0), "sigma_normal must be > 0 and finite"),
    (dict(sigma_normal=NAN), "sigma_normal must be > 0 and finite"), (dict(sigma_normal=INF), "sigma_normal must be > 0 and finite"),
    (dict(sigma_plane=0.0), "sigma_plane must be > 0 and finite"), (dict(sigma_plane=-0.5), "sigma_plane must be > 0 and finite"),
    (dict(sigma_plane=NAN), "sigma_plane must be > 0 and finite"), (dict(sigma_plane=INF), "sigma_plane must be > 0 and finite"),
    (dict(next=0x20008), "the next history must be 16-byte aligned"),
    (dict(prev=0x10004), "the previous history must be 16-byte aligned"),
    (dict(matrix=None), "a previous history needs its world-to-pixel matrix"),
    (dict(m0=NAN), "world-to-pixel entry 0 is not finite"), (dict(m7=INF), "world-to-pixel entry 7 is not finite"),
    (dict(m11=-INF), "world-to-pixel entry 11 is not finite"),
    (dict(prev=None, m5=NAN), "world-to-pixel entry 5 is not finite"),
    (dict(next=0x10000 + 48 * 8 * 4 - 16), "the next history overlaps the previous one"),
    (dict(next=0x1000), "the next history overlaps the color frame"),
    (dict(next=0x4000 - 48 * 8 * 4 + 16), "the next history overlaps the depth frame"),
    (dict(out=0x10000 + 48 * 8 * 4 - 4), "the output overlaps the previous history"),
    (dict(out=0x20000 - 8), "the output overlaps the next history"),
    (dict(out=0x1004), "the output overlaps the color frame without being it"),
    (dict(out=0x2000), "the output overlaps the normal frame"), (dict(out=0x3000 - 4), "the output overlaps the position frame"),
    (dict(out=0x4000 + 12 * 8 * 4 - 4), "the output overlaps the depth frame"),
]


@pytest.mark.parametrize("edit,sentence", ERRORS, ids=[f"{'-'.join(e)}-{i}" for i, (e, _) in enumerate(ERRORS)])
def test_argument_errors_are_invalid_with_their_sentence_and_need_no_device(edit, sentence):
    rc, msg = _call(**_edit(**edit))
    assert rc == INVALID and sentence in msg, (rc, msg)


def test_params_struct_size_the_last_message_and_what_is_not_an_error():
    a = _good_call()
    a["params"].struct_size = 23
    rc, msg = _call(**a)
    assert rc == INVALID and "params.struct_size 23 is below" in msg
    rc, msg2 = _call(**_edit(max_history=0.25))
    assert rc == INVALID and msg2 != msg and "0.25" in msg2
    # no history and no matrix, no output, an output that is the colour frame, history right behind history: all pass
    # every argument check (and only then need a device)
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(prev=None, matrix=None), dict(out=None), dict(out=0x1000), dict(next=0x10000 + 48 * 8 * 4),
                   dict(max_history=1.0, current_weight=7.0)):
            rc, msg = _call(**_edit(**ok))
            assert rc == -2 and "launch failed" in msg, (ok, rc, msg)          # VIMG_E_DEVICE, no silent success


# ---- 3. the restatement, pinned on its own -----------------------------------------------------------------------
def test_a_constant_colour_under_the_identity_keeps_its_bits_and_the_length_counts_up_to_the_cap():
    h, w = 5, 7
    colour = np.random.default_rng(2).gamma(2.0, 0.5, (h, w, 3)).astype(F)       # arbitrary float32, constant in time
    f = R.flat_frames(h, w, colour)
    hist = None
    for i in range(40):
        hist = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], hist, R.IDENTITY, **dict(PARAMS, max_history=8))
        assert np.array_equal(_bits(hist[0, ..., :3]), _bits(colour))
        assert (hist[0, ..., 3] == min(i + 1, 8)).all()
        assert np.array_equal(hist[1, ..., :3], f["normal"]) and (hist[1, ..., 3] == 8).all()
        assert np.array_equal(hist[2, ..., :3], f["position"]) and (hist[2, ..., 3] == 0).all()


def test_k_noisy_frames_under_the_identity_are_their_arithmetic_mean():
    h, w, k = 4, 6, 24
    rng = np.random.default_rng(3)
    frames = rng.gamma(2.0, 0.5, (k, h, w, 3)).astype(F)
    f = R.flat_frames(h, w, 0)
    hist = None
    for c in frames:
        hist = R.accumulate(c, f["normal"], f["position"], f["depth"], hist, R.IDENTITY, **PARAMS)
    assert (hist[0, ..., 3] == k).all()
    assert np.allclose(hist[0, ..., :3], frames.astype(np.float64).mean(axis=0), rtol=1e-6, atol=0)
    # beyond the cap the blend factor stays at 1 / max_history: an exponential average, no longer the mean
    for c in frames:
        hist = R.accumulate(c, f["normal"], f["position"], f["depth"], hist, R.IDENTITY, **dict(PARAMS, max_history=8))
    assert (hist[0, ..., 3] == 8).all()
    want = hist[0, ..., :3].astype(np.float64)
    nxt = R.accumulate(frames[0], f["normal"], f["position"], f["depth"], hist, R.IDENTITY, **dict(PARAMS, max_history=8))
    assert np.allclose(nxt[0, ..., :3], want + (frames[0] - want) / 8, rtol=1e-6)


def test_a_shift_by_one_column_blends_the_left_neighbour_and_the_entering_column_starts_over():
    h, w = 4, 9
    rng = np.random.default_rng(4)
    f = R.flat_frames(h, w, 0)
    H = rng.uniform(0.1, 1, (h, w, 3)).astype(F)
    Cc = rng.uniform(0.1, 1, (h, w, 3)).astype(F)
    prev = R.accumulate(H, f["normal"], f["position"], f["depth"], None, None, **PARAMS)
    out = R.accumulate(Cc, f["normal"], f["position"], f["depth"], prev, R.shift_matrix(-1.0), **PARAMS)
    assert (out[0, :, 0, 3] == 1).all() and np.array_equal(_bits(out[0, :, 0, :3]), _bits(Cc[:, 0]))
    assert (out[0, :, 1:, 3] == 2).all()
    Hs = H[:, :-1]
    assert np.array_equal(_bits(out[0, :, 1:, :3]), _bits(Hs + (Cc[:, 1:] - Hs) * F(0.5)))
    # a half-pixel shift in both directions blends four taps of weight 1/4: the mean of the 2 x 2 block
    out = R.accumulate(Cc, f["normal"], f["position"], f["depth"], prev, R.shift_matrix(-0.5, -0.5), **PARAMS)
    q = F(0.25)
    Hm = (((q * H[:-1, :-1] + q * H[:-1, 1:]) + q * H[1:, :-1]) + q * H[1:, 1:]) / F(1)
    assert np.array_equal(_bits(out[0, 1:, 1:, :3]), _bits(Hm + (Cc[1:, 1:] - Hm) * F(0.5)))
    # ... and on the border the taps outside the image drop out: the remaining ones are renormalised
    Hb = ((q * H[0, :-1] + q * H[0, 1:]) / F(0.5))
    assert np.array_equal(_bits(out[0, 0, 1:, :3]), _bits(Hb + (Cc[0, 1:] - Hb) * F(0.5)))
    assert (out[0, ..., 3] == 2).all()


def _run_sequence(seq, **params):
    hist, out = None, []
    for i, f in enumerate(seq):
        hist = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], hist, seq[i - 1]["matrix"] if i else None, **params)
        out.append(hist)
    return out


def test_the_moved_box_disoccludes_wall_that_starts_over_and_misses_are_nobodys_tap():
    seq = R.synthetic_sequence(16, 32, frames=4)
    hists = _run_sequence(seq, **PARAMS)
    h, w = 16, 32
    for i in (1, 2, 3):
        f, g, L = seq[i], seq[i - 1], hists[i][0, ..., 3]
        # where the wall of pixel x was a frame ago: column x + 1; the box: column x + 2 (both exact, tx = 0)
        src = np.arange(w)[None, :] + np.where(f["box"], 2, 1)
        ok = src < w
        same = np.zeros((h, w), bool)
        rows = np.arange(h)[:, None].repeat(w, 1)
        same[ok] = (g["box"][rows[ok], src[ok]] == f["box"][ok]) & g["hit"][rows[ok], src[ok]]
        same &= f["hit"]
        fresh = f["hit"] & ~same
        assert fresh.sum() == 6 + h - 2          # the column of wall that was behind the box, and the entering column
        assert (L[fresh] == 1).all() and np.array_equal(_bits(hists[i][0][fresh][:, :3]), _bits(f["color"][fresh]))
        prevL = hists[i - 1][0, ..., 3]
        assert np.array_equal(L[same], prevL[rows[same], src[same]] + 1)
        if i == 1:
            assert (L[same] == 2).all()
        # misses: length 0, their own bits, and below them nothing changed because of them
        miss = ~f["hit"]
        assert miss.sum() == 2 * w and (L[miss] == 0).all()
        assert np.array_equal(_bits(hists[i][0][miss][:, :3]), _bits(f["color"][miss]))
    # a history whose wall rows are all misses (length 0) is nobody's tap: every surface pixel starts over
    empty = hists[0].copy()
    empty[0, ..., 3] = 0
    f = seq[1]
    out = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], empty, seq[0]["matrix"], **PARAMS)
    assert (out[0, ..., 3][f["hit"]] == 1).all() and np.array_equal(_bits(out[0, ..., :3]), _bits(f["color"]))
    # the accumulated sequence is nearer the clean picture than its last noisy frame
    mse = lambda a: float(((a.astype(np.float64) - seq[3]["clean"]) ** 2).mean())
    assert mse(hists[3][0, ..., :3]) < 0.5 * mse(seq[3]["color"])


def test_a_nan_history_colour_reaches_the_four_pixels_that_tap_it_and_a_nan_position_starts_over():
    h, w = 8, 10
    rng = np.random.default_rng(6)
    f = R.flat_frames(h, w, 0)
    H = rng.uniform(0.1, 1, (h, w, 3)).astype(F)
    Cc = rng.uniform(0.1, 1, (h, w, 3)).astype(F)
    prev = R.accumulate(H, f["normal"], f["position"], f["depth"], None, None, **PARAMS)
    prev[0, 3, 4, 1] = np.nan
    m = R.shift_matrix(-0.5, -0.5)
    out = R.accumulate(Cc, f["normal"], f["position"], f["depth"], prev, m, **PARAMS)
    bad = np.isnan(out[0]).any(axis=-1)
    assert bad.sum() == 4 and bad[3:5, 4:6].all()
    assert np.isnan(out[0, 3:5, 4:6, 1]).all() and not np.isnan(out[0][..., (0, 2, 3)]).any()
    # under the identity only the pixel itself taps it (the other three weights are 0, and 0 * NaN is not added)
    out = R.accumulate(Cc, f["normal"], f["position"], f["depth"], prev, R.IDENTITY, **PARAMS)
    assert np.isnan(out[0]).sum() == 1 and np.isnan(out[0, 3, 4, 1])
    # a NaN in the current position, normal or depth: no history for that pixel (length 1; 0 for the depth)
    prev[0, 3, 4, 1] = 0.5
    for name, length in (("position", 1), ("normal", 1), ("depth", 0)):
        g = {k: v.copy() for k, v in f.items()}
        g[name][2, 7, 0] = np.nan
        out = R.accumulate(Cc, g["normal"], g["position"], g["depth"], prev, m, **PARAMS)
        assert out[0, 2, 7, 3] == length and np.array_equal(_bits(out[0, 2, 7, :3]), _bits(Cc[2, 7]))
        others = np.ones((h, w), bool)
        others[2, 7] = False
        assert (out[0, ..., 3][others] == 2).all() and not np.isnan(out[0]).any()
    # a NaN guide in the history: the pixels that tap it go on without it
    prev[1, 3, 4, 0] = np.nan
    out = R.accumulate(Cc, f["normal"], f["position"], f["depth"], prev, m, **PARAMS)
    assert not np.isnan(out[0]).any() and (out[0, ..., 3] == 2).all()


def test_current_weight_k_is_the_hand_computed_blend():
    """A history of length 3 and a current frame that is the mean of 2: N = 5, a = 2 / 5.  With max_history 4 the
    length is capped, a = 2 / 4; with current_weight 40 > max_history a would be 40 / 32 and is 1."""
    h, w = 3, 4
    f = R.flat_frames(h, w, 0)
    H, Cc = F(0.7), F(0.2)
    prev = R.accumulate(np.full((h, w, 3), H, F), f["normal"], f["position"], f["depth"], None, None, **PARAMS)
    prev[0, ..., 3] = 3
    col = np.full((h, w, 3), Cc, F)
    for cw, cap, n, a in ((2, 32, 5, F(2) / F(5)), (2, 4, 4, F(0.5)), (40, 32, 32, F(1))):
        out = R.accumulate(col, f["normal"], f["position"], f["depth"], prev, R.IDENTITY,
                           **dict(PARAMS, current_weight=cw, max_history=cap))
        assert (out[0, ..., 3] == n).all()
        assert np.array_equal(_bits(out[0, ..., :3]), _bits(np.full((h, w, 3), H + (Cc - H) * a, F)))


# ---- 4. world_to_pixel ------------------------------------------------------------------------------------------------
def _generate_ray64(cam, x, y):
    """The reference camera's generate_ray for a pinhole, in float64: origin and direction in world space."""
    theta = math.radians(cam.vfov_deg)
    ph = 2.0 * math.tan(theta / 2.0)
    pw = (cam.res_x / cam.res_y) * ph
    d = np.array([pw * (x / cam.res_x) - pw / 2.0, ph * (y / cam.res_y) - ph / 2.0, -1.0])
    d /= np.linalg.norm(d)
    m = np.array(list(cam.cam_to_world), np.float64).reshape(4, 4).T
    return m[:3, 3], m[:3, :3] @ d


def test_world_to_pixel_projects_a_point_on_a_camera_ray_back_to_its_pixel():
    """Seeded look-at cameras up to 1920 x 1080, vfov 30 .. 100 degrees, eyes within 5 of the origin on each axis, with
    and without a lens; points 5 .. 50 along the ray of a random sample position.  The bound of 1e-3 px is what the
    float32 matrix allows there: each entry is off by at most 2^-25 of itself, so hx (or hy) by 2^-25 times the sum
    of its four terms - at most (H / ph) (|P - eye| + 2 |eye|) with H / ph <= 1080 / (2 tan 15 deg) = 2016 pixels per
    unit - and hw is at least half the distance at these fields of view: 3e-8 * 2016 * (2 + 4 * 8.7 / 5) = 5.4e-4 px."""
    from vimg_amd import temporal
    from vimg_amd.host import camera_lookat
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(20):
        res = (int(rng.integers(16, 1921)), int(rng.integers(16, 1081)))
        eye = rng.uniform(-5, 5, 3)
        at = eye + rng.normal(size=3) * 5
        up = np.array([0.0, 1.0, 0.0]) + 0.2 * rng.normal(size=3)
        cam = camera_lookat(eye, at, up, float(rng.uniform(30, 100)), res, float(rng.choice([0.0, 0.1])), 3.0)
        m = temporal.world_to_pixel(cam)
        assert m.dtype == F and m.shape == (12,)
        m = m.astype(np.float64).reshape(3, 4)
        for _ in range(50):
            x, y = rng.uniform(0, res[0]), rng.uniform(0, res[1])
            o, d = _generate_ray64(cam, x, y)
            p = o + d * rng.uniform(5, 50)
            hx, hy, hw = m @ np.append(p, 1.0)
            assert hw > 0
            worst = max(worst, abs(hx / hw - x), abs(hy / hw - (res[1] - y)))
            # ... and the mirrored point lies behind the camera
            assert (m @ np.append(o - d, 1.0))[2] < 0
    print(f"world_to_pixel: worst reprojection error {worst:.2e} px")
    assert worst < 1e-3
