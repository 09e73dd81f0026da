"""The reconstruction library at its boundary, without a GPU: include/vimg_infill.h against its ctypes mirror, the
exports of libvimg_infill.so, every argument error of its call, the lattices of vimg_amd.infill, and the numpy
restatement of the contract (tests/infill_ref.py) pinned on its own against cases worked out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import infill_ref as R
from abi_layout import c_layout, ctypes_layout
from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # VIMG_E_INVALID
F = np.float32
EXPORTS = ["vimg_infill_defaults", "vimg_infill_last_error", "vimg_infill_reconstruct", "vimg_infill_workspace"]


def _defaults():
    p = abi.InfillParams()
    abi.infill_lib().vimg_infill_defaults(C.byref(p))
    return p


def default_kw():
    p = _defaults()
    return {k: getattr(p, k) for k, _ in abi.InfillParams._fields_ if k != "struct_size"}


# ---- 1. header and ctypes ------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_structs(tmp_path):
    structs = {"VimgInfillFrames": abi.InfillFrames, "VimgInfillParams": abi.InfillParams}
    got = c_layout(tmp_path, ["vimg_infill.h"], structs,
                   'printf("codes %d %d\\n", VIMG_OK, VIMG_E_INVALID);'
                   'printf("what %u %u %u %u\\n", VIMG_INFILL_SAMPLED, VIMG_INFILL_GUIDED, VIMG_INFILL_UNGUIDED, VIMG_INFILL_HOLE);'
                   'printf("limits %u %u\\n", VIMG_INFILL_MAX_RADIUS, VIMG_INFILL_WORKSPACE_PER_PIXEL);')
    assert got.pop("codes 0") == str(INVALID)
    assert got.pop("what 0 1 2") == "3" and got.pop("limits 4") == "48"
    assert (abi.INFILL_SAMPLED, abi.INFILL_GUIDED, abi.INFILL_UNGUIDED, abi.INFILL_HOLE) == (0, 1, 2, 3) == (R.SAMPLED, R.GUIDED, R.UNGUIDED, R.HOLE)
    assert abi.INFILL_MAX_RADIUS == 4 and abi.INFILL_WORKSPACE_PER_PIXEL == 48
    assert got == ctypes_layout(structs)
    assert C.sizeof(abi.InfillFrames) == 64 and C.sizeof(abi.InfillParams) == 20
    assert abi.InfillFrames().struct_size == 64 and abi.InfillParams().struct_size == 20
    # the shared eight fields, where frame_lib.h's check_head and hip.FrameCall expect them, then albedo and count
    shared = [(f, getattr(abi.InfillFrames, f).offset) for f, _ in abi.FilterFrames._fields_]
    assert shared == [(f, getattr(abi.FilterFrames, f).offset) for f, _ in abi.FilterFrames._fields_]
    assert [o for _, o in shared[:8]] == [0, 4, 8, 12, 16, 24, 32, 40]
    assert abi.InfillFrames.albedo.offset == 48 and abi.InfillFrames.count.offset == 56


def test_the_workspace_is_48_bytes_per_pixel_and_the_defaults_are_valid():
    lib = abi.infill_lib()
    for w, h in ((1, 1), (3, 5), (1800, 800), (32768, 32768), (0, 7), (0, 0)):
        assert lib.vimg_infill_workspace(w, h) == 48 * w * h
    p = _defaults()
    assert p.struct_size == C.sizeof(abi.InfillParams) and p.radius == 2
    assert 0 < p.sigma_normal < np.inf and 0 < p.sigma_plane < np.inf
    assert 0 < p.albedo_floor < 1 and np.frexp(p.albedo_floor)[0] == 0.5       # a power of two
    # sigma_plane and the floor are the a-trous filter's; sigma_normal is the sweep's
    q = abi.AtrousParams()
    abi.filter_lib().vimg_filter_atrous_defaults(C.byref(q))
    assert (p.sigma_plane, p.albedo_floor) == (q.sigma_plane, q.albedo_floor) and p.sigma_normal == 1.0
    # ... and pass the call's own checks: with them the call gets as far as the launch
    import torch
    if not torch.cuda.is_available():
        rc, msg = _call(**_good_call())
        assert rc == -2 and "launch failed" in msg, (rc, msg)          # VIMG_E_DEVICE, no silent success


def test_the_library_exports_the_four_declared_names_and_leaves_the_other_libraries_alone():
    assert sorted(abi.INFILL_SYMBOLS) == EXPORTS
    abi.infill_lib()                    # loads on a machine without a GPU
    lib = os.path.join(ROOT, "v-img_amd", "lib", "libvimg_infill.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    have = sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("vimg_"))
    assert have == EXPORTS
    for kernel in ("pack", "fill"):
        assert any(f"infill_{kernel}_kernel" in l for l in nm.splitlines()), kernel
    # the shared host skeleton (frames/frame_lib.h) is internal: no error slot and no helper of it is a dynamic symbol
    assert not [l for l in nm.splitlines() if any(w in l for w in ("g_error", "vimg_frames", "4fail", "last_errorEv", "check_", "overlaps"))]
    header = open(os.path.join(ROOT, "include", "vimg_infill.h")).read()
    for name in abi.INFILL_SYMBOLS:
        assert name + "(" in header
    for other in (abi.HIP_SYMBOLS, abi.HIP_TEST_SYMBOLS, abi.FILTER_SYMBOLS, abi.TEMPORAL_SYMBOLS, abi.VARFILTER_SYMBOLS,
                  abi.MOMENTS_SYMBOLS):
        assert not set(abi.INFILL_SYMBOLS) & set(other)
    assert "infill" not in open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read()
    # it links the HIP runtime and none of the project's libraries
    needed = subprocess.run(["readelf", "-d", lib], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libvimg" not in needed.replace("libvimg_infill", "")


def test_the_module_and_the_source_directory_of_the_same_name_do_not_collide():
    import vimg_amd.infill as inf
    assert inf.__file__.endswith("infill.py") and callable(inf.reconstruct) and callable(inf.lattice_mask)
    assert not [f for f in os.listdir(os.path.join(abi.PKG_DIR, "infill")) if f.endswith(".py")]


# ---- 2. argument errors, found before anything is enqueued -------------------------------------------------------
W, H = 8, 4
FRAME, PLANE, CODES, WORK = 12 * W * H, 4 * W * H, W * H, 48 * W * H


def _good_call():
    """Arguments vimg_infill_reconstruct accepts up to the launch (the pointers are never read on the host)."""
    frames = abi.InfillFrames(width=W, height=H, color=0x1000, normal=0x2000, position=0x3000, depth=0x4000, albedo=0x5000,
                              count=0x7000)
    return dict(frames=frames, params=_defaults(), out=0x6000, code=0x8000, workspace=0x10000, nbytes=WORK)


def _call(frames, params, out, code, workspace, nbytes):
    lib = abi.infill_lib()
    rc = lib.vimg_infill_reconstruct(None if frames is None else C.byref(frames), None if params is None else C.byref(params),
                                     C.c_void_p(out), C.c_void_p(code), C.c_void_p(workspace), nbytes, None)
    return rc, lib.vimg_infill_last_error().decode()


def _edit(**kw):
    a = _good_call()
    for k, v in kw.items():
        if k in a:
            a[k] = v
        elif k in dict(abi.InfillFrames._fields_):
            setattr(a["frames"], k, v)
        else:
            setattr(a["params"], k, v)
    return a


NAN, INF = float("nan"), float("inf")
ERRORS = [
    # check_head's, in its order
    (dict(frames=None), "null frames"), (dict(params=None), "null params"),
    (dict(struct_size=63), "frames.struct_size 63 is below the struct's 64"),
    (dict(width=0), "width and height must be 1..32768"), (dict(height=0), "width and height must be 1..32768"),
    (dict(width=32769, nbytes=2 ** 40), "width and height must be 1..32768"),
    (dict(height=32769, nbytes=2 ** 40), "width and height must be 1..32768"),
    (dict(color=None), "null color frame"), (dict(normal=None), "null normal frame"),
    (dict(position=None), "null position frame"), (dict(depth=None), "null depth frame"),
    # the library's own
    (dict(count=None), "null count frame"), (dict(out=None), "null output"),
    (dict(radius=0), "radius must be 1..4, not 0"), (dict(radius=5), "radius must be 1..4, not 5"),
    (dict(sigma_normal=0.0), "sigma_normal must be > 0"), (dict(sigma_normal=-2.0), "sigma_normal must be > 0"),
    (dict(sigma_normal=NAN), "sigma_normal must be > 0"), (dict(sigma_normal=INF), "sigma_normal must be > 0 and finite"),
    (dict(sigma_plane=0.0), "sigma_plane must be > 0"), (dict(sigma_plane=-0.5), "sigma_plane must be > 0"),
    (dict(sigma_plane=NAN), "sigma_plane must be > 0"), (dict(sigma_plane=INF), "sigma_plane must be > 0 and finite"),
    (dict(albedo_floor=0.0), "albedo_floor must be > 0"), (dict(albedo_floor=-0.25), "albedo_floor must be > 0"),
    (dict(albedo_floor=NAN), "albedo_floor must be > 0"), (dict(albedo_floor=INF), "albedo_floor must be > 0 and finite"),
    (dict(workspace=None), "null workspace"),
    (dict(nbytes=WORK - 1), "the workspace has 1535 bytes, 8 x 4 needs 1536"),
    (dict(workspace=0x10008), "the workspace must be 16-byte aligned"),
    # each forbidden overlap: the last byte of one buffer on the first of the other, and the other way round
    (dict(out=0x1000 + 12), "the output overlaps the color frame without being it"),
    (dict(out=0x1000 - FRAME + 1), "the output overlaps the color frame without being it"),
    (dict(out=0x2000), "the output overlaps the normal frame"), (dict(out=0x2000 + FRAME - 1), "the output overlaps the normal frame"),
    (dict(out=0x3000 - FRAME + 1), "the output overlaps the position frame"),
    (dict(out=0x4000), "the output overlaps the depth frame"),
    (dict(out=0x5000 + 4), "the output overlaps the albedo frame"),
    (dict(out=0x7000 + PLANE - 1), "the output overlaps the count frame"), (dict(out=0x7000 - FRAME + 1), "the output overlaps the count frame"),
    (dict(code=0x6000 + FRAME - 1), "the output overlaps the output codes"), (dict(code=0x6000 - CODES + 1), "the output overlaps the output codes"),
    (dict(out=0x10000 + WORK - 1), "the output overlaps the workspace"), (dict(out=0x10000 - FRAME + 1), "the output overlaps the workspace"),
    (dict(code=0x10000 + WORK - 1), "the output codes overlap the workspace"), (dict(code=0x10000 - CODES + 1), "the output codes overlap the workspace"),
]


@pytest.mark.parametrize("edit,sentence", ERRORS, ids=[f"{'-'.join(e)}-{i}" for i, (e, _) in enumerate(ERRORS)])
def test_argument_errors_are_invalid_with_their_sentence_and_need_no_device(edit, sentence):
    rc, msg = _call(**_edit(**edit))
    assert rc == INVALID and msg.startswith("infill: ") and sentence in msg, (rc, msg)


def test_the_checks_come_in_a_fixed_order():
    """Two faults at once: the one that comes first in check_head's order, then the library's, is reported."""
    order = [dict(struct_size=63), dict(width=0), dict(depth=None), dict(count=None), dict(out=None), dict(radius=9),
             dict(sigma_normal=NAN), dict(sigma_plane=NAN), dict(albedo_floor=NAN), dict(workspace=None), dict(nbytes=1)]
    sentences = ["frames.struct_size", "width and height", "null depth frame", "null count frame", "null output", "radius must be",
                 "sigma_normal must be", "sigma_plane must be", "albedo_floor must be", "null workspace", "the workspace has"]
    for i in range(len(order) - 1):
        rc, msg = _call(**_edit(**order[i], **order[i + 1]))
        assert rc == INVALID and sentences[i] in msg, (i, msg)


def test_params_struct_size_and_what_may_be_null_or_touch():
    a = _good_call()
    a["params"].struct_size = 19
    rc, msg = _call(**a)
    assert rc == INVALID and "params.struct_size 19 is below the struct's 20" in msg
    # albedo and the codes may be NULL, the output may be the colour frame, and buffers may touch end to start: the
    # call passes every argument check
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(albedo=None), dict(code=None), dict(out=0x1000), dict(out=0x2000 - FRAME), dict(out=0x2000 + FRAME),
                   dict(code=0x6000 + FRAME), dict(out=0x10000 + WORK), dict(radius=1), dict(radius=4)):
            rc, msg = _call(**_edit(**ok))
            assert rc == -2 and "launch failed" in msg, (ok, rc, msg)


# ---- 3. the lattices ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [2, 3, 4])
def test_the_phases_of_a_stride_partition_the_frame(stride):
    from vimg_amd import infill
    h, w = 5, 7
    masks = [infill.lattice_mask(h, w, stride, ph, device="cpu").numpy() for ph in range(stride * stride)]
    assert all(m.dtype == np.uint8 and m.shape == (h, w) and set(np.unique(m)) <= {0, 1} for m in masks)
    assert np.array_equal(sum(m.astype(int) for m in masks), np.ones((h, w), int))          # every pixel exactly once
    cells = [infill.lattice_cell(stride, ph) for ph in range(stride * stride)]
    assert sorted(cells) == [(x, y) for x in range(stride) for y in range(stride)]
    for ph, (cx, cy) in enumerate(cells):
        assert (cx, cy) == (ph % stride, (ph // stride + ph % stride) % stride)              # the documented order
        assert np.array_equal(masks[ph].astype(bool), R.lattice(h, w, stride, cx, cy))
    # the first `stride` phases touch every row and every column of cells
    assert sorted(c[0] for c in cells[:stride]) == sorted(c[1] for c in cells[:stride]) == list(range(stride))
    assert cells[0] == (0, 0)
    for bad in ((stride, -1), (stride, stride * stride), (1, 0), (5, 0)):
        with pytest.raises(ValueError, match="infill: "):
            infill.lattice_mask(h, w, *bad, device="cpu")


# ---- 4. the restatement, pinned on its own against hand-computed cases ---------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _flat(h, w, z=8.0):
    """A plane facing the camera: normal (0, 0, 1), positions on z = -8 a unit apart, depth 8."""
    yy, xx = np.mgrid[0:h, 0:w]
    normal = np.zeros((h, w, 3), F)
    normal[..., 2] = 1
    position = np.stack([xx, yy, np.full_like(xx, -z)], -1).astype(F)
    return normal, position, np.full((h, w, 3), z, F)


KW = dict(radius=1, sigma_normal=0.5, sigma_plane=0.125, albedo_floor=1 / 64)


def test_three_by_three_with_one_sampled_centre():
    """Every other pixel has the centre as its only tap, S = 0 exactly, w = k (1 for a corner, 2 for an edge):
    (k c) / k = c exactly.  With albedo 1/2 at the centre and 1/4 elsewhere: out = (c / 0.5) 0.25 = c / 2."""
    normal, position, depth = _flat(3, 3)
    color = np.arange(27, dtype=F).reshape(3, 3, 3) + F(100)            # the unsampled pixels' own colours are never read
    centre = np.array([0.3, 1.7, 2.9], F)
    color[1, 1] = centre
    count = np.zeros((3, 3), np.uint32)
    count[1, 1] = 7
    out, code = R.reconstruct(color, normal, position, depth, count, **KW)
    assert out.dtype == F and code.dtype == np.uint8
    assert np.array_equal(_bits(out), _bits(np.broadcast_to(centre, (3, 3, 3))))
    assert np.array_equal(code, [[1, 1, 1], [1, 0, 1], [1, 1, 1]])
    albedo = np.full((3, 3, 3), 0.25, F)
    albedo[1, 1] = 0.5
    out, code = R.reconstruct(color, normal, position, depth, count, albedo, **KW)
    want = np.broadcast_to(centre * F(0.5), (3, 3, 3)).copy()
    want[1, 1] = centre                                                 # the sampled pixel: a copy
    assert np.array_equal(_bits(out), _bits(want)) and code[1, 1] == 0 and (code.sum() == 8)
    # radius 2 reaches the same single tap with other weights: k = (3 - 1)(3 - 1) = 4 for a corner, exact again, and
    # (3 - 1)(3 - 0) = 6 for an edge, where (6 C) / 6 rounds twice
    out2, code2 = R.reconstruct(color, normal, position, depth, count, albedo, **dict(KW, radius=2))
    C = centre / F(0.5)
    want[0, 1] = want[1, 0] = want[1, 2] = want[2, 1] = ((F(6) * C) / F(6)) * F(0.25)
    assert np.array_equal(_bits(out2), _bits(want)) and np.array_equal(code2, code)


def test_two_taps_are_weighted_by_the_tent_and_the_plane_distance():
    """1 x 3, the ends sampled, radius 1: both taps have k = float(1 * 2) = 2.  Coplanar: (2 * 1 + 2 * 3) / 4 = 2.
    The right tap 0.5 off p's tangent plane at sigma_plane z = 1: s_p = 0.25, w = 2 (0.75 * 0.75) = 1.125, and the
    result is (2 * 1 + 1.125 * 3) / (2 + 1.125) = 5.375 / 3.125 in float32."""
    normal, position, depth = _flat(1, 3)
    color = np.array([[[1, 1, 1], [9, 9, 9], [3, 3, 3]]], F)
    count = np.array([[1, 0, 2]], np.uint32)
    out, code = R.reconstruct(color, normal, position, depth, count, **KW)
    assert np.array_equal(code, [[0, 1, 0]]) and np.array_equal(_bits(out[0, 1]), _bits(np.full(3, 2, F)))
    assert np.array_equal(_bits(out[0, ::2]), _bits(color[0, ::2]))
    position[0, 2, 2] += F(0.5)
    out, code = R.reconstruct(color, normal, position, depth, count, **KW)
    assert np.array_equal(code, [[0, 1, 0]])
    assert np.array_equal(_bits(out[0, 1]), _bits(np.full(3, F(5.375) / F(3.125), F)))
    # at 1 off the plane s_p = 1: S < 1 fails, the tap is out and the left one alone remains
    position[0, 2, 2] += F(0.5)
    out, code = R.reconstruct(color, normal, position, depth, count, **KW)
    assert np.array_equal(code, [[0, 1, 0]]) and np.array_equal(_bits(out[0, 1]), _bits(np.full(3, 1, F)))


def test_a_normal_step_forces_the_unguided_fallback():
    """The left column faces +x: 1 - n_p . n_q = 1, s_n = 1 / 0.5 = 2, no guided tap - the centre is taken with its tent
    weight, code 2.  A miss (depth 0) beside a live sampled pixel falls back the same way and is not multiplied by albedo;
    a NaN normal makes S NaN, which is no weight either."""
    normal, position, depth = _flat(3, 3)
    normal[:, 0] = (1, 0, 0)
    normal[0, 2, 0] = np.nan
    depth[2, 2] = 0
    color = np.zeros((3, 3, 3), F)
    centre = np.array([0.3, 1.7, 2.9], F)
    color[1, 1] = centre
    count = np.zeros((3, 3), np.int64)
    count[1, 1] = 1
    albedo = np.full((3, 3, 3), 0.5, F)
    out, code = R.reconstruct(color, normal, position, depth, count, albedo, **KW)
    assert np.array_equal(code, [[2, 1, 2], [2, 0, 1], [2, 1, 2]])
    C = centre / F(0.5)
    want = np.broadcast_to(C * F(0.5), (3, 3, 3)).copy()
    want[2, 2] = C                                                      # not live: C_p as it is
    want[1, 1] = centre
    assert np.array_equal(_bits(out), _bits(want))


def test_misses_continue_the_background_and_not_the_surface():
    """1 x 5: miss, MISS (unsampled), live, LIVE (unsampled), live.  The unsampled miss takes the sampled miss (code 1,
    w = k) although a live sampled pixel is as near; the unsampled live pixel takes its two live neighbours."""
    normal, position, depth = _flat(1, 5)
    depth[0, :2] = 0
    color = np.array([[[4, 4, 4], [0, 0, 0], [1, 1, 1], [0, 0, 0], [2, 2, 2]]], F)
    count = np.array([[1, 0, 1, 0, 1]], np.uint32)
    out, code = R.reconstruct(color, normal, position, depth, count, **KW)
    assert np.array_equal(code, [[0, 1, 0, 1, 0]])
    assert np.array_equal(out[0, :, 0], np.array([4, 4, 1, 1.5, 2], F))


def test_an_all_unsampled_frame_is_holes_and_an_all_sampled_frame_is_itself():
    f = R.creased_frames(9, 13)
    f["color"][4, 5, 1] = np.nan
    guides = [f[k] for k in ("normal", "position", "depth")]
    for albedo in (None, f["albedo"]):
        for radius in (1, 4):
            kw = dict(default_kw(), radius=radius)
            out, code = R.reconstruct(f["color"], *guides, np.zeros((9, 13), np.uint32), albedo, **kw)
            assert np.array_equal(code, np.full((9, 13), 3)) and np.array_equal(_bits(out), np.zeros((9, 13, 3), np.uint32))
            out, code = R.reconstruct(f["color"], *guides, np.full((9, 13), 5, np.uint32), albedo, **kw)
            assert np.array_equal(code, np.zeros((9, 13))) and np.array_equal(_bits(out), _bits(f["color"]))


def test_a_nan_colour_stays_and_reaches_the_pixels_it_is_a_tap_of():
    normal, position, depth = _flat(7, 9)
    color = np.ones((7, 9, 3), F)
    count = R.lattice(7, 9, 2).astype(np.uint32)
    color[2, 4, 1] = np.nan                                             # a sampled pixel of the lattice
    out, code = R.reconstruct(color, normal, position, depth, count, **dict(KW, radius=1))
    nan = np.isnan(out)
    assert nan[..., 1][1:4, 3:6].all() and nan.sum() == 9 and not nan[..., 0].any()
    assert code[2, 4] == 0 and np.isnan(out[2, 4, 1])


@pytest.mark.parametrize("stride", [2, 3, 4])
def test_a_full_lattice_leaves_no_hole_from_radius_stride_minus_one_on(stride):
    """9 x 7 (and the smallest frame, stride x stride), every phase: each pixel has a sampled pixel within stride - 1."""
    from vimg_amd import infill
    for h, w in ((7, 9), (stride, stride)):
        f = R.creased_frames(h, w)
        for phase in range(stride * stride):
            count = R.lattice(h, w, stride, *infill.lattice_cell(stride, phase)).astype(np.uint32)
            for radius in range(stride - 1, 5):
                if radius < 1:
                    continue
                out, code = R.reconstruct(f["color"], f["normal"], f["position"], f["depth"], count, f["albedo"],
                                          **dict(default_kw(), radius=radius))
                assert not (code == 3).any(), (h, w, phase, radius)
                assert np.array_equal(code == 0, count > 0)
                assert np.isfinite(out).all()
