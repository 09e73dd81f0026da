"""The weighted temporal library at its boundary, without a GPU: include/vimg_wtemporal.h against its ctypes mirror, the
exports of libvimg_wtemporal.so, every argument error of vimg_wtemporal_accumulate, and the numpy restatement of its
contract (tests/wtemporal_ref.py) pinned on its own: against tests/temporal_ref.py at uniform weights, against cases
worked out by hand for each code, and on a synthetic sequence of sparse frames."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import infill_ref as IR
import temporal_ref as TR
import wtemporal_ref as R
from abi_layout import c_layout, ctypes_layout
from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # VIMG_E_INVALID
F = np.float32
EXPORTS = ["vimg_wtemporal_accumulate", "vimg_wtemporal_defaults", "vimg_wtemporal_last_error"]
PARAMS = dict(max_history=32, sigma_normal=0.1, sigma_plane=0.01)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _defaults():
    p = abi.WTemporalParams()
    abi.wtemporal_lib().vimg_wtemporal_defaults(C.byref(p))
    return p


# ---- 1. header and ctypes ------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_structs(tmp_path):
    structs = {"VimgWTemporalFrames": abi.WTemporalFrames, "VimgWTemporalParams": abi.WTemporalParams}
    got = c_layout(tmp_path, ["vimg_wtemporal.h"], structs,
                   'printf("per_pixel %u\\n", VIMG_WTEMPORAL_HISTORY_PER_PIXEL);'
                   'printf("what %u %u %u %u %u\\n", VIMG_WTEMPORAL_DEAD, VIMG_WTEMPORAL_STARTED, VIMG_WTEMPORAL_BLENDED, '
                   'VIMG_WTEMPORAL_CARRIED, VIMG_WTEMPORAL_SHOWN);')
    assert got.pop("per_pixel") == "48" == str(abi.TEMPORAL_HISTORY_PER_PIXEL)
    assert got.pop("what 0 1 2 3") == "4"
    assert (abi.WTEMPORAL_DEAD, abi.WTEMPORAL_STARTED, abi.WTEMPORAL_BLENDED, abi.WTEMPORAL_CARRIED, abi.WTEMPORAL_SHOWN) \
        == (0, 1, 2, 3, 4) == (R.DEAD, R.STARTED, R.BLENDED, R.CARRIED, R.SHOWN)
    assert got == ctypes_layout(structs)
    assert C.sizeof(abi.WTemporalFrames) == 56 and C.sizeof(abi.WTemporalParams) == 20
    assert abi.WTemporalFrames().struct_size == 56 and abi.WTemporalParams().struct_size == 20
    # the shared eight fields, where frame_lib.h's check_head and hip.FrameCall expect them, then the weight frame
    shared = ("struct_size", "width", "height", "reserved", "color", "normal", "position", "depth")
    assert [f for f, _ in abi.WTemporalFrames._fields_] == list(shared) + ["weight"]
    assert [got[f"VimgWTemporalFrames.{f}"] for f in shared] == ["0", "4", "8", "12", "16", "24", "32", "40"]
    assert [getattr(abi.WTemporalFrames, f).offset for f in shared] == [getattr(abi.TemporalFrames, f).offset for f in shared]
    assert abi.WTemporalFrames.weight.offset == 48
    assert [f for f, _ in abi.WTemporalParams._fields_] == ["struct_size", "reserved", "max_history", "sigma_normal", "sigma_plane"]


def test_the_defaults_are_the_temporal_librarys_and_valid():
    p, q = _defaults(), abi.TemporalParams()
    abi.temporal_lib().vimg_temporal_defaults(C.byref(q))
    assert p.struct_size == C.sizeof(abi.WTemporalParams) == 20 and p.reserved == 0
    assert (p.max_history, p.sigma_normal, p.sigma_plane) == (q.max_history, q.sigma_normal, q.sigma_plane)
    assert (p.max_history, p.sigma_normal, p.sigma_plane) == (32.0, F(0.1), F(0.00005))
    # ... and the call takes them.  Its pointers are made up, so it is only made where no device could follow them:
    # there it passes every argument check and fails at the launch
    import torch
    if not torch.cuda.is_available():
        rc, msg = _call(**_good_call())
        assert rc == -2 and "launch failed" in msg, (rc, msg)          # VIMG_E_DEVICE, no silent success


def test_the_library_exports_the_three_declared_names_and_leaves_the_other_libraries_alone():
    assert sorted(abi.WTEMPORAL_SYMBOLS) == EXPORTS
    abi.wtemporal_lib()                    # loads on a machine without a GPU
    lib = os.path.join(ROOT, "v-img_amd", "lib", "libvimg_wtemporal.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    have = sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("vimg_"))
    assert have == EXPORTS
    assert any("wtemporal_accumulate_kernel" in l for l in nm.splitlines())       # ... and its kernel is in it
    # the shared host skeleton (frames/frame_lib.h) is internal: no error slot and no helper of it is a dynamic symbol
    assert not [l for l in nm.splitlines() if any(w in l for w in ("g_error", "vimg_frames", "4fail", "last_errorEv", "check_", "overlaps"))]
    header = open(os.path.join(ROOT, "include", "vimg_wtemporal.h")).read()
    for name in abi.WTEMPORAL_SYMBOLS:
        assert name + "(" in header
    for other in (abi.HIP_SYMBOLS, abi.HIP_TEST_SYMBOLS, abi.FILTER_SYMBOLS, abi.TEMPORAL_SYMBOLS, abi.VARFILTER_SYMBOLS,
                  abi.MOMENTS_SYMBOLS, abi.INFILL_SYMBOLS):
        assert not set(abi.WTEMPORAL_SYMBOLS) & set(other)
    assert "wtemporal" not in open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read()
    # it links the HIP runtime and none of the project's libraries
    needed = subprocess.run(["readelf", "-d", lib], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libvimg" not in needed.replace("libvimg_wtemporal", "")


def test_the_module_and_the_source_directory_of_the_same_name_do_not_collide():
    import vimg_amd.wtemporal as wt
    from vimg_amd import temporal
    assert wt.__file__.endswith("wtemporal.py") and callable(wt.accumulate) and callable(wt.sparse_weights)
    assert not [f for f in os.listdir(os.path.join(abi.PKG_DIR, "wtemporal")) if f.endswith(".py")]
    # the history is the temporal library's: its class and its byte count, no second ones
    assert wt.History is temporal.History and wt.history_bytes is temporal.history_bytes
    assert 0 <= wt.FILL_WEIGHT <= 1


# ---- 2. argument errors, found before anything is enqueued -------------------------------------------------------
W, H = 8, 4
FRAME, PLANE, CODES, HIST = 12 * W * H, 4 * W * H, W * H, 48 * W * H


def _good_call():
    """Arguments vimg_wtemporal_accumulate accepts up to the launch (the device pointers are never read on the host)."""
    frames = abi.WTemporalFrames(width=W, height=H, color=0x1000, normal=0x2000, position=0x3000, depth=0x4000, weight=0x5000)
    return dict(frames=frames, prev=0x10000, matrix=TR.IDENTITY.tolist(), params=_defaults(), next=0x20000, out=0x6000, code=0x7000)


def _call(frames, prev, matrix, params, next, out, code):
    lib = abi.wtemporal_lib()
    m = None if matrix is None else (abi.f32 * 12)(*matrix)
    rc = lib.vimg_wtemporal_accumulate(None if frames is None else C.byref(frames), C.c_void_p(prev), m,
                                       None if params is None else C.byref(params), C.c_void_p(next), C.c_void_p(out),
                                       C.c_void_p(code), None)
    return rc, lib.vimg_wtemporal_last_error().decode()


def _edit(**kw):
    a = _good_call()
    for k, v in kw.items():
        if k.startswith("m") and k[1:].isdigit():
            a["matrix"][int(k[1:])] = v
        elif k in a:
            a[k] = v
        elif k in dict(abi.WTemporalFrames._fields_):
            setattr(a["frames"], k, v)
        else:
            assert k in dict(abi.WTemporalParams._fields_), k
            setattr(a["params"], k, v)
    return a


NAN, INF = float("nan"), float("inf")
ERRORS = [
    # check_head's, in its order
    (dict(frames=None), "wtemporal: null frames"), (dict(params=None), "wtemporal: null params"),
    (dict(struct_size=55), "wtemporal: frames.struct_size 55 is below the struct's 56"),
    (dict(width=0), "wtemporal: width and height must be 1..32768, not 0 x 4"),
    (dict(height=0), "wtemporal: width and height must be 1..32768, not 8 x 0"),
    (dict(width=32769), "wtemporal: width and height must be 1..32768, not 32769 x 4"),
    (dict(height=32769), "wtemporal: width and height must be 1..32768, not 8 x 32769"),
    (dict(color=None), "wtemporal: null color frame"), (dict(normal=None), "wtemporal: null normal frame"),
    (dict(position=None), "wtemporal: null position frame"), (dict(depth=None), "wtemporal: null depth frame"),
    # the library's own
    (dict(weight=None), "wtemporal: null weight frame"), (dict(next=None), "wtemporal: null next history"),
    (dict(max_history=0.5), "wtemporal: max_history must be >= 1 and finite, not 0.5"),
    (dict(max_history=NAN), "wtemporal: max_history must be >= 1 and finite, not nan"),
    (dict(max_history=INF), "wtemporal: max_history must be >= 1 and finite, not inf"),
    (dict(max_history=-2.0), "wtemporal: max_history must be >= 1 and finite, not -2"),
    (dict(sigma_normal=0.0), "wtemporal: sigma_normal must be > 0 and finite, not 0"),
    (dict(sigma_normal=-1.0), "wtemporal: sigma_normal must be > 0 and finite, not -1"),
    (dict(sigma_normal=NAN), "wtemporal: sigma_normal must be > 0 and finite, not nan"),
    (dict(sigma_normal=INF), "wtemporal: sigma_normal must be > 0 and finite, not inf"),
    (dict(sigma_plane=0.0), "wtemporal: sigma_plane must be > 0 and finite, not 0"),
    (dict(sigma_plane=-0.5), "wtemporal: sigma_plane must be > 0 and finite, not -0.5"),
    (dict(sigma_plane=NAN), "wtemporal: sigma_plane must be > 0 and finite, not nan"),
    (dict(sigma_plane=INF), "wtemporal: sigma_plane must be > 0 and finite, not inf"),
    (dict(next=0x20008), "wtemporal: the next history must be 16-byte aligned"),
    (dict(weight=0x5002), "wtemporal: the weight frame must be 4-byte aligned"),
    (dict(prev=0x10004), "wtemporal: the previous history must be 16-byte aligned"),
    (dict(matrix=None), "wtemporal: a previous history needs its world-to-pixel matrix"),
    (dict(m0=NAN), "wtemporal: world-to-pixel entry 0 is not finite (nan)"),
    (dict(m7=INF), "wtemporal: world-to-pixel entry 7 is not finite (inf)"),
    (dict(m11=-INF), "wtemporal: world-to-pixel entry 11 is not finite (-inf)"),
    (dict(prev=None, m5=NAN), "wtemporal: world-to-pixel entry 5 is not finite (nan)"),
    # each forbidden overlap: the last byte of one buffer on the first of the other
    (dict(next=0x10000 + HIST - 16), "wtemporal: the next history overlaps the previous one"),
    (dict(next=0x10000 - HIST + 16), "wtemporal: the next history overlaps the previous one"),
    (dict(next=0x1000), "wtemporal: the next history overlaps the color frame"),
    (dict(next=0x2000 + FRAME - 16), "wtemporal: the next history overlaps the normal frame"),
    (dict(next=0x3000), "wtemporal: the next history overlaps the position frame"),
    (dict(next=0x4000 - HIST + 16), "wtemporal: the next history overlaps the depth frame"),
    (dict(next=0x5000 + PLANE - 16, out=None, code=None), "wtemporal: the next history overlaps the weight frame"),
    (dict(next=0x5000 - HIST + 16, depth=0x40000), "wtemporal: the next history overlaps the weight frame"),
    (dict(out=0x10000 + HIST - 4), "wtemporal: the output overlaps the previous history"),
    (dict(out=0x20000 - FRAME + 4), "wtemporal: the output overlaps the next history"),
    (dict(out=0x1004), "wtemporal: the output overlaps the color frame without being it"),
    (dict(out=0x1000 - FRAME + 4), "wtemporal: the output overlaps the color frame without being it"),
    (dict(out=0x2000), "wtemporal: the output overlaps the normal frame"),
    (dict(out=0x3000 - FRAME + 4), "wtemporal: the output overlaps the position frame"),
    (dict(out=0x4000 + FRAME - 4), "wtemporal: the output overlaps the depth frame"),
    (dict(out=0x5000 + PLANE - 4), "wtemporal: the output overlaps the weight frame"),
    (dict(out=0x5000 - FRAME + 4, depth=0x40000), "wtemporal: the output overlaps the weight frame"),
    (dict(code=0x10000 + HIST - 1), "wtemporal: the output codes overlap the previous history"),
    (dict(code=0x20000 - CODES + 1), "wtemporal: the output codes overlap the next history"),
    (dict(code=0x1000 + FRAME - 1), "wtemporal: the output codes overlap the color frame"),
    (dict(code=0x2000 - CODES + 1), "wtemporal: the output codes overlap the normal frame"),
    (dict(code=0x3000), "wtemporal: the output codes overlap the position frame"),
    (dict(code=0x4000 + FRAME - 1), "wtemporal: the output codes overlap the depth frame"),
    (dict(code=0x5000 + PLANE - 1), "wtemporal: the output codes overlap the weight frame"),
    (dict(code=0x5000 - CODES + 1), "wtemporal: the output codes overlap the weight frame"),
    (dict(code=0x6000 + FRAME - 1), "wtemporal: the output codes overlap the output"),
    (dict(code=0x6000 - CODES + 1), "wtemporal: the output codes overlap the output"),
]


@pytest.mark.parametrize("edit,sentence", ERRORS, ids=[f"{'-'.join(e)}-{i}" for i, (e, _) in enumerate(ERRORS)])
def test_argument_errors_are_invalid_with_their_whole_sentence_and_need_no_device(edit, sentence):
    rc, msg = _call(**_edit(**edit))
    assert rc == INVALID and msg == sentence, (rc, msg)


def test_the_checks_come_in_a_fixed_order():
    """Two faults at once: the one that comes first in check_head's order, then the library's, is reported."""
    order = [dict(struct_size=55), dict(width=0), dict(depth=None), dict(weight=None), dict(next=None), dict(max_history=NAN),
             dict(sigma_normal=NAN), dict(sigma_plane=NAN), dict(weight=0x5001), dict(prev=0x10008), dict(m3=NAN)]
    sentences = ["frames.struct_size", "width and height", "null depth frame", "null weight frame", "null next history",
                 "max_history must be", "sigma_normal must be", "sigma_plane must be", "the weight frame must be",
                 "the previous history must be", "world-to-pixel entry 3"]
    for i in range(len(order) - 1):
        if set(order[i]) & set(order[i + 1]):
            continue
        rc, msg = _call(**_edit(**order[i], **order[i + 1]))
        assert rc == INVALID and sentences[i] in msg, (i, msg)


def test_params_struct_size_the_slot_of_its_own_and_what_is_not_an_error():
    a = _good_call()
    a["params"].struct_size = 19
    rc, msg = _call(**a)
    assert rc == INVALID and msg == "wtemporal: params.struct_size 19 is below the struct's 20"
    # the last-error slot is this library's: a failure of libvimg_temporal leaves it alone, and the other way round
    import test_temporal_abi as TA
    tmp, wtm = abi.temporal_lib(), abi.wtemporal_lib()
    fail_w = lambda: _call(**_edit(max_history=0.25))
    fail_t = lambda: TA._call(**TA._edit(sigma_plane=-3.0))
    for first, second in ((fail_w, fail_t), (fail_t, fail_w)):
        assert first()[0] == INVALID and second()[0] == INVALID
        assert wtm.vimg_wtemporal_last_error().decode() == "wtemporal: max_history must be >= 1 and finite, not 0.25"
        assert tmp.vimg_temporal_last_error().decode() == "temporal: sigma_plane must be > 0 and finite, not -3"
        first()
        assert wtm.vimg_wtemporal_last_error().decode().startswith("wtemporal: max_history")
        assert tmp.vimg_temporal_last_error().decode().startswith("temporal: sigma_plane")
    # no history and no matrix, no output, no codes, an output that is the colour frame, buffers that touch end to
    # start: all pass every argument check (and only then need a device)
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(prev=None, matrix=None), dict(out=None), dict(code=None), dict(out=None, code=None), dict(out=0x1000),
                   dict(next=0x10000 + HIST), dict(code=0x6000 + FRAME), dict(code=0x5000 + PLANE), dict(max_history=1.0)):
            rc, msg = _call(**_edit(**ok))
            assert rc == -2 and "launch failed" in msg, (ok, rc, msg)          # VIMG_E_DEVICE, no silent success


# ---- 3. the restatement, pinned on its own -----------------------------------------------------------------------
def _random_case(w, h):
    import test_temporal as TT
    return TT.random_case(w, h), TT.matrices(w, h)


@pytest.mark.parametrize("size", [(5, 3), (67, 5)], ids=["5x3", "67x5"])
def test_uniform_weights_from_one_up_give_the_temporal_restatements_bits(size):
    """(a) With every weight one value v >= 1 the contract is vimg_temporal_accumulate's at current_weight = v."""
    w, h = size
    (f, prev), ms = _random_case(w, h)
    kw = dict(max_history=6.0, sigma_normal=0.05, sigma_plane=0.02)
    blended = 0
    for name, m in ms.items():
        for v in (1, 2, 3.5, 7):
            want = TR.accumulate(f["color"], f["normal"], f["position"], f["depth"], prev, m, current_weight=v, **kw)
            got, code = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], np.full((h, w), v, F), prev, m, **kw)
            assert np.array_equal(_bits(got), _bits(want)), (name, v)
            L = want[0, ..., 3]
            assert np.array_equal(code == R.DEAD, L == 0) and set(np.unique(code)) <= {R.DEAD, R.STARTED, R.BLENDED}
            assert ((code == R.STARTED) <= (L == 1)).all()
            blended += int((code == R.BLENDED).sum())
    assert blended > 0
    want = TR.accumulate(f["color"], f["normal"], f["position"], f["depth"], None, None, current_weight=2, **kw)
    got, code = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], np.full((h, w), 2, F), None, None, **kw)
    assert np.array_equal(_bits(got), _bits(want))


def _pair(weights, lengths=(3.0, 3.0), live=(True, True), history=True, shift=0.0, max_history=32):
    """A 1 x 2 picture of the flat wall: history colour 0.7 of the given lengths, current colour 0.2."""
    f = TR.flat_frames(1, 2, 0.2)
    for x in (0, 1):
        if not live[x]:
            f["depth"][0, x] = 0
    prev = None
    if history:
        g = TR.flat_frames(1, 2, 0.7)
        prev = TR.accumulate(g["color"], g["normal"], g["position"], g["depth"], None, None, current_weight=1, **PARAMS)
        prev[0, 0, :, 3] = lengths
    nxt, code = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], np.array([weights], F), prev,
                             TR.shift_matrix(shift) if history else None, **dict(PARAMS, max_history=max_history))
    return nxt[0, 0], code[0]


def test_each_code_by_hand_on_one_by_two():
    """(b) H = 0.7 of length 3, C = 0.2; weights 0, 0.25, 1, NaN, -1, inf."""
    H, Cc = F(0.7), F(0.2)
    rgb = lambda v: np.full(3, v, F)
    # code 0: not live, whatever the weight - {C, 0}
    A, code = _pair([1.0, 0.0], live=(False, False))
    assert list(code) == [0, 0] and (A[:, 3] == 0).all() and np.array_equal(_bits(A[:, :3]), _bits(np.stack([rgb(Cc)] * 2)))
    # code 1: no history - {C, min(wt, 1)}: 0.25 stays 0.25, 1 is 1, inf is 1
    A, code = _pair([0.25, 1.0], history=False)
    assert list(code) == [1, 1] and list(A[:, 3]) == [0.25, 1.0] and np.array_equal(_bits(A[0, :3]), _bits(rgb(Cc)))
    A, code = _pair([INF, 3.0], history=False)
    assert list(code) == [1, 1] and list(A[:, 3]) == [1.0, 1.0]
    # ... and a history that is there but of length 0 at the tapped pixel is none
    A, code = _pair([0.25, 0.0], lengths=(0.0, 0.0))
    assert list(code) == [1, 4] and list(A[:, 3]) == [0.25, 0.0]
    # code 2: N = 3 + wt, a = wt / N
    A, code = _pair([0.25, 1.0])
    assert list(code) == [2, 2] and list(A[:, 3]) == [3.25, 4.0]
    assert np.array_equal(_bits(A[0, :3]), _bits(rgb(H + (Cc - H) * (F(0.25) / F(3.25)))))
    assert np.array_equal(_bits(A[1, :3]), _bits(rgb(H + (Cc - H) * F(0.25))))
    # ... capped: max_history 3.5 gives N = 3.5, a = 1 / 3.5; weight inf gives N = 32, a = inf / 32 cut to 1
    A, code = _pair([1.0, INF], max_history=3.5)
    assert list(code) == [2, 2] and list(A[:, 3]) == [3.5, 3.5]
    assert np.array_equal(_bits(A[0, :3]), _bits(rgb(H + (Cc - H) * (F(1) / F(3.5)))))
    assert np.array_equal(_bits(A[1, :3]), _bits(rgb(H + (Cc - H) * F(1))))
    # code 3: weight 0, NaN, -1 - the history alone, its length kept (and capped)
    for wts in ([0.0, NAN], [-1.0, -0.0]):
        A, code = _pair(wts, lengths=(3.0, 40.0))
        assert list(code) == [3, 3] and list(A[:, 3]) == [3.0, 32.0]
        assert np.array_equal(_bits(A[:, :3]), _bits(np.stack([rgb(H)] * 2)))
    # ... and C does not enter: a NaN colour stays out
    f = TR.flat_frames(1, 2, np.nan)
    g = TR.flat_frames(1, 2, 0.7)
    prev = TR.accumulate(g["color"], g["normal"], g["position"], g["depth"], None, None, current_weight=1, **PARAMS)
    nxt, code = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], np.zeros((1, 2), F), prev, TR.IDENTITY, **PARAMS)
    assert list(code[0]) == [3, 3] and np.array_equal(_bits(nxt[0, 0, :, :3]), _bits(np.stack([rgb(H)] * 2)))
    # code 4: weight 0 (NaN, -1) and no history - {C, 0}; with a shift of one column pixel 0 looks off the image
    A, code = _pair([0.0, NAN], history=False)
    assert list(code) == [4, 4] and (A[:, 3] == 0).all() and np.array_equal(_bits(A[:, :3]), _bits(np.stack([rgb(Cc)] * 2)))
    A, code = _pair([-1.0, 0.0], shift=-1.0)
    assert list(code) == [4, 3] and list(A[:, 3]) == [0.0, 3.0]
    assert np.array_equal(_bits(A[0, :3]), _bits(rgb(Cc))) and np.array_equal(_bits(A[1, :3]), _bits(rgb(H)))
    # what a code 4 pixel leaves is nobody's tap in the next step
    f = TR.flat_frames(1, 2, 0.2)
    first, code = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], np.array([[0.0, 1.0]], F), None, None, **PARAMS)
    assert list(code[0]) == [4, 1]
    second, code = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], np.array([[0.0, 1.0]], F), first, TR.IDENTITY, **PARAMS)
    assert list(code[0]) == [4, 2] and list(second[0, 0, :, 3]) == [0.0, 2.0]


INFILL_DEFAULTS = dict(radius=2, sigma_normal=1.0, sigma_plane=0.005, albedo_floor=1 / 64)
TEMPORAL_DEFAULTS = dict(max_history=32, sigma_normal=0.1, sigma_plane=0.00005)


def sparse_sequence_error(seed, fill_weight, stride=2, frames=8):
    """tests/temporal_ref.py's synthetic sequence at 16 x 32, `frames` frames; each frame samples the lattice
    infill.lattice_cell(stride, i mod stride^2), is filled by infill_ref.reconstruct at the infill library's defaults and
    accumulated by wtemporal_ref at the temporal defaults with weight 1 where sampled, fill_weight where the fill is
    guided, 0 elsewhere.  (e of the last accumulated frame, e of the last filled frame alone) over its hit pixels,
    against `clean`."""
    from vimg_amd import infill
    seq = TR.synthetic_sequence(16, 32, frames=frames, seed=seed)
    hist = None
    for i, f in enumerate(seq):
        count = IR.lattice(16, 32, stride, *infill.lattice_cell(stride, i % (stride * stride))).astype(np.uint32)
        filled, code = IR.reconstruct(f["color"], f["normal"], f["position"], f["depth"], count, **INFILL_DEFAULTS)
        weight = np.where(count > 0, F(1), np.where(code == IR.GUIDED, F(fill_weight), F(0))).astype(F)
        hist, _ = R.accumulate(filled, f["normal"], f["position"], f["depth"], weight, hist, seq[i - 1]["matrix"] if i else None,
                               **TEMPORAL_DEFAULTS)
    last = seq[-1]
    return IR.rel_error(hist[0, ..., :3], last["clean"], last["hit"]), IR.rel_error(filled, last["clean"], last["hit"])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sparse_frames_with_history_beat_the_fill_alone_and_weight_one_is_worse_than_the_default(seed):
    """(c) On the restatements alone, at vimg_amd.wtemporal.FILL_WEIGHT: e(sparse + history) < e(fill alone), and
    counting a filled pixel as one real sample - what vimg_temporal_accumulate would do - is worse than the default.
    Measured at 1/16, seeds 1 / 2 / 3: fill alone 0.3514 / 0.3812 / 0.3546, with history 0.3082 / 0.3138 / 0.3053 (ratios
    0.877 / 0.823 / 0.861), at fill weight 1 0.4622 / 0.4285 / 0.4493; DESIGN.md 4.24 has the other weights."""
    from vimg_amd import wtemporal
    e_default, e_fill = sparse_sequence_error(seed, wtemporal.FILL_WEIGHT)
    e_one, _ = sparse_sequence_error(seed, 1.0)
    print(f"seed {seed}: fill alone {e_fill:.4f}, fill_weight {wtemporal.FILL_WEIGHT:g} {e_default:.4f} "
          f"(ratio {e_default / e_fill:.3f}), fill_weight 1 {e_one:.4f}")
    assert e_default < e_fill
    assert e_one > e_default
