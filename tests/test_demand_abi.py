"""The sampling mask at its boundary, without a GPU: include/vimg_demand.h against its ctypes mirror, the exports of
libvimg_demand.so and of libvimg_hip.so, every argument error of vimg_demand_mask with its whole sentence and the pinned
order of two faults at once, and the numpy restatement of its contract (tests/demand_ref.py) pinned on its own against
infill.lattice_mask and against tests/wtemporal_ref.py, whose carried lengths it must give."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import demand_ref as R
import temporal_ref as T
import wtemporal_ref as WT
from abi_layout import c_layout, ctypes_layout
from vimg_amd import abi
from vimg_amd import demand as dm      # the binding under test: without it nothing here says anything

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # VIMG_E_INVALID
F = np.float32
EXPORTS = ["vimg_demand_defaults", "vimg_demand_last_error", "vimg_demand_mask"]


def _defaults():
    p = abi.DemandParams()
    abi.demand_lib().vimg_demand_defaults(C.byref(p))
    return p


def _exports(name):
    lib = os.path.join(ROOT, "v-img_amd", "lib", f"libvimg_{name}.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    return nm, sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("vimg_"))


# ---- 1. header and ctypes ------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_structs(tmp_path):
    structs = {"VimgDemandFrames": abi.DemandFrames, "VimgDemandParams": abi.DemandParams}
    got = c_layout(tmp_path, ["vimg_demand.h"], structs,
                   'printf("codes %d %d\\n", VIMG_OK, VIMG_E_INVALID);'
                   'printf("limits %u %u %u %u\\n", VIMG_DEMAND_MAX_EXTENT, VIMG_DEMAND_HISTORY_PER_PIXEL, VIMG_DEMAND_MAX_STRIDE,'
                   ' VIMG_DEMAND_COUNTS);')
    assert got.pop("codes 0") == str(INVALID)
    assert got.pop("limits 32768 48 4") == str(abi.DEMAND_COUNTS)
    assert (abi.TEMPORAL_HISTORY_PER_PIXEL, abi.DEMAND_MAX_STRIDE, abi.DEMAND_COUNTS) == (48, 4, 4) and R.COUNTS == dm.COUNTS and len(dm.COUNTS) == 4
    assert got == ctypes_layout(structs)
    assert C.sizeof(abi.DemandFrames) == 40 and C.sizeof(abi.DemandParams) == 28
    assert abi.DemandFrames().struct_size == 40 and abi.DemandParams().struct_size == 28
    assert [(f, getattr(abi.DemandFrames, f).offset) for f, _ in abi.DemandFrames._fields_] == \
        [("struct_size", 0), ("width", 4), ("height", 8), ("reserved", 12), ("normal", 16), ("position", 24), ("depth", 32)]
    assert [(f, getattr(abi.DemandParams, f).offset) for f, _ in abi.DemandParams._fields_] == \
        [("struct_size", 0), ("stride", 4), ("phase", 8), ("reserved", 12), ("min_history", 16), ("sigma_normal", 20), ("sigma_plane", 24)]


def test_the_defaults_are_the_headers_and_valid():
    p = _defaults()
    assert p.struct_size == C.sizeof(abi.DemandParams) and p.reserved == 0
    got = {k: getattr(p, k) for k, _ in abi.DemandParams._fields_ if k not in ("struct_size", "reserved")}
    assert got == {k: (v if isinstance(v, int) else float(F(v))) for k, v in R.DEFAULTS.items()}
    assert (p.stride, p.phase, p.min_history) == (2, 0, 1.0)
    # the sigmas are the accumulating libraries' own defaults
    w = abi.WTemporalParams()
    abi.wtemporal_lib().vimg_wtemporal_defaults(C.byref(w))
    assert (p.sigma_normal, p.sigma_plane) == (w.sigma_normal, w.sigma_plane)
    # ... and pass the call's own checks: with them the call gets as far as the device
    import torch
    if not torch.cuda.is_available():
        rc, msg = _call(**_good_call())
        assert rc == -2 and "launch failed" in msg, (rc, msg)          # VIMG_E_DEVICE, no silent success


def test_the_library_exports_the_three_declared_names_and_libvimg_hip_gains_nothing():
    assert sorted(abi.DEMAND_SYMBOLS) == EXPORTS
    assert "demand" not in abi._LIBRARIES and "demand" in abi._LATER_LIBRARIES
    assert not set(abi._LIBRARIES) & set(abi._LATER_LIBRARIES)
    lib = abi.demand_lib()
    assert lib is abi.demand_lib() and callable(lib.vimg_demand_mask)
    nm, have = _exports("demand")
    assert have == EXPORTS
    assert any("demand_mask_kernel" in l for l in nm.splitlines())
    # the shared host skeleton (frames/frame_lib.h, frames/reproject.h) is internal: no error slot and no helper of it is
    # a dynamic symbol
    assert not [l for l in nm.splitlines() if any(w in l for w in ("g_error", "vimg_frames", "4fail", "last_errorEv", "check_", "overlaps"))]
    header = open(os.path.join(ROOT, "include", "vimg_demand.h")).read()
    for name in abi.DEMAND_SYMBOLS:
        assert name + "(" in header
    # libvimg_hip.so exports its golden list, and no library shares a name with this one
    hip = open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read().split()
    assert _exports("hip")[1] == sorted(hip) and "demand" not in " ".join(hip)
    for table in (abi.HIP_SYMBOLS, abi.HIP_TEST_SYMBOLS, abi.HOST_SYMBOLS, abi.EXPOSURE_SYMBOLS, abi.WTEMPORAL_SYMBOLS, abi.TEMPORAL_SYMBOLS,
                  abi.INFILL_SYMBOLS):
        assert not set(abi.DEMAND_SYMBOLS) & set(table)
    # it links the HIP runtime and none of the project's libraries
    path = os.path.join(ROOT, "v-img_amd", "lib", "libvimg_demand.so")
    needed = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libvimg" not in needed.replace("libvimg_demand", "")


def test_the_module_and_the_source_directory_of_the_same_name_do_not_collide():
    assert dm.__file__.endswith("demand.py") and callable(dm.mask) and callable(dm.params) and callable(dm.read)
    assert not [f for f in os.listdir(os.path.join(abi.PKG_DIR, "demand")) if f.endswith(".py")]
    # the reprojection stays ONE definition: the unit includes frames/reproject.h and projects nothing itself
    unit = open(os.path.join(abi.PKG_DIR, "demand", "demand.hip")).read()
    assert '#include "../frames/reproject.h"' in unit and '#include "../frames/frame_lib.h"' in unit
    assert "floorf" not in unit and "hw" not in unit and "(reproject(w, h, prev, " in unit


def test_params_takes_two_integer_fields_and_refuses_what_does_not_fit():
    d, p = _defaults(), dm.params()
    assert all(getattr(p, k) == getattr(d, k) for k, _ in abi.DemandParams._fields_)
    p = dm.params(stride=3, phase=8, min_history=0.5, sigma_plane=0.001)
    assert (p.stride, p.phase, p.min_history, p.sigma_plane, p.sigma_normal) == (3, 8, 0.5, float(F(0.001)), d.sigma_normal)
    for kw, sentence in ((dict(stride=-1), "demand: stride must be 0 or 2..4, not -1"),
                         (dict(phase=2 ** 32), "demand: phase must be 0..stride^2 - 1, not 4294967296")):
        with pytest.raises(ValueError) as e:
            dm.params(**kw)
        assert str(e.value) == sentence
    with pytest.raises(TypeError, match=r"demand: unknown parameters \['max_history'\]"):
        dm.params(max_history=4.0)


def test_the_preview_refuses_a_demand_it_cannot_use():
    from vimg_amd import preview
    assert preview.demand_kw(None, "x") is None and preview.demand_kw(False, "x") is None
    assert preview.demand_kw(True, "x") == {} and preview.demand_kw(dict(min_history=2), "x") == dict(min_history=2)
    with pytest.raises(ValueError, match="preview: demand must be None, a bool or a dict"):
        preview.demand_kw(3, "preview")
    with pytest.raises(TypeError, match=r"demand: unknown parameters \['stride'\]"):
        preview.demand_kw(dict(stride=3), "preview")
    import inspect
    from vimg_amd import hip
    for fn in (preview.TemporalPreview.__init__, hip.DeviceScene.temporal_preview):
        assert inspect.signature(fn).parameters["demand"].default is None


# ---- 2. argument errors, found before anything is enqueued -------------------------------------------------------
W, H = 8, 4
N = W * H
FRAME, HIST, MASK, LENGTH, COUNTS = 12 * N, 48 * N, N, 4 * N, 16
NORMAL, POSITION, DEPTH, PREV, OUT_MASK, OUT_LENGTH, OUT_COUNTS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x7000


def _good_call():
    """Arguments vimg_demand_mask accepts up to the device (the pointers are never read on the host)."""
    frames = abi.DemandFrames(width=W, height=H, normal=NORMAL, position=POSITION, depth=DEPTH)
    return dict(frames=frames, params=_defaults(), prev=PREV, matrix=T.IDENTITY.copy(), mask=OUT_MASK, length=OUT_LENGTH, counts=OUT_COUNTS)


def _call(frames, params, prev, matrix, mask, length, counts):
    lib = abi.demand_lib()
    m = None if matrix is None else (abi.f32 * 12)(*np.asarray(matrix, F).tolist())
    rc = lib.vimg_demand_mask(None if frames is None else C.byref(frames), C.c_void_p(prev), m, None if params is None else C.byref(params),
                              C.c_void_p(mask), C.c_void_p(length), C.c_void_p(counts), None)
    return rc, lib.vimg_demand_last_error().decode()


def _edit(**kw):
    a = _good_call()
    for k, v in kw.items():
        if k.startswith("m") and k[1:].isdigit():
            a["matrix"][int(k[1:])] = v
        elif k in a:
            a[k] = v
        elif k in dict(abi.DemandFrames._fields_):
            setattr(a["frames"], k, v)
        else:
            setattr(a["params"], k, v)
    return a


NAN, INF = float("nan"), float("inf")
ERRORS = [
    (dict(frames=None), "null frames"), (dict(params=None), "null params"),
    (dict(struct_size=39), "frames.struct_size 39 is below the struct's 40"),
    (dict(width=0), "width and height must be 1..32768, not 0 x 4"), (dict(height=0), "width and height must be 1..32768, not 8 x 0"),
    (dict(width=32769), "width and height must be 1..32768, not 32769 x 4"),
    (dict(height=32769), "width and height must be 1..32768, not 8 x 32769"),
    (dict(normal=None), "null normal frame"), (dict(position=None), "null position frame"), (dict(depth=None), "null depth frame"),
    (dict(mask=None), "null mask"),
    (dict(stride=1), "stride must be 0 or 2..4, not 1"), (dict(stride=5), "stride must be 0 or 2..4, not 5"),
    (dict(phase=4), "phase must be 0..3 at stride 2, not 4"), (dict(stride=3, phase=9), "phase must be 0..8 at stride 3, not 9"),
    (dict(stride=4, phase=16), "phase must be 0..15 at stride 4, not 16"), (dict(stride=0, phase=1), "phase must be 0 at stride 0, not 1"),
    (dict(min_history=-0.5), "min_history must be >= 0 and finite, not -0.5"), (dict(min_history=NAN), "min_history must be >= 0 and finite, not nan"),
    (dict(min_history=INF), "min_history must be >= 0 and finite, not inf"),
    (dict(sigma_normal=0.0), "sigma_normal must be > 0 and finite, not 0"), (dict(sigma_normal=-1.0), "sigma_normal must be > 0 and finite, not -1"),
    (dict(sigma_normal=NAN), "sigma_normal must be > 0 and finite, not nan"), (dict(sigma_normal=INF), "sigma_normal must be > 0 and finite, not inf"),
    (dict(sigma_plane=0.0), "sigma_plane must be > 0 and finite, not 0"), (dict(sigma_plane=NAN), "sigma_plane must be > 0 and finite, not nan"),
    (dict(sigma_plane=INF), "sigma_plane must be > 0 and finite, not inf"),
    (dict(prev=PREV + 8), "the previous history must be 16-byte aligned"), (dict(prev=PREV + 4), "the previous history must be 16-byte aligned"),
    (dict(matrix=None), "a previous history needs its world-to-pixel matrix"),
    (dict(m0=NAN), "world-to-pixel entry 0 is not finite (nan)"), (dict(m11=INF), "world-to-pixel entry 11 is not finite (inf)"),
    (dict(m5=-INF), "world-to-pixel entry 5 is not finite (-inf)"), (dict(prev=None, m7=NAN), "world-to-pixel entry 7 is not finite (nan)"),
    (dict(length=OUT_LENGTH + 2), "the output lengths must be 4-byte aligned"), (dict(counts=OUT_COUNTS + 1), "the output counts must be 4-byte aligned"),
    # each forbidden overlap: the last byte of one buffer on the first of the other, and the other way round
    (dict(mask=PREV + HIST - 1), "the mask overlaps the previous history"), (dict(mask=PREV - MASK + 1), "the mask overlaps the previous history"),
    (dict(mask=NORMAL + FRAME - 1), "the mask overlaps the normal frame"), (dict(mask=NORMAL - MASK + 1), "the mask overlaps the normal frame"),
    (dict(mask=POSITION), "the mask overlaps the position frame"), (dict(mask=DEPTH + FRAME - 1), "the mask overlaps the depth frame"),
    (dict(length=PREV + HIST - 4), "the output lengths overlap the previous history"),
    (dict(length=PREV - LENGTH + 4), "the output lengths overlap the previous history"),
    (dict(length=NORMAL), "the output lengths overlap the normal frame"), (dict(length=POSITION + FRAME - 4), "the output lengths overlap the position frame"),
    (dict(length=DEPTH - LENGTH + 4), "the output lengths overlap the depth frame"),
    (dict(length=OUT_MASK + MASK - 4), "the output lengths overlap the mask"), (dict(length=OUT_MASK - LENGTH + 4), "the output lengths overlap the mask"),
    (dict(counts=PREV + HIST - 4), "the output counts overlap the previous history"), (dict(counts=NORMAL - COUNTS + 4), "the output counts overlap the normal frame"),
    (dict(counts=POSITION + 8), "the output counts overlap the position frame"), (dict(counts=DEPTH + FRAME - 4), "the output counts overlap the depth frame"),
    (dict(counts=OUT_MASK + MASK - 4), "the output counts overlap the mask"), (dict(counts=OUT_MASK - COUNTS + 4), "the output counts overlap the mask"),
    (dict(counts=OUT_LENGTH + LENGTH - 4), "the output counts overlap the output lengths"),
    (dict(counts=OUT_LENGTH - COUNTS + 4), "the output counts overlap the output lengths"),
]


@pytest.mark.parametrize("edit,sentence", ERRORS, ids=[f"{'-'.join(e)}-{i}" for i, (e, _) in enumerate(ERRORS)])
def test_argument_errors_are_invalid_with_their_sentence_and_need_no_device(edit, sentence):
    rc, msg = _call(**_edit(**edit))
    assert rc == INVALID and msg == "demand: " + sentence, (rc, msg)


def test_the_checks_come_in_the_headers_order():
    """Two faults at once: the one that comes first in the header's list - the structs, the extent, the guide frames, the
    mask, stride, phase, min_history, the sigmas, the history's alignment, its matrix, the matrix entries, the alignment of
    the lengths and of the counts, then the overlaps of the mask, the lengths and the counts - is reported."""
    order = [dict(struct_size=39), dict(width=0), dict(depth=None), dict(mask=None), dict(stride=5), dict(phase=4), dict(min_history=NAN),
             dict(sigma_normal=NAN), dict(sigma_plane=NAN), dict(prev=PREV + 8), dict(m3=NAN), dict(length=OUT_LENGTH + 2),
             dict(counts=OUT_COUNTS + 2), dict(mask=DEPTH), dict(length=NORMAL), dict(counts=OUT_MASK)]
    sentences = ["frames.struct_size", "width and height", "null depth frame", "null mask", "stride must be", "phase must be", "min_history must be",
                 "sigma_normal must be", "sigma_plane must be", "previous history must be 16-byte", "entry 3 is not finite", "lengths must be 4-byte",
                 "counts must be 4-byte", "the mask overlaps the depth frame", "the output lengths overlap the normal frame"]
    assert len(order) == len(sentences) + 1
    for i in range(len(order) - 1):
        for later in order[i + 1:]:
            if set(order[i]) & set(later):
                continue              # (the same argument cannot carry two faults)
            rc, msg = _call(**_edit(**order[i], **later))
            assert rc == INVALID and sentences[i] in msg, (i, later, msg)
    # within a stage: frames before params, the frames' size before the params', normal before position before depth,
    # the missing matrix before a bad entry cannot meet, the lowest bad entry first, the history before the guides and
    # those before an earlier output
    rc, msg = _call(**_edit(frames=None, params=None))
    assert "null frames" in msg
    a = _edit(struct_size=39)
    a["params"].struct_size = 27
    assert "frames.struct_size" in _call(**a)[1]
    assert "null normal frame" in _call(**_edit(normal=None, position=None, depth=None))[1]
    assert "null position frame" in _call(**_edit(position=None, depth=None))[1]
    assert "needs its world-to-pixel matrix" in _call(**_edit(matrix=None, length=OUT_LENGTH + 2))[1]
    assert "entry 2 is not finite" in _call(**_edit(m9=NAN, m2=INF))[1]
    rc, msg = _call(**_edit(prev=NORMAL - HIST + 16, mask=NORMAL))          # the history's last 16 bytes and the normal frame's first
    assert rc == INVALID and "the mask overlaps the previous history" in msg
    rc, msg = _call(**_edit(position=NORMAL, length=NORMAL))
    assert rc == INVALID and "overlap the normal frame" in msg
    rc, msg = _call(**_edit(mask=OUT_LENGTH, counts=OUT_LENGTH))            # mask against lengths is the LENGTHS' fault, found before the counts'
    assert rc == INVALID and msg == "demand: the output lengths overlap the mask"


def test_params_struct_size_and_what_may_be_null_or_touch():
    a = _good_call()
    a["params"].struct_size = 27
    rc, msg = _call(**a)
    assert rc == INVALID and msg == "demand: params.struct_size 27 is below the struct's 28"
    # the history, its matrix, the lengths and the counts may be NULL, buffers may touch end to start, the guides may be
    # one buffer (they are only read), and the ends of every range are inside it: the call passes every argument check
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(prev=None), dict(prev=None, matrix=None), dict(length=None), dict(counts=None), dict(length=None, counts=None),
                   dict(mask=PREV + HIST), dict(mask=PREV - MASK), dict(length=OUT_MASK + MASK), dict(counts=OUT_LENGTH + LENGTH),
                   dict(counts=OUT_LENGTH - COUNTS), dict(position=NORMAL, depth=NORMAL), dict(stride=0), dict(stride=4, phase=15),
                   dict(stride=3, phase=8), dict(min_history=0.0), dict(min_history=3e38), dict(prev=None, mask=PREV)):
            rc, msg = _call(**_edit(**ok))
            assert rc == -2 and "launch failed" in msg, (ok, rc, msg)


# ---- 3. the restatement, pinned on its own: tests/temporal_ref.py's synthetic sequence, refs only ---------------------
SIGMAS = dict(sigma_normal=0.1, sigma_plane=0.00005)
GUIDES = dm.FRAMES          # ("normal", "position", "depth"): the call's own order


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module", params=[1, 2, 3])
def sequence(request):
    """(frames, histories): histories[i] is the weighted accumulation of frames 0..i with a sparse lattice's weights - real
    samples, fills worth 1/16 and pixels worth nothing - so its lengths spread around 1."""
    frames = T.synthetic_sequence(16, 32, frames=4, seed=request.param)
    rng = np.random.default_rng(100 + request.param)
    histories, prev = [], None
    for i, f in enumerate(frames):
        weight = rng.choice(np.array([0, 0.0625, 1], F), size=(16, 32), p=(0.25, 0.5, 0.25))
        prev = WT.accumulate(f["color"], f["normal"], f["position"], f["depth"], weight, prev, frames[i - 1]["matrix"] if i else None,
                             max_history=32, **SIGMAS)[0]
        histories.append(prev)
    return frames, histories


def test_min_history_0_is_the_lattice_masks_bytes(sequence):
    from vimg_amd import infill
    frames, histories = sequence
    g = [frames[3][k] for k in GUIDES]
    for stride in (2, 3, 4):
        for phase in range(stride * stride):
            m, L, counts = R.mask(*g, histories[2], frames[2]["matrix"], stride=stride, phase=phase, min_history=0.0, **SIGMAS)
            want = infill.lattice_mask(16, 32, stride, phase, device="cpu").numpy()
            assert m.dtype == want.dtype == np.uint8 and np.array_equal(m, want)
            assert R.cell(stride, phase) == infill.lattice_cell(stride, phase)
            assert R.read(counts) == dict(masked=int(want.sum()), needed=0, extra=0, live=int(frames[3]["hit"].sum()))
    # stride 0 and nothing needed: nothing masked
    assert not R.mask(*g, histories[2], frames[2]["matrix"], stride=0, min_history=0.0, **SIGMAS)[0].any()


def test_no_history_is_the_lattice_and_every_live_pixel(sequence):
    frames, _ = sequence
    f = frames[1]
    g = [f[k] for k in GUIDES]
    assert f["hit"].any() and not f["hit"].all()
    for stride, phase in ((0, 0), (2, 3), (3, 4), (4, 15)):
        m, L, counts = R.mask(*g, stride=stride, phase=phase, **SIGMAS)
        lat = R.lattice(16, 32, stride, phase)
        assert np.array_equal(m.astype(bool), lat | f["hit"]) and not L.any()
        assert R.read(counts) == dict(masked=int((lat | f["hit"]).sum()), needed=int(f["hit"].sum()), extra=int((f["hit"] & ~lat).sum()),
                                      live=int(f["hit"].sum()))


@pytest.mark.parametrize("min_history", [0.5, 1.0, 2.0])
def test_the_length_is_what_wtemporal_carries_at_weight_0_and_the_needed_set_follows(sequence, min_history):
    """Weight 0 everywhere and a max_history above every length: wtemporal's plane-A length is the reprojected length
    where it carries (code 3) and 0 where it shows without carrying (code 4) or the pixel is dead - the header's L, bit for
    bit.  Needed = its code-4 pixels and its carried lengths below min_history."""
    frames, histories = sequence
    seen = set()
    for i in (1, 2, 3):
        f = frames[i]
        g = [f[k] for k in GUIDES]
        nxt, code = WT.accumulate(f["color"], *g, np.zeros((16, 32), F), histories[i - 1], frames[i - 1]["matrix"], max_history=3e38, **SIGMAS)
        m, L, counts = R.mask(*g, histories[i - 1], frames[i - 1]["matrix"], stride=0, min_history=min_history, **SIGMAS)
        assert np.array_equal(_bits(L), _bits(nxt[0, ..., 3]))
        assert set(np.unique(code)) <= {WT.DEAD, WT.CARRIED, WT.SHOWN}
        need = (code == WT.SHOWN) | ((code == WT.CARRIED) & (nxt[0, ..., 3] < F(min_history)))
        assert np.array_equal(m.astype(bool), need)
        assert R.read(counts) == dict(masked=int(need.sum()), needed=int(need.sum()), extra=int(need.sum()), live=int((code != WT.DEAD).sum()))
        seen |= set(np.unique(code).tolist())
        # and with a lattice the mask is the union
        m2 = R.mask(*g, histories[i - 1], frames[i - 1]["matrix"], stride=3, phase=5, min_history=min_history, **SIGMAS)[0]
        assert np.array_equal(m2.astype(bool), need | R.lattice(16, 32, 3, 5))
    assert seen == {WT.DEAD, WT.CARRIED, WT.SHOWN}           # the sequence disoccludes: all three occur


def test_the_planted_frame_has_every_case():
    cur, prev, matrix = R.planted(67, 130, seed=1)
    m, L, counts = R.mask(cur["normal"], cur["position"], cur["depth"], prev, matrix, stride=3, phase=4, **SIGMAS)
    c = R.read(counts)
    assert 0 < c["extra"] < c["needed"] < c["masked"] < c["live"] < 67 * 130
    assert np.isfinite(L[np.isfinite(L)]).all() and (L >= 0).all() and (L > 1).any() and ((L > 0) & (L < 1)).any()
    assert np.isinf(L).sum() >= 1                            # the planted infinite length is carried as it is
