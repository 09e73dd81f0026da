"""What the two frame libraries share (v-img_amd/frames/frame_lib.h, hip._Tensors, hip.FrameCall, hip.GuideCache;
DESIGN.md 4.20): every argument error is, code and whole sentence, what it was before the host skeleton was shared
(tests/golden/frame_lib_errors.json, recorded from the two separate units), of two faults made at once every library
reports the one it reported while its checks were its own copy (the record's "order"), each library keeps an error
slot of its own, the two frames structs open with the same eight fields, a call collects its tensors in one place, and a preview
renders its guides again after an edit of the scene and only then."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import scenes
import test_filter_abi as FA
import test_temporal_abi as TA
from abi_layout import c_layout
from vimg_amd import abi, hip

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_lib_errors.json")))
CASES = [(lib, case) for lib in ("filter", "temporal") for case in GOLDEN[lib]]


def _arguments(mod, case):
    """The arguments of the recorded case: "<edited names>-<index into the module's ERRORS>", or the params.struct_size
    case its last-message test makes."""
    if case == "params.struct_size":
        a = mod._good_call()
        a["params"].struct_size = 23
        return a
    edit = mod.ERRORS[int(case.rsplit("-", 1)[1])][0]
    assert case.rsplit("-", 1)[0] == "-".join(edit)
    return mod._edit(**edit)


# ---- a. whole sentences ---------------------------------------------------------------------------------------------
def test_the_record_holds_every_argument_error_of_both_libraries():
    for mod, lib in ((FA, "filter"), (TA, "temporal")):
        assert len(GOLDEN[lib]) == len(mod.ERRORS) + 1 and "params.struct_size" in GOLDEN[lib]
        assert all(rec["code"] == -1 for rec in GOLDEN[lib].values())       # VIMG_E_INVALID only: no device needed


@pytest.mark.parametrize("lib,case", CASES, ids=[f"{lib}:{case}" for lib, case in CASES])
def test_an_argument_error_is_the_recorded_code_and_sentence(lib, case):
    mod = {"filter": FA, "temporal": TA}[lib]
    rc, msg = mod._call(**_arguments(mod, case))
    assert {"code": rc, "message": msg} == GOLDEN[lib][case]


# ---- a'. which of two faults is reported ----------------------------------------------------------------------------
# GOLDEN["order"]: per library its "faults", single edits of the module's _good_call() listed in the order of the
# checks they trip ("nan" stands for the float), and "pairs" [i, j, code, message]: what the call said with faults i
# and j made at once, j up to three places behind i, recorded from the units before their reprojection checks
# (frames/reproject.h) and workspace checks (frame_lib.h's check_workspace) were written once.
def _order_modules():
    import test_infill_abi as IA
    import test_moments_abi as MA
    import test_varfilter_abi as VA
    import test_wtemporal_abi as WA
    return {"filter": FA, "temporal": TA, "varfilter": VA, "moments": MA, "infill": IA, "wtemporal": WA}


def _fault(edit):
    return {k: float(v) if isinstance(v, str) else v for k, v in edit.items()}


def _clash(a, b):
    """Two faults that cannot be made at once: they edit one argument (matrix and its entries m0..m11 are one)."""
    keys = lambda e: {"matrix" if k[0] == "m" and k[1:].isdigit() else k for k in e}
    return bool(keys(a) & keys(b))


ORDER = [(lib, i, j) for lib, rec in GOLDEN["order"].items() for i, j, _, _ in rec["pairs"]]


def test_the_order_record_covers_the_chains_and_the_seams():
    assert sorted(GOLDEN["order"]) == sorted(_order_modules())
    for lib, rec in GOLDEN["order"].items():
        said = " | ".join(m for _, _, _, m in rec["pairs"])
        if lib in ("filter", "varfilter", "infill"):
            want = ("null workspace", "the workspace has 1 bytes")      # (null + short, short + misaligned)
        else:
            want = ("must be 16-byte aligned", "needs its world-to-pixel matrix", "entry 3 is not finite", "overlaps the previous one",
                    "the next history overlaps the depth frame", "the output overlaps the previous history",
                    "the output overlaps the position frame")
            want += {"temporal": (), "moments": ("min_history must be", "is above max_history", "the output overlaps the variance frame",
                                                 "the output variance overlaps the previous history", "the output variance overlaps the output"),
                     "wtemporal": ("null weight frame", "the weight frame must be 4-byte aligned", "the output overlaps the weight frame",
                                   "the output codes overlap the previous history", "the output codes overlap the weight frame")}[lib]
        assert all(w in said for w in want), (lib, [w for w in want if w not in said])
        # every adjacent pair that can be made at once is in the record
        have = {(i, j) for i, j, _, _ in rec["pairs"]}
        faults = rec["faults"]
        assert all((i, i + 1) in have for i in range(len(faults) - 1) if not _clash(faults[i], faults[i + 1]))


@pytest.mark.parametrize("lib,i,j", ORDER, ids=[f"{lib}:{i}+{j}" for lib, i, j in ORDER])
def test_two_faults_at_once_report_the_recorded_one(lib, i, j):
    mod, rec = _order_modules()[lib], GOLDEN["order"][lib]
    rc, msg = mod._call(**mod._edit(**_fault(rec["faults"][i]), **_fault(rec["faults"][j])))
    assert [i, j, rc, msg] in rec["pairs"], (rec["faults"][i], rec["faults"][j], rc, msg)


# ---- b. two error slots ---------------------------------------------------------------------------------------------
def test_each_library_keeps_its_own_last_error():
    flt, tmp = abi.filter_lib(), abi.temporal_lib()
    fail_filter = lambda: FA._call(**FA._edit(iterations=99))
    fail_temporal = lambda: TA._call(**TA._edit(max_history=0.25))
    for first, second in ((fail_filter, fail_temporal), (fail_temporal, fail_filter)):
        assert first()[0] == -1 and second()[0] == -1
        assert flt.vimg_filter_last_error().decode() == "atrous: iterations must be 1..12, not 99"
        assert tmp.vimg_temporal_last_error().decode() == "temporal: max_history must be >= 1 and finite, not 0.25"
        # ... and a further failure of one leaves the other's sentence alone
        first()
        assert flt.vimg_filter_last_error().decode().startswith("atrous: iterations")
        assert tmp.vimg_temporal_last_error().decode().startswith("temporal: max_history")


# ---- c. the shared prefix -------------------------------------------------------------------------------------------
def test_the_two_frames_structs_open_with_the_same_eight_fields(tmp_path):
    """What frame_lib.h's check_head and hip.FrameCall rest on."""
    shared = ("struct_size", "width", "height", "reserved", "color", "normal", "position", "depth")
    structs = {"VimgFilterFrames": abi.FilterFrames, "VimgTemporalFrames": abi.TemporalFrames}
    got = c_layout(tmp_path, ["vimg_filter.h", "vimg_temporal.h"], structs)
    for i, f in enumerate(shared):
        assert abi.FilterFrames._fields_[i][0] == abi.TemporalFrames._fields_[i][0] == f
        assert got[f"VimgFilterFrames.{f}"] == got[f"VimgTemporalFrames.{f}"] == str(getattr(abi.FilterFrames, f).offset)
    assert [got[f"VimgFilterFrames.{f}"] for f in shared] == ["0", "4", "8", "12", "16", "24", "32", "40"]
    for t in (abi.GeometryUpdateV1, abi.GeometryUpdate, abi.RebuildOptions, abi.FilterFrames, abi.TemporalFrames):
        assert t().struct_size == C.sizeof(t) and t._fields_[0][0] == "struct_size"


# ---- d. the collector -----------------------------------------------------------------------------------------------
def test_a_call_collects_its_tensors_in_one_place(monkeypatch):
    sent = []

    def upload(a):
        sent.append(a)
        return torch.from_numpy(a)       # (stays on the host: where a tensor lands is what is tested)
    monkeypatch.setattr(hip, "_upload", upload)
    before = torch.cuda.is_initialized()
    c = hip._Tensors()
    rays = np.zeros((7, 8), np.float32)
    t = c.take(rays, "rays", ("float32",), (None, 8), aligned=True)
    assert len(sent) == 1 and c.made == [t] and c.used == [] and tuple(t.shape) == (7, 8)
    mine, theirs = torch.zeros(3), torch.zeros(4)
    assert c.own(mine) is mine and c.use(theirs) is theirs
    assert c.made == [t, mine] and c.used == [theirs]
    # a refused input raises before any upload, and lands nowhere
    for bad, word in ((np.zeros((7, 8), np.float64), "float32"), (np.zeros((7, 7), np.float32), "shape"), ([0.0] * 8, "numpy array")):
        with pytest.raises(ValueError, match=word):
            c.take(bad, "rays", ("float32",), (None, 8), aligned=True)
    # a caller's output is refused in _device_tensor's one sentence
    for out in (np.zeros((7, 4), np.float32), torch.zeros((7, 4)), torch.zeros((7, 4), dtype=torch.float64), [1.0]):
        with pytest.raises(ValueError, match=r"^trace_rays: out must be a contiguous torch.float32 CUDA tensor of shape "
                                             r"\(7, 4\) on the current device$"):
            c.output(out, "trace_rays", "float32", (7, 4), aligned=True)
    assert len(sent) == 1 and len(c.made) == 2 and len(c.used) == 1 and torch.cuda.is_initialized() == before


def test_a_frame_call_checks_the_colour_shape_first_and_numpy_in_means_numpy_out(monkeypatch):
    FrameCall = hip.FrameCall
    monkeypatch.setattr(hip, "_upload", torch.from_numpy)
    for bad in (np.zeros((4, 5), np.float32), np.zeros((4, 5, 4), np.float32), [1.0]):
        shape = tuple(bad.shape) if hasattr(bad, "shape") else None
        with pytest.raises(ValueError) as e:
            FrameCall("atrous", bad)
        assert str(e.value) == f"atrous color: shape must be (H, W, 3), not {shape}"
    f = np.zeros((4, 5, 3), np.float32)
    c = FrameCall("temporal", f)
    assert (c.h, c.w, c.to_host) == (4, 5, True)
    t = c.frames(("color", "normal", "albedo"), (f, f, None), optional=("albedo",))
    assert list(t) == ["color", "normal"] and len(c.made) == 2 and c.used == []
    with pytest.raises(ValueError, match=r"^temporal normal: shape must be \(4, 5, 3\), not \(4, 4, 3\)$"):
        c.frames(("normal",), (np.zeros((4, 4, 3), np.float32),))
    with pytest.raises(ValueError, match="^temporal normal: expected a torch CUDA tensor or a numpy array, not NoneType$"):
        c.frames(("normal",), (None,))
    assert isinstance(c.result(torch.zeros(2)), np.ndarray)
    assert not FrameCall("atrous", torch.zeros((4, 5, 3))).to_host


# ---- e. guides after an edit ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_preview_renders_its_guides_again_after_an_edit_and_only_then():
    """cornell_box_spheres 64 x 64, mis: preview(4), a new camera, reset(), preview(4) is bit for bit the filter on a
    fresh 4 spp render with freshly rendered guides (4 feature samples) under the new camera; a third preview without
    an edit renders no guides.  (tests/test_filter.py pins the same for an unedited scene and a set_camera to the
    camera the scene already had.)"""
    from vimg_amd import filter as flt
    hip.init(0)
    s = scenes.json_scene("cornell_box_spheres.json", res=(64, 64))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    calls = []
    render_features = dev.render_features
    dev.render_features = lambda *a, **kw: calls.append(a[1]) or render_features(*a, **kw)
    acc = dev.progressive(p)
    first = acc.preview(4).clone()
    assert len(calls) == 1
    dev.set_camera((300.0, 290.0, -780.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 40.0)
    acc.reset()
    second = acc.preview(4)
    assert len(calls) == 2 and calls[1] == flt.GUIDES
    g = render_features(p, flt.GUIDES)
    want = flt.atrous(dev.render(p, stats=False), g["normal"], g["position"], g["depth"], albedo=g["albedo"])
    assert torch.equal(second.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(second, first)                    # (the camera did move the picture)
    kept = acc._guides[1]
    assert all(torch.equal(kept[k].view(torch.int32), g[k].view(torch.int32)) for k in flt.GUIDES)
    third = acc.preview(4)
    assert len(calls) == 2 and acc._guides[1] is kept and acc.samples == 8
    p8 = s.default_params(integrator="mis", samples=8)
    want = flt.atrous(dev.render(p8, stats=False), g["normal"], g["position"], g["depth"], albedo=g["albedo"])
    assert torch.equal(third.view(torch.int32), want.view(torch.int32))
    acc.close()
    dev.close()
