"""The history clamp on the GPU (libvimg_rectify.so, include/vimg_rectify.h): vimg_rectify_clamp against
the numpy restatement of its contract (tests/rectify_ref.py) BIT FOR BIT - plane A in place, the colour frame and the
codes - at the sizes where the tile and apron arithmetic can go wrong; then DeviceScene.temporal_preview(rectify=...):
with k = inf it is the plain preview bit for bit, a frame is the composition of the public pieces, after an edit of the
light the preview is nearer the relit scene than without it, on the orbit without an edit it costs no more than the
measured margin, and what it refuses."""
import numpy as np
import pytest

import rectify_ref as R
import scenes
from test_antilag import dim_the_light
from test_temporal import RES, STEPS, orbit_camera, rse

F = np.float32
# every parameter explicit: the bit-level tests do not depend on the library's defaults.  sigma_normal 0.15: the two walls
# of rectify_ref.synthetic_histories (1 - n.n = 0.2) are two surfaces; sigma_plane 0.05: their relief decides near 1
EXPLICIT = dict(k=1.5, cut=0.75, sigma_normal=0.15, sigma_plane=0.05, albedo_floor=0.02)
# e_rectify / e_plain on the orbit without an edit, as tools/rectify_sweep.py measured it for the shipped defaults on
# cornell_box_spheres 64 x 64, and 2 % of it on top
NO_EDIT_RATIO = 0.013672738 / 0.014285087          # e_rectify / e_plain = 0.9571
NO_EDIT_BOUND = NO_EDIT_RATIO * 1.02
AFTER = 8


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ibits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F, what
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


@pytest.fixture(scope="module")
def gpu():
    from vimg_amd import hip, rectify
    hip.init(0)
    return rectify


SIZES = [(1, 1), (5, 3), (64, 4), (67, 45), (130, 67)]
TOO_SMALL = {(1, 1), (5, 3)}      # for twenty clamped pixels, or for all four codes


@pytest.fixture(scope="module")
def synthetic():
    """(w, h, planes) -> rectify_ref.synthetic_histories of that picture, made once."""
    made = {}

    def get(w, h, planes):
        if (w, h, planes) not in made:
            made[w, h, planes] = R.synthetic_histories(h, w, planes=planes)
        return made[w, h, planes]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_every_radius_is_the_restatement_bit_for_bit(gpu, synthetic, radius, size):
    """1 x 1 is a tile that is all apron, 5 x 3 is narrower than the window of radius 3, 64 x 4 is one whole workgroup
    with no partial one, 67 x 45 and 130 x 67 are no multiples of the 64 x 4 tile, and 130 x 67 has three workgroups
    across.  Two walls that meet at an edge, misses, pixels without a slow or a fast history, a NaN and an inf fast colour, a NaN slow colour, an albedo below the floor; with and without the albedo
    frame, and with a moments.History as ``slow``, whose fourth plane stays what it was."""
    import torch
    from vimg_amd import moments, temporal
    w, h = size
    seen = set()
    for planes, use_albedo in ((3, True), (3, False), (4, True)):
        slow, fast, albedo = synthetic(w, h, planes)
        p = dict(EXPLICIT, radius=radius, min_taps=min(4 + radius, (2 * radius + 1) ** 2))
        want_plane, want_rgb, want_code = R.clamp(slow, fast, albedo if use_albedo else None, **p)
        hist = (moments.History if planes == 4 else temporal.History)(torch.from_numpy(slow).cuda())
        fast_d, albedo_d = temporal.History(torch.from_numpy(fast).cuda()), torch.from_numpy(albedo).cuda()
        out, code = torch.full((h, w, 3), -3.0, device="cuda"), torch.full((h, w), 9, dtype=torch.uint8, device="cuda")
        got, rgb, rc = gpu.clamp(hist, fast_d, albedo=albedo_d if use_albedo else None, out=out, code=code, **p)
        assert got is hist and rgb is out and rc is code
        what = (planes, use_albedo)
        assert np.array_equal(code.cpu().numpy(), want_code), (what, np.argwhere(code.cpu().numpy() != want_code)[:4].tolist())
        _same(hist.tensor[0].cpu().numpy(), want_plane, what)
        _same(out.cpu().numpy(), want_rgb, what)
        # every other byte of the two histories and the albedo frame is what it was
        assert np.array_equal(_bits(hist.tensor[1:].cpu().numpy()), _bits(slow[1:])), what
        assert np.array_equal(_bits(fast_d.tensor.cpu().numpy()), _bits(fast)) and np.array_equal(_bits(albedo_d.cpu().numpy()), _bits(albedo))
        seen |= set(np.unique(want_code).tolist())
        if (w, h) not in TOO_SMALL:
            assert (want_code == 1).sum() >= 20 and not np.array_equal(_bits(want_plane), _bits(slow[0]))
    assert seen == {0, 1, 2, 3} or (w, h) in TOO_SMALL, seen


@pytest.mark.gpu
def test_no_outputs_a_new_code_frame_numpy_histories_a_callers_stream_the_defaults_and_what_is_refused(gpu, synthetic):
    import torch
    from vimg_amd import hip, temporal
    slow, fast, albedo = synthetic(67, 45, 3)
    h, w = 45, 67
    p = dict(EXPLICIT, radius=2, min_taps=5)
    want_plane, want_rgb, want_code = R.clamp(slow, fast, albedo, **p)
    dev = lambda: (temporal.History(torch.from_numpy(slow).cuda()), temporal.History(torch.from_numpy(fast).cuda()))
    # neither output
    s, f = dev()
    got, rgb, code = gpu.clamp(s, f, albedo=torch.from_numpy(albedo).cuda(), out=False, **p)
    assert got is s and rgb is None and code is None
    _same(s.tensor[0].cpu().numpy(), want_plane, "no outputs")
    # outputs of the call's own
    s, f = dev()
    got, rgb, code = gpu.clamp(s, f, albedo=torch.from_numpy(albedo).cuda(), code=True, **p)
    _same(rgb.cpu().numpy(), want_rgb, "own outputs")
    assert code.dtype == torch.uint8 and np.array_equal(code.cpu().numpy(), want_code)
    # numpy in, numpy out: a new history of the class, the argument untouched
    before = slow.copy()
    got, rgb, code = gpu.clamp(temporal.History(slow), temporal.History(fast), albedo=albedo, code=True, **p)
    assert isinstance(got, temporal.History) and isinstance(got.tensor, np.ndarray) and isinstance(rgb, np.ndarray)
    _same(got.tensor[0], want_plane, "numpy")
    _same(rgb, want_rgb, "numpy")
    assert np.array_equal(code, want_code) and np.array_equal(_bits(slow), _bits(before))
    # a stream of the caller's
    s, f = dev()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got, rgb, code = gpu.clamp(s, f, albedo=torch.from_numpy(albedo).cuda(), code=True, stream=side, **p)
    side.synchronize()
    _same(s.tensor[0].cpu().numpy(), want_plane, "side stream")
    assert np.array_equal(code.cpu().numpy(), want_code)
    # the library's defaults are what the header names
    d = gpu.params()
    want_plane, want_rgb, want_code = R.clamp(slow, fast, albedo, **{k: getattr(d, k) for k, _ in type(d)._fields_
                                                                     if k not in ("struct_size", "reserved")})
    s, f = dev()
    got, rgb, code = gpu.clamp(s, f, albedo=torch.from_numpy(albedo).cuda(), code=True)
    _same(s.tensor[0].cpu().numpy(), want_plane, "defaults")
    assert np.array_equal(code.cpu().numpy(), want_code)
    # what the binding and the library refuse
    s, f = dev()
    with pytest.raises(ValueError, match="rectify: fast must be a temporal.History or a moments.History"):
        gpu.clamp(s, f.tensor, **p)
    with pytest.raises(ValueError, match="rectify fast"):
        gpu.clamp(s, temporal.History(f.tensor[:, :5].contiguous()), **p)
    with pytest.raises(ValueError, match="rectify: the two histories must both hold"):
        gpu.clamp(s, temporal.History(fast), **p)
    with pytest.raises(hip.HipError, match="radius must be 1..3, not 4"):
        gpu.clamp(s, f, **dict(p, radius=4))
    with pytest.raises(hip.HipError, match="min_taps must be 1..25, not 26"):
        gpu.clamp(s, f, **dict(p, min_taps=26))
    with pytest.raises(hip.HipError, match="the slow history overlaps the fast history"):
        gpu.clamp(s, s, **p)
    with pytest.raises(hip.HipError, match="the output overlaps the fast history"):
        gpu.clamp(s, f, out=f.tensor.view(-1)[: h * w * 3].view(h, w, 3), **p)


# ---- rendered frames ------------------------------------------------------------------------------------------------
def _scene():
    from vimg_amd import hip
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    return s, hip.DeviceScene(s), s.default_params(integrator="mis", samples=4)


def _states_equal(a, b):
    import torch
    return all(torch.equal(_ibits(a[n]), _ibits(b[n])) for n in ("sum", "count", "batches", "m2"))


@pytest.mark.gpu
def test_with_k_infinite_the_preview_is_the_plain_preview_bit_for_bit(gpu):
    """Four orbit steps and one standing frame: every frame(), the history and the accumulator."""
    import torch
    s, dev, p = _scene()
    plain, rect = dev.temporal_preview(p, samples=4, denoise=False), dev.temporal_preview(p, samples=4, denoise=False, rectify=dict(k=float("inf")))
    assert plain.rectify is None and plain.last_rectify_code is None and rect.rectify == dict(k=float("inf"))
    cams = (0, 1, 2, 3, 3)
    for step, cam in enumerate(cams):
        if step == 0 or cam != cams[step - 1]:
            dev.set_camera(*orbit_camera(cam))
        a, b = plain.frame(), rect.frame()
        assert torch.equal(_ibits(a), _ibits(b)), step
        assert torch.equal(_ibits(plain.history.tensor), _ibits(rect.history.tensor)), step
        assert _states_equal(plain.acc.state(), rect.acc.state()), step
        code = rect.last_rectify_code
        assert code.shape == (RES, RES) and not (code == 1).any() and (code == 0).any()
    for x in (plain, rect):
        x.close()
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variance_guided", [False, True])
def test_a_frame_with_rectify_is_the_public_pieces_called_by_hand(gpu, variance_guided):
    """A first frame, a camera move, a standing frame, another move: every frame's picture, slow and fast history and codes
    are acc.render + temporal.accumulate or moments.accumulate (slow, no picture) + temporal.accumulate (fast, max_history
    = fast_history) + rectify.clamp (+ the variance-guided filter) called by hand, bit for bit; the accumulator is a
    plain Progressive's."""
    import torch
    from vimg_amd import moments, preview as pv, temporal, varfilter
    s, dev, p = _scene()
    kw = dict(fast_history=3, radius=1, k=1.0, cut=1.0)
    preview = dev.temporal_preview(p, samples=4, denoise=variance_guided, variance_guided=variance_guided, rectify=kw)
    assert preview.fast_history == 3.0 and preview.rectify == dict(radius=1, k=1.0, cut=1.0)
    frozen = fast_frozen = history = fast = hand = None
    clamps = 0
    cams = (0, 1, 1, 2)
    for step, cam in enumerate(cams):
        moved = step == 0 or cam != cams[step - 1]
        if moved:
            dev.set_camera(*orbit_camera(cam))
        got = preview.frame().clone()
        now = temporal.world_to_pixel(dev.camera)
        if moved:
            g = dev.render_features(p, pv.GUIDES)
            if hand is not None:
                hand.close()
            hand, frozen, fast_frozen, k = dev.progressive(p), history, fast, 0
        mean = hand.render(4)
        k += 1
        guides = (g["normal"], g["position"], g["depth"])
        if variance_guided:
            variance = torch.empty((RES, RES), device="cuda")
            history = moments.accumulate(mean, *guides, variance=hand.variance() if k >= 2 else None, history=frozen, world_to_pixel=now,
                                         out_variance=variance, current_weight=k)
        else:
            history = temporal.accumulate(mean, *guides, history=frozen, world_to_pixel=now, current_weight=k)
        fast = temporal.accumulate(mean, *guides, history=fast_frozen, world_to_pixel=now, current_weight=k, max_history=3)
        _, out, code = gpu.clamp(history, fast, albedo=g["albedo"], code=True, radius=1, k=1.0, cut=1.0)
        clamps += int((code == 1).sum())
        if variance_guided:
            out = varfilter.atrous(out, *guides, albedo=g["albedo"], variance=variance)[0]
        assert torch.equal(_ibits(got), _ibits(out)), step
        assert torch.equal(_ibits(preview.history.tensor), _ibits(history.tensor)), step
        assert torch.equal(_ibits(preview._rectify.fast.tensor), _ibits(fast.tensor)), step
        assert torch.equal(preview.last_rectify_code, code), step
        plain = dev.progressive(p)
        for _ in range(k):
            plain.render(4, out=False)
        assert _states_equal(preview.acc.state(), plain.state()), step
        plain.close()
    assert clamps > 0
    preview.reset()
    assert preview.history is None and preview._rectify.fast is None and preview.last_rectify_code is None
    for x in (preview, hand):
        x.close()
    dev.close()


@pytest.fixture(scope="module")
def relit(gpu):
    """cornell_box_spheres 64 x 64, mis at 4 spp, no filter and no antilag: the orbit of tests/test_temporal.py walked by a
    plain preview and one with ``rectify=True``, side by side on one resident scene; after its last step the light's
    emission is quartered and eight more frames follow with the camera standing.  e against mis at 1024 spp of the
    scene as it then stands."""
    s, dev, p = _scene()
    many = s.default_params(integrator="mis", samples=1024)
    plain, rect = dev.temporal_preview(p, samples=4, denoise=False), dev.temporal_preview(p, samples=4, denoise=False, rectify=True)
    o = {}
    for i in range(STEPS + 1):
        dev.set_camera(*orbit_camera(i))
        a, b = plain.frame().cpu().numpy(), rect.frame().cpu().numpy()
    ref = dev.render(many, stats=False).cpu().numpy()
    o["orbit"] = (rse(a, ref), rse(b, ref))
    o["clamped"] = float((rect.last_rectify_code == 1).float().mean())
    dim_the_light(dev, s)
    ref = dev.render(many, stats=False).cpu().numpy()
    o["after"] = []
    for k in range(AFTER):
        a, b = plain.frame().cpu().numpy(), rect.frame().cpu().numpy()
        o["after"].append((rse(a, ref), rse(b, ref)))
    o["finite"] = bool(np.isfinite(b).all())
    for x in (plain, rect):
        x.close()
    dev.close()
    return o


@pytest.mark.gpu
def test_after_the_light_is_dimmed_the_preview_with_rectify_is_nearer_the_relit_scene(relit):
    """Frame 8 after the edit, against mis at 1024 spp of the scene as edited: e with rectify strictly below e without.
    This asserts the direction only.  Measured, frames 1..8: plain 0.26169 0.20545 0.16989 0.14336 0.12299 0.10667 0.09358
    0.08283; rectify 0.14277 0.00717 0.00586 0.00481 0.00421 0.00378 0.00349 0.00316."""
    print("e after the edit, frames 1..8: plain " + " ".join(f"{a:.5f}" for a, _ in relit["after"])
          + "; rectify " + " ".join(f"{b:.5f}" for _, b in relit["after"]))
    assert relit["finite"]
    plain8, rect8 = relit["after"][AFTER - 1]
    assert rect8 < plain8


@pytest.mark.gpu
def test_without_an_edit_rectify_costs_no_more_than_the_measured_margin(relit):
    """The last frame of the orbit without an edit: e_rectify <= e_plain * bound, e_plain from the plain preview of the
    same fixture, bound = the ratio tools/rectify_sweep.py measured for the shipped defaults on this scene (DESIGN.md
    4.33) times 1.02.  Measured: 0.01367 against 0.01429, ratio 0.9571 under the bound 0.9763; 6.96 % of the pixels were
    clamped on the last step."""
    e_plain, e_rect = relit["orbit"]
    print(f"e on the orbit without an edit: plain {e_plain:.5f}, rectify {e_rect:.5f} (ratio {e_rect / e_plain:.4f}, bound "
          f"{NO_EDIT_BOUND:.4f}); {100 * relit['clamped']:.2f} % of the pixels were clamped on the last step")
    assert e_rect <= e_plain * NO_EDIT_BOUND


@pytest.mark.gpu
def test_what_the_preview_refuses(gpu):
    s, dev, p = _scene()
    with pytest.raises(ValueError, match="temporal_preview: rectify does not go with sparse: a filled pixel's weight would have to enter "
                                         "the fast history too"):
        dev.temporal_preview(p, sparse=2, rectify=True)
    with pytest.raises(TypeError, match=r"rectify: unknown parameters \['max_history'\]"):
        dev.temporal_preview(p, rectify=dict(max_history=4))
    for bad in (0, 0.5, -2):
        with pytest.raises(ValueError, match="temporal_preview: rectify's fast_history must be >= 1 and finite"):
            dev.temporal_preview(p, rectify=dict(fast_history=bad))
    with pytest.raises(ValueError, match="temporal_preview: rectify must be None, a bool or a dict"):
        dev.temporal_preview(p, rectify=2)
    # it goes with the other options, and renders the albedo frame without the filter
    on = dev.temporal_preview(p, denoise=False, rectify=True, antilag=True, despeckle=True, exposure=True, motion=s)
    off = dev.temporal_preview(p, denoise=False)
    assert "albedo" in on._features and "albedo" not in off._features
    off.close()
    dev.set_camera(*orbit_camera(0))
    assert bool(on.frame().isfinite().all())
    dev.temporal_preview(p, sparse=2, rectify=None).close()
    on.close()
    dev.close()
