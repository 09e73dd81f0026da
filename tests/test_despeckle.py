"""The firefly clamp on the GPU (libvimg_despeckle.so, include/vimg_despeckle.h): vimg_despeckle_clamp
against the numpy restatement of its contract (tests/despeckle_ref.py) BIT FOR BIT, colour and codes, on synthetic frames
with injected speckles and at the sizes where the tile and halo arithmetic can go wrong; then what is built on it -
``despeckle=`` on Progressive.preview, DeviceScene.render_denoised and DeviceScene.temporal_preview, each equal to its
pieces called by hand and unchanged without the argument - and its use: at 4 spp the filtered preview is nearer the
converged frame with the clamp than without, and the clamp leaves a converged frame alone."""
import math

import numpy as np
import pytest

import atrous_ref
import despeckle_ref as R
import infill_ref
import scenes

F = np.float32
# every parameter explicit: the bit-level tests do not depend on the library's defaults
EXPLICIT = dict(gain=2.5, sigma_normal=0.3, sigma_plane=0.05, albedo_floor=0.02)
GUIDES = ("normal", "position", "depth")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def _ibits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module")
def gpu():
    from vimg_amd import despeckle, hip
    hip.init(0)
    return despeckle


@pytest.fixture(scope="module")
def synthetic():
    """atrous_ref.synthetic_frame (64 x 96: a sphere over a checkered floor under a sky of misses) with speckles: 1 % of
    the live pixels times 10..1000, a NaN, a +inf and a -inf colour, a NaN normal, a NaN depth.  (host frames, device
    frames), made once."""
    import torch
    sf = atrous_ref.synthetic_frame()
    f = R.speckled(sf, sf["noisy"], sf["hit"])
    names = ("color",) + GUIDES + ("albedo",)
    return f, {k: torch.from_numpy(f[k]).cuda() for k in names}


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("rank", [1, 2, 3, 4])
def test_every_radius_and_rank_is_the_restatement_bit_for_bit(gpu, synthetic, radius, rank):
    """The speckled synthetic frame, with and without albedo, out of place and on the colour frame itself."""
    f, dev = synthetic
    seen = set()
    for use_albedo in (True, False):
        p = dict(EXPLICIT, radius=radius, rank=rank, min_taps=max(rank, 4))
        want, want_code = R.clamp(f["color"], *(f[k] for k in GUIDES), f["albedo"] if use_albedo else None, **p)
        got, code = gpu.clamp(dev["color"], *(dev[k] for k in GUIDES), albedo=dev["albedo"] if use_albedo else None, **p)
        assert np.array_equal(code.cpu().numpy(), want_code), (use_albedo, np.argwhere(code.cpu().numpy() != want_code)[:4].tolist())
        _same(got.cpu().numpy(), want)
        assert np.array_equal(_bits(dev["color"].cpu().numpy()), _bits(f["color"]))      # the frames were only read
        seen |= set(np.unique(want_code).tolist())
        color = dev["color"].clone()
        res, code = gpu.clamp(color, *(dev[k] for k in GUIDES), albedo=dev["albedo"] if use_albedo else None, out=color, **p)
        assert res is color and np.array_equal(code.cpu().numpy(), want_code)
        _same(color.cpu().numpy(), want)
        # the speckles were found, the NaN and the infinities stand where they stood
        odd = ~np.isfinite(f["color"])
        assert (want_code == 1).sum() >= 20 and np.array_equal(_bits(want[odd]), _bits(f["color"][odd]))
    assert seen == {0, 1, 2, 3}, seen


SIZES = [(w, h) for w in (1, 2, 63, 64, 65, 129) for h in (1, 3, 4, 5, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_tile_and_its_halo_at_every_edge_size(gpu, size):
    """Widths 1, 2 (narrower than a halo), 63, 64, 65 (a wave and one pixel either way), 129 (three workgroups) by
    heights 1, 3, 4, 5 (a row tile and one row either way), 9: infill_ref.creased_frames - a crease, a depth step, a
    block of misses, NaNs in the guides - with speckles, every radius, ranks in turn, with and without albedo."""
    import torch
    w, h = size
    cf = infill_ref.creased_frames(h, w)
    f = R.speckled(cf, cf["color"], cf["depth"][..., 0] > 0, share=0.03)
    dev = {k: torch.from_numpy(f[k]).cuda() for k in ("color",) + GUIDES + ("albedo",)}
    for radius in (1, 2, 3):
        for use_albedo in (True, False):
            rank = 1 + (radius + w + h + use_albedo) % 4
            p = dict(EXPLICIT, radius=radius, rank=rank, min_taps=rank)
            want, want_code = R.clamp(f["color"], *(f[k] for k in GUIDES), f["albedo"] if use_albedo else None, **p)
            got, code = gpu.clamp(dev["color"], *(dev[k] for k in GUIDES), albedo=dev["albedo"] if use_albedo else None, **p)
            assert np.array_equal(code.cpu().numpy(), want_code), (radius, use_albedo)
            _same(got.cpu().numpy(), want)
    if (w, h) == (1, 1):
        assert want_code[0, 0] == 2          # a live pixel without a tap


@pytest.mark.gpu
def test_numpy_frames_no_codes_a_callers_buffers_and_a_callers_stream(gpu, synthetic):
    import torch
    from vimg_amd import hip
    f, dev = synthetic
    h, w = f["color"].shape[:2]
    p = dict(EXPLICIT, radius=2, rank=2, min_taps=5)
    want, want_code = R.clamp(f["color"], *(f[k] for k in GUIDES), f["albedo"], **p)
    # numpy in, numpy out
    got, code = gpu.clamp(f["color"], *(f[k] for k in GUIDES), albedo=f["albedo"], **p)
    assert isinstance(got, np.ndarray) and isinstance(code, np.ndarray) and code.dtype == np.uint8
    _same(got, want)
    assert np.array_equal(code, want_code)
    # without codes
    got, code = gpu.clamp(dev["color"], *(dev[k] for k in GUIDES), albedo=dev["albedo"], out_code=False, **p)
    assert code is None
    _same(got.cpu().numpy(), want)
    # the caller's out, out_code and workspace (float32, exactly the size asked for)
    out, out_code = torch.full_like(dev["color"], -3.0), torch.full((h, w), 9, dtype=torch.uint8, device="cuda")
    work = torch.empty(gpu.workspace_bytes(w, h) // 4, dtype=torch.float32, device="cuda")
    assert work.numel() * 4 == 32 * h * w
    res, rc = gpu.clamp(dev["color"], *(dev[k] for k in GUIDES), albedo=dev["albedo"], out=out, out_code=out_code, workspace=work, **p)
    assert res is out and rc is out_code
    _same(out.cpu().numpy(), want)
    assert np.array_equal(out_code.cpu().numpy(), want_code)
    # a stream of the caller's
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got, code = gpu.clamp(dev["color"], *(dev[k] for k in GUIDES), albedo=dev["albedo"], stream=side, **p)
    side.synchronize()
    _same(got.cpu().numpy(), want)
    assert np.array_equal(code.cpu().numpy(), want_code)
    # the library's defaults are what the header names
    d = gpu.params()
    want, want_code = R.clamp(f["color"], *(f[k] for k in GUIDES), f["albedo"],
                              **{k: getattr(d, k) for k, _ in type(d)._fields_ if k != "struct_size"})
    got, code = gpu.clamp(dev["color"], *(dev[k] for k in GUIDES), albedo=dev["albedo"])
    _same(got.cpu().numpy(), want)
    assert np.array_equal(code.cpu().numpy(), want_code)
    # what the binding and the library refuse
    with pytest.raises(ValueError, match="despeckle normal"):
        gpu.clamp(dev["color"], dev["normal"][:, :5].contiguous(), dev["position"], dev["depth"], **p)
    with pytest.raises(hip.HipError, match="radius must be 1..3, not 4"):
        gpu.clamp(dev["color"], *(dev[k] for k in GUIDES), **dict(p, radius=4))
    with pytest.raises(hip.HipError, match="min_taps must be 2..24, not 25"):
        gpu.clamp(dev["color"], *(dev[k] for k in GUIDES), **dict(p, min_taps=25))
    with pytest.raises(hip.HipError, match="the workspace has"):
        gpu.clamp(dev["color"], *(dev[k] for k in GUIDES), workspace=work[:-1], **p)
    with pytest.raises(hip.HipError, match="overlaps the normal frame"):
        gpu.clamp(dev["color"], *(dev[k] for k in GUIDES), out=dev["normal"], **p)


# ---- rendered frames ------------------------------------------------------------------------------------------------
RES = 64
PIVOT = np.array([278.0, 278.0, 556.0])      # the centre of the box's back wall
EYE0 = np.array([278.0, 278.0, -800.0])


def orbit_camera(i, degrees=1.5):
    """Step i of an orbit about the back wall's centre that keeps the viewing direction: (look_from, look_at, up, vfov)."""
    a = math.radians(degrees * i)
    r = EYE0 - PIVOT
    eye = PIVOT + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])
    return eye, eye + np.array([0.0, 0.0, 800.0]), (0.0, 1.0, 0.0), 40.0


@pytest.fixture(scope="module")
def cornell(gpu):
    """cornell_box_spheres 64 x 64: (scene, resident scene, mis parameters at 4 spp, the four feature frames at 4 spp)."""
    from vimg_amd import hip
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    return s, dev, p, dev.render_features(p, gpu.GUIDES)


def _clamped(gpu, color, g, **kw):
    return gpu.clamp(color, g["normal"], g["position"], g["depth"], albedo=g["albedo"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("variance_guided", [False, True])
def test_preview_with_despeckle_is_render_clamp_and_filter_by_hand(gpu, cornell, variance_guided):
    import torch
    from vimg_amd import filter as flt, varfilter
    s, dev, p, g = cornell
    acc, hand, off, plain = (dev.progressive(p) for _ in range(4))

    def filtered(color):
        if variance_guided:
            return varfilter.atrous(color, g["normal"], g["position"], g["depth"], albedo=g["albedo"], variance=hand.variance())[0]
        return flt.atrous(color, g["normal"], g["position"], g["depth"], albedo=g["albedo"])

    got = acc.preview(4, despeckle=True, variance_guided=variance_guided)
    noisy = hand.render(4)
    clamped, code = _clamped(gpu, noisy, g)
    assert (code == 1).any() and not torch.equal(_ibits(clamped), _ibits(noisy))          # the clamp had work to do
    assert torch.equal(_ibits(got), _ibits(filtered(clamped)))
    # the accumulator was not written: it is the one that only rendered
    a, b = acc.state(), hand.state()
    assert all(torch.equal(_ibits(a[k]), _ibits(b[k])) for k in ("sum", "count", "batches", "m2"))
    # None and False: the bits the call gives without the argument
    without = plain.preview(4, variance_guided=variance_guided)
    assert torch.equal(_ibits(off.preview(4, despeckle=None, variance_guided=variance_guided)), _ibits(without))
    off.reset()
    assert torch.equal(_ibits(off.preview(4, despeckle=False, variance_guided=variance_guided)), _ibits(without))
    assert not torch.equal(_ibits(without), _ibits(got))
    # a dict: the parameters
    acc.reset()
    hand.reset()
    got = acc.preview(4, despeckle=dict(rank=1, gain=1.5), variance_guided=variance_guided)
    clamped, _ = _clamped(gpu, hand.render(4), g, rank=1, gain=1.5)
    assert torch.equal(_ibits(got), _ibits(filtered(clamped)))
    for x in (acc, hand, off, plain):
        x.close()


@pytest.mark.gpu
def test_render_denoised_with_despeckle_is_its_pieces_and_unchanged_without(gpu, cornell):
    import torch
    from vimg_amd import filter as flt
    s, dev, p, g = cornell
    got = dev.render_denoised(p, despeckle=dict(rank=2))
    clamped, code = _clamped(gpu, dev.render(p, stats=False), g, rank=2)
    assert (code == 1).any()
    assert torch.equal(_ibits(got), _ibits(flt.atrous(clamped, g["normal"], g["position"], g["depth"], albedo=g["albedo"])))
    plain = dev.render_denoised(p)
    assert torch.equal(_ibits(dev.render_denoised(p, despeckle=None)), _ibits(plain))
    assert torch.equal(_ibits(dev.render_denoised(p, despeckle=False)), _ibits(plain))
    assert not torch.equal(_ibits(got), _ibits(plain))
    with pytest.raises(ValueError, match="render_denoised: despeckle must be"):
        dev.render_denoised(p, despeckle="yes")
    with pytest.raises(TypeError, match="despeckle: unknown parameters"):
        dev.render_denoised(p, despeckle=dict(sigma_color=1.0))


@pytest.mark.gpu
@pytest.mark.parametrize("antilag", [False, True])
def test_temporal_preview_with_despeckle_is_its_pieces_over_moves_and_a_standing_frame(gpu, antilag):
    """A first frame, a camera move, a standing frame, another move, with ``despeckle=True`` and without the filter: every
    frame's picture and history are acc.render + despeckle.clamp (+ antilag.rescale on the frames that froze a history)
    + temporal.accumulate called by hand, bit for bit; the accumulator is a plain Progressive's after the standing frame
    and at the end."""
    import torch
    from vimg_amd import antilag as lag, hip, temporal
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    preview = dev.temporal_preview(p, samples=4, denoise=False, despeckle=True, antilag=antilag)
    assert preview.despeckle == {}
    frozen = history = hand = None
    clamps = 0
    for step, cam in enumerate((0, 1, 1, 2)):
        moved = step == 0 or cam != (0, 1, 1, 2)[step - 1]
        if moved:
            dev.set_camera(*orbit_camera(cam))
        got = preview.frame().clone()
        now = temporal.world_to_pixel(dev.camera)
        if moved:
            g = dev.render_features(p, gpu.GUIDES)
            if hand is not None:
                hand.close()
            hand, frozen, k = dev.progressive(p), history, 0
        mean = hand.render(4)
        mean, code = _clamped(gpu, mean, g, out=mean)
        clamps += int((code == 1).sum())
        if antilag and moved and frozen is not None:
            lag.rescale(mean, g["normal"], g["position"], g["depth"], frozen, now)
        k += 1
        out = torch.empty_like(mean)
        history = temporal.accumulate(mean, g["normal"], g["position"], g["depth"], history=frozen, world_to_pixel=now, out=out,
                                      current_weight=k)
        assert torch.equal(_ibits(got), _ibits(out)), step
        assert torch.equal(_ibits(preview.history.tensor), _ibits(history.tensor)), step
        plain = dev.progressive(p)
        for _ in range(k):
            plain.render(4, out=False)
        a, b = preview.acc.state(), plain.state()
        assert all(torch.equal(_ibits(a[n]), _ibits(b[n])) for n in ("sum", "count", "batches", "m2")), step
        plain.close()
    assert clamps > 0
    for x in (preview, hand):
        x.close()
    dev.close()


@pytest.mark.gpu
def test_temporal_preview_without_despeckle_is_unchanged_and_sparse_refuses_it(gpu):
    import torch
    from vimg_amd import hip
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    a, b, c = dev.temporal_preview(p), dev.temporal_preview(p, despeckle=None), dev.temporal_preview(p, despeckle=False)
    on = dev.temporal_preview(p, despeckle=dict(gain=3))
    assert a.despeckle is None and b.despeckle is None and on.despeckle == dict(gain=3)
    for cam, move in ((0, True), (1, True), (1, False)):
        if move:
            dev.set_camera(*orbit_camera(cam))
        fa, fb, fc, fo = (x.frame() for x in (a, b, c, on))
        assert torch.equal(_ibits(fa), _ibits(fb)) and torch.equal(_ibits(fa), _ibits(fc))
        assert torch.equal(_ibits(a.history.tensor), _ibits(b.history.tensor))
        assert not torch.equal(_ibits(fa), _ibits(fo))
    with pytest.raises(ValueError, match="temporal_preview: despeckle does not go with sparse: a lattice pixel's neighbours carry no samples"):
        dev.temporal_preview(p, sparse=2, despeckle=True)
    with pytest.raises(ValueError, match="temporal_preview: despeckle must be"):
        dev.temporal_preview(p, despeckle=2)
    with pytest.raises(TypeError, match="despeckle: unknown parameters"):
        dev.temporal_preview(p, despeckle=dict(max_history=4))
    dev.temporal_preview(p, sparse=2, despeckle=None).close()
    for x in (a, b, c, on):
        x.close()
    dev.close()


@pytest.mark.gpu
def test_the_clamped_preview_is_nearer_the_converged_frame_and_a_converged_frame_is_left_alone(gpu, cornell):
    """cornell_box_spheres 64 x 64, mis at 4 spp, against mis at 256 spp rendered here, e = mean((x - ref)^2 / (ref^2 +
    0.01)): the filtered preview with ``despeckle=True`` has a strictly lower e than without it (the CPU oracle's frames
    gave 0.034 against 0.048).  Condition: the clamp applied to the 256-spp frame itself changes at most 1 % of its live
    pixels - a clamp that rewrites a converged picture is bias, not a filter for outliers.

    Measured on the GPU at the library's defaults (radius 1, rank 3, gain 3): e 0.02082 with the clamp against 0.02135
    without; the clamp changes 0.052 % of the live pixels of the 256-spp frame and keeps 0.9956 of its luminance (with a
    gain of 2: 0.02039, 0.104 %, 0.9945)."""
    s, dev, p, g = cornell
    ref = dev.render(s.default_params(integrator="mis", samples=256), stats=False)
    plain, clamped = dev.progressive(p), dev.progressive(p)
    e_plain = R.rel_error(plain.preview(4).cpu().numpy(), ref.cpu().numpy())
    e_clamped = R.rel_error(clamped.preview(4, despeckle=True).cpu().numpy(), ref.cpu().numpy())
    out, code = _clamped(gpu, ref, g)
    code = code.cpu().numpy()
    live = code != 3
    share = (code == 1).sum() / live.sum()
    kept = R.luminance(out.cpu().numpy()).mean() / R.luminance(ref.cpu().numpy()).mean()
    print(f"e of the filtered preview at 4 spp: plain {e_plain:.5f}, clamped first {e_clamped:.5f}; the clamp changes "
          f"{100 * share:.3f} % of the live pixels of the 256-spp frame and keeps {kept:.4f} of its luminance")
    for x in (plain, clamped):
        x.close()
    assert live.sum() > 0
    assert share <= 0.01
    assert e_clamped < e_plain
