"""The anti-lag library on the GPU (libvimg_antilag.so, include/vimg_antilag.h): vimg_antilag_rescale
against the numpy restatement of its contract (tests/antilag_ref.py) BIT FOR BIT - the new lengths, the scale frame,
and every other byte of the history as it was - what the binding refuses, and DeviceScene.temporal_preview(antilag=True):
after an edit of the light the preview is nearer the relit scene than the preview without it, on the orbit without an
edit it is no worse than the measured margin, a standing frame makes no call, and with ``sparse`` and
``variance_guided`` a frame is the composition of the public pieces."""
import numpy as np
import pytest

import antilag_ref as R
import scenes
import temporal_ref as TR
from test_antilag_abi import NOISY, grey_case, history_of
from test_temporal import RES, STEPS, matrices, orbit_camera, random_case, rse

F = np.float32
# every parameter explicit: the bit-level tests do not depend on the library's defaults
EXPLICIT = dict(t_low=2.0, t_high=5.0, min_matches=3.0, sigma_normal=0.05, sigma_plane=0.02)
FLAT = dict(t_low=3.0, t_high=6.0, min_matches=8.0, sigma_normal=0.1, sigma_plane=0.00005)      # for the flat wall
# e_antilag / e_plain on the orbit without an edit, as tools/antilag_sweep.py measured it for the shipped defaults on
# cornell_box_spheres 64 x 64, and 2 % of it on top
NO_EDIT_RATIO = 0.014756699 / 0.014285087          # e_antilag / e_plain = 1.0330
NO_EDIT_BOUND = NO_EDIT_RATIO * 1.02


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def gpu():
    from vimg_amd import antilag, hip
    hip.init(0)
    return antilag


def _history(tensor, matrix=None):
    from vimg_amd import moments, temporal
    return (moments.History if tensor.shape[0] == 4 else temporal.History)(tensor, matrix)


def _run(lag, cur, hist, matrix, **kw):
    """antilag.rescale on device copies: (the history, the scale frame) as numpy arrays."""
    import torch
    dev = {k: torch.from_numpy(np.ascontiguousarray(cur[k])).cuda() for k in ("color", "normal", "position", "depth")}
    history = _history(torch.from_numpy(hist).cuda(), TR.IDENTITY)
    scale = torch.full(hist.shape[1:3], -7.0, device="cuda")
    got, s = lag.rescale(dev["color"], dev["normal"], dev["position"], dev["depth"], history, matrix, out_scale=scale, **kw)
    assert got is history and s is scale
    for k, v in dev.items():
        assert np.array_equal(_bits(v.cpu().numpy()), _bits(cur[k])), k          # the frames were only read
    return history.tensor.cpu().numpy(), scale.cpu().numpy()


def _check(lag, cur, hist, matrix, **params):
    want, want_s = R.rescale(cur["color"], cur["normal"], cur["position"], cur["depth"], hist, matrix, **params)
    got, s = _run(lag, cur, hist, matrix, **params)
    assert np.array_equal(_bits(s), _bits(want_s))
    assert np.array_equal(_bits(got), _bits(want))
    keep = np.ones(hist.shape, bool)
    keep[0, ..., 3] = False
    assert np.array_equal(_bits(got)[keep], _bits(hist)[keep])          # ... of which only the lengths may differ from before
    return want, want_s


SIZES = [(1, 1), (5, 3), (67, 5), (130, 9)]
RADII = [1, 4, 8]


@pytest.mark.gpu
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_kernels_are_the_restatement_bit_for_bit(gpu, size, radius):
    """W x H = 1 x 1, 5 x 3, 67 x 5 (a ragged second wave) and 130 x 9 (three workgroups across), radius 1, 4 and 8 (windows
    wider than the picture).  test_temporal.random_case - a bumpy surface, misses, a NaN and a negative depth, lengths
    0, fractional and negative - under the identity, a half-pixel shift and a perspective matrix, as it is and with
    the current colour halved on the left; with a NaN and an inf in each of the seven inputs in turn; a 4-plane
    moments history whose plane M must come back as it was; and the flat-wall cases of tests/test_antilag_abi.py:
    unchanged, shifted, a noise-free change, noise alone, noise and a change."""
    w, h = size
    f, prev = random_case(w, h)
    ms = matrices(w, h)
    kw = dict(EXPLICIT, radius=radius)
    values = set()
    for name, m in ms.items():
        _, s = _check(gpu, f, prev, m, **kw)
        g = dict(f, color=f["color"].copy())
        g["color"][:, : (w + 1) // 2] *= F(0.5)
        _, s2 = _check(gpu, g, prev, m, **kw)
        values |= set(np.unique(s).tolist()) | set(np.unique(s2).tolist())
    if w * h >= 15:
        d, v = R.pairs(f["color"], f["normal"], f["position"], f["depth"], prev, ms["half_pixel"], **kw)
        assert 0 < v.sum() < w * h
        assert 1.0 in values and min(values) < 1.0, values
    # NaN and inf in each input in turn
    n = w * h
    one, two = np.unravel_index(n // 3, (h, w)), np.unravel_index((2 * n) // 3, (h, w))
    for k in ("color", "normal", "position", "depth"):
        g = {a: v.copy() for a, v in f.items()}
        g[k][one][0] = np.nan
        g[k][two][1 if k != "depth" and one == two else 0] = np.inf
        _check(gpu, g, prev, ms["half_pixel"], **kw)
    for plane in range(3):
        q = prev.copy()
        q[(plane,) + one][0] = np.nan
        q[(plane,) + two][1] = np.inf                               # an infinite colour, normal, position
        _check(gpu, f, q, ms["half_pixel"], **kw)
    q = prev.copy()
    q[(0,) + one][3] = np.nan                                       # a NaN length: no history, not written
    _check(gpu, f, q, ms["identity"], **kw)
    # a moments history: plane M is not touched
    m4 = np.concatenate([prev, np.random.default_rng(3).normal(size=(1, h, w, 4)).astype(F)], axis=0)
    m4[3, 0, 0, 0] = np.nan
    want, _ = _check(gpu, f, m4, ms["perspective"], **kw)
    assert np.array_equal(_bits(want[3]), _bits(m4[3]))
    # the flat wall
    flat = dict(FLAT, radius=radius)
    for shift in (0.0, 2.0):
        cur, hist = grey_case(h, w, 0.625)
        cur["position"][..., 0] -= F(shift)
        want, s = _check(gpu, cur, hist, TR.shift_matrix(shift), **flat)
        assert (s == 1).all() and np.array_equal(_bits(want), _bits(hist))
    cur, hist = grey_case(h, w, 0.5, left=0.25)
    _, s = _check(gpu, cur, hist, TR.IDENTITY, **dict(flat, min_matches=2))
    x = np.arange(w)
    if w > 1:
        assert (s[:, x < w // 2 - radius] == 0).all() and (s[:, x >= w // 2 + radius] == 1).all()
    for left in (1.0, 0.5):
        cur, hist = grey_case(h, w, 1.0, sigma=0.5, left=left, seed=1)
        _check(gpu, cur, hist, TR.IDENTITY, **flat)


@pytest.mark.gpu
def test_the_noisy_cases_and_the_synthetic_sequence_on_the_gpu(gpu):
    """The two statistical cases of tests/test_antilag_abi.py at their own sizes (64 x 64: four workgroup rows) and
    parameters, and tests/temporal_ref.py's moving sequence, whose history pixels partly leave the picture or become
    hidden: the restatement's bits; the caps hold for what the GPU wrote."""
    for h, w in ((64, 64), (9, 130)):
        cur, hist = grey_case(h, w, 1.0, sigma=0.5, seed=1)
        _, s = _check(gpu, cur, hist, TR.IDENTITY, **dict(FLAT, **NOISY))
        assert (s < 1).mean() <= 0.02
        cur, hist = grey_case(h, w, 1.0, sigma=0.5, left=0.5, seed=1)
        _, s = _check(gpu, cur, hist, TR.IDENTITY, **dict(FLAT, **NOISY))
        assert (s[:, : w // 2 - NOISY["radius"]] == 0).mean() >= 0.95
    seq = TR.synthetic_sequence(16, 32, frames=3)
    for i in (1, 2):
        for radius in (1, 4, 8):
            _check(gpu, seq[i], history_of(seq[i - 1]), seq[i]["matrix"], **dict(FLAT, radius=radius))


@pytest.mark.gpu
def test_the_ways_to_call_it_and_what_is_refused(gpu):
    import torch
    from vimg_amd import hip, moments, temporal
    w, h = 67, 5
    f, prev = random_case(w, h)
    m = matrices(w, h)["perspective"]
    kw = dict(EXPLICIT, radius=2)
    want, want_s = R.rescale(f["color"], f["normal"], f["position"], f["depth"], prev, m, **kw)
    dev = [torch.from_numpy(f[k]).cuda() for k in ("color", "normal", "position", "depth")]
    fresh = lambda: temporal.History(torch.from_numpy(prev).cuda(), TR.IDENTITY)
    # a scale frame of the call's own, none at all, a workspace of the caller's, the defaults' radius by name
    hist, s = gpu.rescale(*dev, fresh(), m, **kw)
    assert np.array_equal(_bits(s.cpu().numpy()), _bits(want_s)) and np.array_equal(_bits(hist.tensor.cpu().numpy()), _bits(want))
    work = torch.empty((gpu.workspace_bytes(w, h),), dtype=torch.uint8, device="cuda")
    hist, s = gpu.rescale(*dev, fresh(), m, out_scale=False, workspace=work, **kw)
    assert s is None and np.array_equal(_bits(hist.tensor.cpu().numpy()), _bits(want))
    assert gpu.workspace_bytes(w, h) == 8 * w * h
    # numpy in, numpy out: a new history of the same class, the one handed in untouched
    mine = temporal.History(prev.copy(), TR.IDENTITY)
    hist, s = gpu.rescale(f["color"], f["normal"], f["position"], f["depth"], mine, m, **kw)
    assert isinstance(hist, temporal.History) and isinstance(hist.tensor, np.ndarray) and isinstance(s, np.ndarray)
    assert np.array_equal(_bits(hist.tensor), _bits(want)) and np.array_equal(_bits(s), _bits(want_s))
    assert np.array_equal(_bits(mine.tensor), _bits(prev)) and np.array_equal(hist.world_to_pixel, TR.IDENTITY)
    # a stream of the caller's
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    hist, s = gpu.rescale(*dev, fresh(), m, stream=side, **kw)
    side.synchronize()
    assert np.array_equal(_bits(s.cpu().numpy()), _bits(want_s)) and np.array_equal(_bits(hist.tensor.cpu().numpy()), _bits(want))
    # refused
    with pytest.raises(ValueError, match="antilag normal"):
        gpu.rescale(dev[0], dev[1][:, :4].contiguous(), dev[2], dev[3], fresh(), m)
    with pytest.raises(ValueError, match="history must be a temporal.History or a moments.History"):
        gpu.rescale(*dev, torch.from_numpy(prev).cuda(), m)
    with pytest.raises(ValueError, match="antilag history"):
        gpu.rescale(*dev, moments.History(torch.zeros((4, h, w - 1, 4), device="cuda")), m)
    with pytest.raises(ValueError, match="goes with numpy frames"):
        gpu.rescale(*dev, temporal.History(prev.copy()), m)
    with pytest.raises(ValueError, match="world_to_pixel must have 12 entries"):
        gpu.rescale(*dev, fresh(), m[:11])
    with pytest.raises(ValueError, match="antilag out_scale: out must be a contiguous torch.float32"):
        gpu.rescale(*dev, fresh(), m, out_scale=torch.zeros((h, w), dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError, match="antilag: unknown parameters"):
        gpu.rescale(*dev, fresh(), m, max_history=3)
    with pytest.raises(ValueError, match="antilag: radius must be 1..8"):
        gpu.rescale(*dev, fresh(), m, radius=-2)
    with pytest.raises(hip.HipError, match="radius must be 1..8, not 9"):
        gpu.rescale(*dev, fresh(), m, radius=9)
    with pytest.raises(hip.HipError, match="t_high must be > 3 and finite, not 2"):
        gpu.rescale(*dev, fresh(), m, t_low=3, t_high=2)
    with pytest.raises(hip.HipError, match="the workspace has 8 bytes"):
        gpu.rescale(*dev, fresh(), m, workspace=work[:8])
    hist = fresh()
    with pytest.raises(hip.HipError, match="the scale output overlaps the history"):
        gpu.rescale(*dev, hist, m, out_scale=hist.tensor.reshape(-1)[: h * w].view(h, w))
    with pytest.raises(hip.HipError, match="world-to-pixel entry 4 is not finite"):
        gpu.rescale(*dev, fresh(), np.where(np.arange(12) == 4, np.nan, m).astype(F))
    # the preview's option
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    scene = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    with pytest.raises(TypeError, match="antilag: unknown parameters"):
        scene.temporal_preview(p, antilag=dict(max_history=4))
    with pytest.raises(ValueError, match="antilag: radius must be"):
        scene.temporal_preview(p, antilag=dict(radius=-1))
    off, on = scene.temporal_preview(p), scene.temporal_preview(p, antilag=dict(radius=2, t_low=2.5))
    assert off.antilag is None and on.antilag == dict(radius=2, t_low=2.5) and on.last_scale is None
    off.close()
    on.close()
    scene.close()


# ---- on the renderer ---------------------------------------------------------------------------------------------
def _ibits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def dim_the_light(dev, host, factor=0.25):
    """update_materials with every emitting material's ``emit`` times ``factor``."""
    mats = host.materials()
    lit = 0
    for m in mats:
        if max(m.emit[0], m.emit[1], m.emit[2]) > 0:
            m.emit[0], m.emit[1], m.emit[2] = m.emit[0] * factor, m.emit[1] * factor, m.emit[2] * factor
            lit += 1
    assert lit
    dev.update_materials(materials=mats)


@pytest.fixture(scope="module")
def relit(gpu):
    """cornell_box_spheres 64 x 64, mis at 4 spp: the orbit of tests/test_temporal.py walked by a preview without antilag
    - the existing code path - and one with it, side by side on one resident scene; after its last step the light's
    emission is quartered and three more frames follow.  Everything the tests compare is recorded here."""
    from vimg_amd import hip
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    many = s.default_params(integrator="mis", samples=1024)
    plain, lag = dev.temporal_preview(p, samples=4, denoise=False), dev.temporal_preview(p, samples=4, denoise=False, antilag=True)
    o = dict(scales=[])
    for i in range(STEPS + 1):
        dev.set_camera(*orbit_camera(i))
        a, b = plain.frame().cpu().numpy(), lag.frame().cpu().numpy()
        if i:
            live = lag._frozen.tensor[1, ..., 3] > 0
            o["scales"].append(float(lag.last_scale[live].mean()))
            o["touched"] = float((lag.last_scale[live] < 1).float().mean())
    ref = dev.render(many, stats=False).cpu().numpy()
    o["orbit"] = (rse(a, ref), rse(b, ref))
    dim_the_light(dev, s)
    ref = dev.render(many, stats=False).cpu().numpy()
    o["after"] = []
    for k in range(3):
        a, b = plain.frame().cpu().numpy(), lag.frame().cpu().numpy()
        o["after"].append((rse(a, ref), rse(b, ref)))
        if k == 0:
            live = lag._frozen.tensor[1, ..., 3] > 0
            o["edit_scale"] = float(lag.last_scale[live].mean())
    o["finite"] = bool(np.isfinite(b).all())
    plain.close()
    lag.close()
    dev.close()
    return o


@pytest.mark.gpu
def test_after_the_light_is_dimmed_the_preview_with_antilag_is_nearer_the_relit_scene(relit):
    """(a) The first and the third frame after the edit, against mis at 1024 spp of the scene as edited: e with antilag
    strictly below e without; and the mean scale over the live history pixels is below what any orbit step without
    an edit gave.  Measured: frame 1 0.01225 against 0.26169, frame 3 0.00556 against 0.16989; mean scale 0.0611 against
    0.9374 .. 0.9764 on the orbit's steps."""
    (p1, l1), _, (p3, l3) = relit["after"]
    print(f"e after the edit, frame 1: plain {p1:.5f}, antilag {l1:.5f}; frame 3: plain {p3:.5f}, antilag {l3:.5f}; "
          f"mean scale {relit['edit_scale']:.4f} against {min(relit['scales']):.4f} .. {max(relit['scales']):.4f} on the orbit")
    assert relit["finite"]
    assert l1 < p1 and l3 < p3
    assert relit["edit_scale"] < min(relit["scales"])


@pytest.mark.gpu
def test_without_an_edit_antilag_costs_no_more_than_the_measured_margin(relit):
    """(b) The last frame of the orbit without an edit: e_antilag <= e_plain (1 + margin), e_plain from the preview
    without antilag, 1 + margin = the ratio tools/antilag_sweep.py measured for the shipped defaults on this scene
     and 2 % of it.  Measured: 0.01476 against 0.01429, ratio 1.0330 under the bound 1.0537; 9.78 % of
    the live history pixels had s < 1 on the last step."""
    e_plain, e_lag = relit["orbit"]
    print(f"e on the orbit without an edit: plain {e_plain:.5f}, antilag {e_lag:.5f} (ratio {e_lag / e_plain:.4f}, bound "
          f"{NO_EDIT_BOUND:.4f}); {100 * relit['touched']:.2f} % of the live history pixels had s < 1 on the last step")
    assert e_lag <= e_plain * NO_EDIT_BOUND


@pytest.mark.gpu
def test_a_standing_frame_makes_no_call_and_the_accumulator_stays_a_progressive(gpu, monkeypatch):
    """(c) frame(), set_camera, frame(), frame(), frame(): one rescale call, on the frame after the change - none on the
    first frame, which freezes no history, none while the camera stands - and the accumulator is bit for bit a plain
    Progressive after three increments."""
    import torch
    from vimg_amd import hip
    calls = []
    real = gpu.rescale
    monkeypatch.setattr(gpu, "rescale", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    preview = dev.temporal_preview(p, samples=4, denoise=False, antilag=True)
    preview.frame()
    assert not calls and preview.last_scale is None
    dev.set_camera(*orbit_camera(1))
    seen = []
    for _ in range(3):
        preview.frame()
        seen.append(len(calls))
    assert seen == [1, 1, 1] and preview.last_scale.shape == (RES, RES)
    plain = dev.progressive(p)
    for _ in range(3):
        plain.render(4, out=False)
    a, b = preview.acc.state(), plain.state()
    assert {k: bool(torch.equal(_ibits(a[k]), _ibits(b[k]))) for k in ("sum", "count", "batches", "m2")} == \
        dict(sum=True, count=True, batches=True, m2=True)
    for x in (preview, plain):
        x.close()
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["sparse", "variance_guided"])
def test_with_sparse_and_variance_guided_a_frame_after_the_edit_is_the_public_pieces(gpu, mode):
    """(d) Two frames of two cameras, then the light is dimmed and frame() runs: the frozen history is antilag.rescale of
    the last frame's history against this frame's increment - with ``sparse`` the filled one - under the current
    camera's matrix, every byte (plane M of the moments history included), last_scale is its scale frame, and the new
    history is wtemporal.accumulate / moments.accumulate on that rescaled history: all bit for bit, from the pieces
    called by hand."""
    import torch
    from vimg_amd import hip, infill, moments, temporal, wtemporal
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    kw = dict(sparse=2, denoise=False) if mode == "sparse" else dict(variance_guided=True)
    preview = dev.temporal_preview(p, samples=4, antilag=True, **kw)
    for cam in (0, 1):
        dev.set_camera(*orbit_camera(cam))
        preview.frame()
    cls = temporal.History if mode == "sparse" else moments.History
    assert isinstance(preview.history, cls)
    before = cls(preview.history.tensor.clone(), preview.history.world_to_pixel)
    dim_the_light(dev, s)
    got = preview.frame().clone()
    now = temporal.world_to_pixel(dev.camera)
    g = dev.render_features(p, infill.GUIDES)
    acc = dev.progressive(p)
    if mode == "sparse":
        noisy = acc.render(4, mask=infill.lattice_mask(RES, RES, 2, 2))          # the third frame since the reset: phase 2
        mean, code = infill.reconstruct(noisy, g["normal"], g["position"], g["depth"], acc.counts(), albedo=g["albedo"], radius=2)
    else:
        mean = acc.render(4)
    hist, scale = gpu.rescale(mean, g["normal"], g["position"], g["depth"], before, now)
    assert hist is before and torch.equal(_ibits(preview._frozen.tensor), _ibits(before.tensor))
    assert torch.equal(_ibits(preview.last_scale), _ibits(scale))
    assert (scale < 1).any() and (scale == 1).any()          # the edit was seen, and not everywhere
    if mode == "sparse":
        wgt = wtemporal.sparse_weights(acc.counts(), code, acc.state()["batches"], fill_weight=wtemporal.FILL_WEIGHT)
        out = torch.empty_like(mean)
        nxt, _ = wtemporal.accumulate(mean, g["normal"], g["position"], g["depth"], wgt, history=before, world_to_pixel=now, out=out)
        assert torch.equal(_ibits(got), _ibits(out))
    else:
        nxt = moments.accumulate(mean, g["normal"], g["position"], g["depth"], variance=None, history=before, world_to_pixel=now,
                                 current_weight=1)
    assert torch.equal(_ibits(preview.history.tensor), _ibits(nxt.tensor))
    assert torch.isfinite(got).all()
    for x in (preview, acc):
        x.close()
    dev.close()
