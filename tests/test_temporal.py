"""Temporal accumulation on the GPU (libvimg_temporal.so, include/vimg_temporal.h):
vimg_temporal_accumulate against the numpy restatement of its contract (tests/temporal_ref.py) BIT FOR BIT, then
temporal.world_to_pixel on rendered position frames, and DeviceScene.temporal_preview over a moving camera: nearer the
converged frame than the noisy frame and than the filter alone, the plain progressive stream while the camera stands."""
import math

import numpy as np
import pytest

import scenes
import temporal_ref as R

F = np.float32
# every parameter explicit: the bit-level tests do not depend on the library's defaults
EXPLICIT = dict(max_history=6.0, current_weight=1.0, sigma_normal=0.05, sigma_plane=0.02)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, produced=None):
    """The same bits.  ``produced``: a mask of the elements that the contract COMPUTES (a blend); there, and only there,
    a NaN is any NaN, because one that an operation produces (inf - inf) has no agreed sign.  What the contract copies -
    the guide planes, the colour of a pixel without history - keeps an injected NaN's bits."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F
    diff = _bits(got) != _bits(want)
    if produced is not None:
        diff &= ~(np.broadcast_to(produced, got.shape) & np.isnan(got) & np.isnan(want))
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def _blended(want):
    """[H, W, 1] mask of the pixels of a restated history whose plane A is a blend: a length that is neither 0 nor 1."""
    length = want[0, ..., 3]
    return ~((length == 0) | (length == 1))[..., None]


def _same_history(got, want):
    _same(got[0], want[0], _blended(want))
    _same(got[1:], want[1:])


def random_case(w, h, seed=0):
    """Current frames and a previous history of one slanted, bumpy surface, P near (x + 0.5, y + 0.5, -z): under matrices
    near the identity neighbours are tapped with fractional weights, and normals and positions differ enough that
    some taps pass the two surface tests and some fail.  From 15 pixels on, misses in both, a negative and a NaN
    depth, lengths 0 and fractional lengths in the history."""
    rng = np.random.default_rng(1000 * h + w + seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)

    def surface():
        n = np.stack([0.3 * np.sin(xx / 5.0), 0.3 * np.cos(yy / 7.0), np.ones_like(xx)], -1) + 0.04 * rng.normal(size=(h, w, 3))
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        z = 4.0 + 0.02 * xx + 0.03 * yy + 0.01 * rng.normal(size=(h, w))
        P = np.stack([xx + 0.5, yy + 0.5, -z], -1) + 0.2 * rng.uniform(-1, 1, size=(h, w, 3)) * np.array([1, 1, 0.1])
        return n, P, z

    n, P, z = surface()
    f = {k: np.ascontiguousarray(v, dtype=F) for k, v in dict(color=rng.gamma(2.0, 0.5, (h, w, 3)), normal=n, position=P,
                                                             depth=np.repeat(z[..., None], 3, -1)).items()}
    n, P, z = surface()
    prev = np.zeros((3, h, w, 4), F)
    prev[0, ..., :3] = rng.gamma(2.0, 0.5, (h, w, 3))
    prev[0, ..., 3] = np.where(rng.random((h, w)) < 0.5, rng.integers(1, 9, (h, w)), rng.uniform(0.5, 8, (h, w)))
    prev[1, ..., :3], prev[1, ..., 3], prev[2, ..., :3] = n, z, P
    if h * w >= 15:
        cells = rng.permutation(h * w)
        at = lambda i: np.unravel_index(cells[i], (h, w))
        m = max(1, h * w // 12)
        for i in range(m):                                 # misses: a twelfth of the frame, another of the history
            for k in ("normal", "position", "depth"):
                f[k][at(i)] = 0
            prev[(slice(None),) + at(m + i)] = 0
            prev[(0,) + at(m + i)][:3] = 0.25                # (a miss keeps its colour; its length is 0)
        f["depth"][at(2 * m)] = -1.0
        f["depth"][at(2 * m + 1)] = np.nan
        f["depth"][at(2 * m + 2)][1:] = (0.0, np.nan)      # only the first component is read: this pixel is live
        prev[(0,) + at(2 * m + 3)][3] = -2.0                 # a negative length is no surface either
    return f, prev


def matrices(w, h, seed=0):
    rng = np.random.default_rng(77 + seed)
    near = lambda: rng.uniform(-0.05, 0.05)
    # some pixels leave the image, and where x > ~0.6 w the point is behind the old camera (hw < 0)
    persp = np.array([1.1 + near(), near(), 0.1, 0.3, near(), 0.95 + near(), near(), 0.2,
                      -1.5 / w, 0.3 / h, near(), 0.9], F)
    return {"identity": R.IDENTITY, "half_pixel": R.shift_matrix(-0.5, -0.5), "perspective": persp}


@pytest.fixture(scope="module")
def gpu():
    from vimg_amd import hip, temporal
    hip.init(0)
    return temporal


def _run(tmp, f, prev, matrix, **kw):
    """temporal.accumulate on device copies: (next history, rgb output) as numpy arrays."""
    import torch
    dev = {k: torch.from_numpy(v).cuda() for k, v in f.items()}
    hist = None if prev is None else tmp.History(torch.from_numpy(prev).cuda(), matrix)
    out = torch.full_like(dev["color"], -7.0)
    nxt = tmp.accumulate(dev["color"], dev["normal"], dev["position"], dev["depth"], history=hist, out=out, **kw)
    assert np.array_equal(_bits(dev["color"].cpu().numpy()), _bits(f["color"]))          # the frame was only read
    return nxt.tensor.cpu().numpy(), out.cpu().numpy()


def _check(tmp, f, prev, matrix, **params):
    want = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], prev, matrix, **params)
    nxt, rgb = _run(tmp, f, prev, matrix, **params)
    _same_history(nxt, want)
    _same(rgb, np.ascontiguousarray(want[0, ..., :3]), _blended(want))
    return want


SIZES = [(1, 1), (5, 3), (67, 5), (130, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_kernel_is_the_restatement_bit_for_bit(gpu, size):
    """W x H = 1 x 1, 5 x 3, 67 x 5 (a ragged second wave) and 130 x 9 (three workgroups in both directions), each under
    the identity, a half-pixel shift and a perspective matrix that sends pixels off the image and behind the camera,
    with a NaN and an inf injected into each of the seven inputs in turn, without a history, with the output on the
    colour frame, with numpy frames, and on a stream of the caller's."""
    import torch
    w, h = size
    f, prev = random_case(w, h)
    ms = matrices(w, h)
    for name, m in ms.items():
        want = _check(gpu, f, prev, m, **EXPLICIT)
        L = want[0, ..., 3]
        if name == "perspective" and w * h >= 15:
            assert (L == 1).any() and (L > 1).any() and (L == 0).any()          # restarts, blends and misses
    # current_weight k and a cap below it
    _check(gpu, f, prev, ms["half_pixel"], **dict(EXPLICIT, current_weight=3.0, max_history=2.5))
    # NaN and inf in each input in turn
    n = w * h
    one, two = np.unravel_index(n // 3, (h, w)), np.unravel_index((2 * n) // 3, (h, w))
    for k in ("color", "normal", "position", "depth"):
        g = {a: v.copy() for a, v in f.items()}
        g[k][one][0] = np.nan
        g[k][two][1 if k != "depth" and one == two else 0] = np.inf
        _check(gpu, g, prev, ms["half_pixel"], **EXPLICIT)
    for plane in range(3):
        q = prev.copy()
        q[(plane,) + one][0] = np.nan
        q[(plane,) + two][3 if plane < 2 else 1] = np.inf           # an infinite length, depth, position
        _check(gpu, f, q, ms["half_pixel"], **EXPLICIT)
    # no history: lengths 1 and 0, the colour's bits
    want = _check(gpu, f, None, None, **EXPLICIT)
    assert np.array_equal(_bits(want[0, ..., :3]), _bits(f["color"])) and set(np.unique(want[0, ..., 3])) <= {0.0, 1.0}
    # the output is the colour frame itself; a next_history of the caller's
    want = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], prev, ms["perspective"], **EXPLICIT)
    dev = {k: torch.from_numpy(v).cuda() for k, v in f.items()}
    hist = gpu.History(torch.from_numpy(prev).cuda(), ms["perspective"])
    mine = torch.empty((3, h, w, 4), dtype=torch.float32, device="cuda")
    now = np.arange(12, dtype=F)
    res = gpu.accumulate(dev["color"], dev["normal"], dev["position"], dev["depth"], history=hist, world_to_pixel=now,
                         out=dev["color"], next_history=mine, **EXPLICIT)
    assert res.tensor is mine and np.array_equal(res.world_to_pixel, now)
    _same_history(mine.cpu().numpy(), want)
    _same(dev["color"].cpu().numpy(), np.ascontiguousarray(want[0, ..., :3]), _blended(want))
    _same(res.color.cpu().numpy(), want[0, ..., :3], _blended(want))
    _same(res.length.cpu().numpy(), want[0, ..., 3], _blended(want)[..., 0])
    # numpy in, numpy out (the history too)
    res = gpu.accumulate(f["color"], f["normal"], f["position"], f["depth"], history=gpu.History(prev, ms["perspective"]), **EXPLICIT)
    assert isinstance(res.tensor, np.ndarray)
    _same_history(res.tensor, want)
    # a stream of the caller's
    dev["color"] = torch.from_numpy(f["color"]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = gpu.accumulate(dev["color"], dev["normal"], dev["position"], dev["depth"], history=hist, stream=side, **EXPLICIT)
    side.synchronize()
    _same_history(res.tensor.cpu().numpy(), want)


@pytest.mark.gpu
def test_what_the_binding_and_the_library_refuse(gpu):
    import torch
    from vimg_amd import hip
    f, prev = random_case(5, 3)
    dev = [torch.from_numpy(f[k]).cuda() for k in ("color", "normal", "position", "depth")]
    hist = gpu.History(torch.from_numpy(prev).cuda(), R.IDENTITY)
    with pytest.raises(ValueError, match="temporal normal"):
        gpu.accumulate(dev[0], dev[1][:, :4].contiguous(), dev[2], dev[3])
    with pytest.raises(ValueError, match="does not know its world_to_pixel"):
        gpu.accumulate(*dev, history=gpu.History(hist.tensor))
    with pytest.raises(ValueError, match="temporal history"):
        gpu.accumulate(*dev, history=gpu.History(hist.tensor[:, :2].contiguous(), R.IDENTITY))
    with pytest.raises(TypeError, match="unknown parameters"):
        gpu.accumulate(*dev, iterations=3)
    with pytest.raises(hip.HipError, match="max_history must be >= 1"):
        gpu.accumulate(*dev, max_history=0.5)
    with pytest.raises(hip.HipError, match="overlaps the previous one"):
        gpu.accumulate(*dev, history=hist, next_history=hist.tensor)


# ---- on the renderer ---------------------------------------------------------------------------------------------
RES = 64
STEPS, DEGREES = 8, 1.5
PIVOT = np.array([278.0, 278.0, 556.0])      # the centre of the box's back wall
EYE0 = np.array([278.0, 278.0, -800.0])


def orbit_camera(i):
    """Step i of the orbit: the eye on a circle about the back wall's centre, 1.5 degrees per step about the vertical
    axis, keeping its viewing direction (+z).  (look_from, look_at, up, vfov)."""
    a = math.radians(DEGREES * i)
    r = EYE0 - PIVOT
    eye = PIVOT + np.array([r[0] * math.cos(a) + r[2] * math.sin(a), r[1], -r[0] * math.sin(a) + r[2] * math.cos(a)])
    return eye, eye + np.array([0.0, 0.0, 800.0]), (0.0, 1.0, 0.0), 40.0


def _project(m, position):
    """(column, row, hw) of a [.., 3] position frame under the 12 float32 of a world-to-pixel matrix, in float64."""
    m = np.asarray(m, np.float64).reshape(3, 4)
    hp = position.astype(np.float64) @ m[:, :3].T + m[:, 3]
    with np.errstate(all="ignore"):
        return hp[..., 0] / hp[..., 2], hp[..., 1] / hp[..., 2], hp[..., 2]


def rse(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float((((x - ref) ** 2) / (ref ** 2 + 0.01)).mean())


@pytest.fixture(scope="module")
def orbit(gpu):
    """The 8-step orbit of cornell_box_spheres at 64 x 64, mis at 4 spp, walked once by two previews of one resident
    scene (with and without the filter), then three more frames standing still; everything the tests compare is
    recorded here, so no test depends on what another left behind."""
    import torch
    from vimg_amd import hip
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    plain, filtered = dev.temporal_preview(p, samples=4, denoise=False), dev.temporal_preview(p, samples=4, denoise=True)
    shifts, first = [], None
    yy, xx = np.mgrid[0:RES, 0:RES]
    for i in range(STEPS + 1):
        dev.set_camera(*orbit_camera(i))
        old = plain.history
        frame = plain.frame().cpu().numpy()
        den = filtered.frame().cpu().numpy()
        if i == 0:
            first = frame
        else:                      # how far each surface point moved on the picture since the last step
            now = plain.history.tensor.cpu().numpy()              # planes G0 = {n, z}, G1 = {P, 0} of the new frame
            col, row, hw = _project(old.world_to_pixel, now[2, ..., :3])
            live = (now[1, ..., 3] > 0) & (hw > 0)
            shifts.append(float(np.median(np.hypot(col - (xx + 0.5), row - (yy + 0.5))[live])))
    o = dict(scene=s, dev=dev, params=p, shifts=shifts, first=first, temporal=frame, temporal_atrous=den,
             length=plain.history.length.cpu().numpy())
    o["noisy"] = dev.render(p, stats=False).cpu().numpy()
    o["atrous"] = dev.render_denoised(p).cpu().numpy()
    o["ref"] = dev.render(s.default_params(integrator="mis", samples=1024), stats=False).cpu().numpy()
    # standing still: three more frames of the same camera, beside a plain Progressive of it
    o["still"] = [frame] + [plain.frame().cpu().numpy() for _ in range(3)]
    acc = dev.progressive(p)
    for _ in range(4):
        acc.render(4, out=False)
    o["samples"] = (plain.acc.samples, acc.samples)
    a, b = plain.acc.state(), acc.state()
    as_bits = lambda v: v.view(torch.int32) if v.dtype == torch.float32 else v
    o["state_equal"] = {k: bool(torch.equal(as_bits(a[k]), as_bits(b[k]))) for k in ("sum", "count", "batches", "m2")}
    acc.close()
    plain.close()
    filtered.close()
    return o


@pytest.mark.gpu
def test_world_to_pixel_sends_every_covered_pixels_position_back_into_its_pixel(gpu):
    """cornell_box_spheres at 64 x 64, a pinhole, `position` at 1 spp: the first hit of the one sample of pixel (x, y)
    of the arrays projects into [x - 0.01, x + 1.01] x [y - 0.01, y + 1.01], for every pixel whose sample hit
    (coverage == 1), under the scene's own camera and under a camera set later.  The slack of 0.01 px is a thousand times
    the float32 error of a hit position at this scene's scale."""
    from vimg_amd import hip
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    dev = hip.DeviceScene(s)
    assert dev.camera.aperture_radius == 0 and (dev.camera.res_x, dev.camera.res_y) == (RES, RES)
    p = s.default_params(integrator="mis", samples=1)
    yy, xx = np.mgrid[0:RES, 0:RES]
    for cam in (None, orbit_camera(5), ((100.0, 420.0, -700.0), (300.0, 200.0, 300.0), (0.1, 1.0, 0.0), 55.0)):
        if cam is not None:
            dev.set_camera(*cam)
        g = {k: v.cpu().numpy() for k, v in dev.render_features(p, ("position", "coverage")).items()}
        live = g["coverage"][..., 0] == 1
        assert live.sum() > RES * RES // 2
        col, row, hw = _project(gpu.world_to_pixel(dev.camera), g["position"])
        assert (hw[live] > 0).all()
        dx, dy = (col - xx)[live], (row - yy)[live]
        print(f"world_to_pixel: column offset {dx.min():.4f} .. {dx.max():.4f}, row offset {dy.min():.4f} .. {dy.max():.4f}")
        assert dx.min() >= -0.01 and dx.max() <= 1.01 and dy.min() >= -0.01 and dy.max() <= 1.01


@pytest.mark.gpu
def test_the_orbit_moves_every_step_and_history_beats_the_noisy_frame_and_the_filter_alone(orbit):
    """Median reprojection shift per step >= 2 px: the per-pixel random streams, which restart identically after every
    reset, then meet different surface points.  Against mis at 1024 spp from the last camera,
    e = mean((x - ref)^2 / (ref^2 + 0.01)): temporal < noisy 4 spp, temporal + a-trous < a-trous alone.
    Measured: shifts 2.92 .. 3.06 px; noisy 0.05481, temporal 0.01429, a-trous alone 0.01825,
    temporal + a-trous 0.01514."""
    print("median shift per step:", " ".join(f"{v:.2f}" for v in orbit["shifts"]))
    assert len(orbit["shifts"]) == STEPS and min(orbit["shifts"]) >= 2.0
    e = {k: rse(orbit[k], orbit["ref"]) for k in ("noisy", "temporal", "atrous", "temporal_atrous")}
    print("relative squared error: " + ", ".join(f"{k} {v:.5f}" for k, v in e.items()))
    length = orbit["length"]
    print(f"history length: median {np.median(length):.2f}, {100 * (length > 1).mean():.1f} % of the pixels have history")
    assert np.isfinite(orbit["temporal"]).all() and np.isfinite(orbit["temporal_atrous"]).all()
    assert e["temporal"] < e["noisy"]
    assert e["temporal_atrous"] < e["atrous"]


@pytest.mark.gpu
def test_standing_still_continues_the_progressive_stream_and_the_error_falls(orbit):
    """After the orbit's last step (one frame at the last camera) three more frames without a change: the accumulator
    is bit for bit a Progressive after 4 x render(4), and e falls from each of the four frames to the next."""
    es = [rse(f, orbit["ref"]) for f in orbit["still"]]
    print("standing still, e per frame: " + " ".join(f"{v:.5f}" for v in es))
    assert orbit["samples"] == (16, 16)
    assert all(orbit["state_equal"].values()), orbit["state_equal"]
    assert len(es) == 4 and all(y < x for x, y in zip(es, es[1:])), es


@pytest.mark.gpu
def test_reset_then_frame_is_the_first_frames_bits(orbit):
    """Without history a frame is the plain render of its camera; reset() brings that back.  (A preview of its own.)"""
    dev, p = orbit["dev"], orbit["params"]
    tp = dev.temporal_preview(p, samples=4, denoise=False)
    dev.set_camera(*orbit_camera(STEPS - 1))
    tp.frame()
    dev.set_camera(*orbit_camera(STEPS))
    moved = tp.frame().cpu().numpy()
    assert (tp.history.length.cpu().numpy() > 1).any() and not np.array_equal(_bits(moved), _bits(orbit["noisy"]))
    tp.reset()
    again = tp.frame().cpu().numpy()
    assert np.array_equal(_bits(again), _bits(orbit["noisy"]))
    assert set(np.unique(tp.history.length.cpu().numpy())) <= {0.0, 1.0}
    # the same walk from the first camera gives the first frame's bits again
    dev.set_camera(*orbit_camera(0))
    tp.reset()
    assert np.array_equal(_bits(tp.frame().cpu().numpy()), _bits(orbit["first"]))
    tp.close()
    with pytest.raises(ValueError, match="whole frames"):
        dev.temporal_preview(orbit["scene"].default_params(samples=4, tile_world=2, tile_rank=0))


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [True, False])
def test_the_filtered_preview_is_accumulate_then_atrous_with_sigma_color_over_sqrt_n(gpu, scale):
    """denoise=True: frame n since the reset is filter.atrous on the unfiltered accumulation, guided by the frame's
    feature frames, at sigma_color / sqrt(n) - or, with scale_sigma_color=False, at sigma_color itself."""
    import torch
    from vimg_amd import filter as flt, hip
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    base = 1.5
    got, plain, guides = [], [], []
    for pv in (dev.temporal_preview(p, denoise=True, scale_sigma_color=scale, filter_kw=dict(sigma_color=base, iterations=2)),
               dev.temporal_preview(p, denoise=False)):
        for i in (0, 1):
            dev.set_camera(*orbit_camera(i))
            (got if pv.denoise else plain).append(pv.frame().clone())
            if not pv.denoise:
                guides.append(dev.render_features(p, flt.GUIDES))
        pv.close()
    for n, (out, acc, g) in enumerate(zip(got, plain, guides), start=1):
        want = flt.atrous(acc, g["normal"], g["position"], g["depth"], albedo=g["albedo"], iterations=2,
                          sigma_color=base / math.sqrt(n) if scale else base)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), n
    assert not torch.equal(got[1], plain[1])
