"""Temporal accumulation with per-pixel weights on the GPU (libvimg_wtemporal.so, include/vimg_wtemporal.h, DESIGN.md
4.24): vimg_wtemporal_accumulate against the numpy restatement of its contract (tests/wtemporal_ref.py) BIT FOR BIT,
against libvimg_temporal at uniform weights and on each other's histories, what the binding refuses, and
DeviceScene.temporal_preview(sparse=2): a frame is the composition of the public pieces, the lattice phase runs on
across camera changes, a standing camera ends at the plain progressive accumulator, and on the orbit of
tests/test_temporal.py the sparse preview is nearer the converged frame than a sparse render alone."""
import numpy as np
import pytest

import scenes
import temporal_ref as TR
import wtemporal_ref as R
from test_temporal import RES, STEPS, _same, matrices, orbit_camera, random_case, rse

F = np.float32
# every parameter explicit: the bit-level tests do not depend on the library's defaults
EXPLICIT = dict(max_history=6.0, sigma_normal=0.05, sigma_plane=0.02)
WEIGHTS = np.array([0, 0, 0.25, 1, 1, 3, np.nan, -1, np.inf], F)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def weights(w, h):
    return np.random.default_rng(5).choice(WEIGHTS, size=(h, w)).astype(F)


def _computed(code):
    """[H, W, 1] mask of the pixels whose plane A the contract COMPUTES (codes 2 and 3: H is a quotient of sums), where
    test_temporal._same takes any NaN for a NaN."""
    return ((code == R.BLENDED) | (code == R.CARRIED))[..., None]


def _same_result(history, rgb, code, want, want_code):
    assert code.dtype == np.uint8 and np.array_equal(code, want_code)
    _same(history[0], want[0], _computed(want_code))
    _same(history[1:], want[1:])
    if rgb is not None:
        _same(rgb, np.ascontiguousarray(want[0, ..., :3]), _computed(want_code))


@pytest.fixture(scope="module")
def gpu():
    from vimg_amd import hip, wtemporal
    hip.init(0)
    return wtemporal


def _run(wt, f, wgt, prev, matrix, **kw):
    """wtemporal.accumulate on device copies: (next history, rgb output, codes) as numpy arrays."""
    import torch
    dev = {k: torch.from_numpy(v).cuda() for k, v in f.items()}
    hist = None if prev is None else wt.History(torch.from_numpy(prev).cuda(), matrix)
    out = torch.full_like(dev["color"], -7.0)
    code = torch.full(wgt.shape, 9, dtype=torch.uint8, device="cuda")
    nxt, got = wt.accumulate(dev["color"], dev["normal"], dev["position"], dev["depth"], torch.from_numpy(wgt).cuda(), history=hist,
                             out=out, out_code=code, **kw)
    assert got is code
    assert np.array_equal(_bits(dev["color"].cpu().numpy()), _bits(f["color"]))          # the frame was only read
    return nxt.tensor.cpu().numpy(), out.cpu().numpy(), code.cpu().numpy()


def _check(wt, f, wgt, prev, matrix, **params):
    want, want_code = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], wgt, prev, matrix, **params)
    nxt, rgb, code = _run(wt, f, wgt, prev, matrix, **params)
    _same_result(nxt, rgb, code, want, want_code)
    return want, want_code


SIZES = [(1, 1), (5, 3), (67, 5), (130, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_kernel_is_the_restatement_bit_for_bit(gpu, size):
    """W x H = 1 x 1, 5 x 3, 67 x 5 (a ragged second wave) and 130 x 9 (three workgroups in both directions) of
    test_temporal.random_case, weights drawn from {0, 0, 0.25, 1, 1, 3, NaN, -1, inf}, each under the identity, a
    half-pixel shift and a perspective matrix - from 5 x 3 on the three together produce all five codes - with a NaN and
    an inf injected into each of the eight inputs in turn, without a history, with the output on the colour frame,
    without a code buffer, with numpy frames, and on a stream of the caller's."""
    import torch
    w, h = size
    f, prev = random_case(w, h)
    wgt = weights(w, h)
    ms = matrices(w, h)
    seen = set()
    for name, m in ms.items():
        _, code = _check(gpu, f, wgt, prev, m, **EXPLICIT)
        seen |= set(np.unique(code).tolist())
    if w * h >= 15:
        assert seen == {0, 1, 2, 3, 4}, seen
    # a cap below the weights
    _check(gpu, f, wgt, prev, ms["half_pixel"], **dict(EXPLICIT, max_history=2.5))
    # NaN and inf in each input in turn
    n = w * h
    one, two = np.unravel_index(n // 3, (h, w)), np.unravel_index((2 * n) // 3, (h, w))
    for k in ("color", "normal", "position", "depth"):
        g = {a: v.copy() for a, v in f.items()}
        g[k][one][0] = np.nan
        g[k][two][1 if k != "depth" and one == two else 0] = np.inf
        _check(gpu, g, wgt, prev, ms["half_pixel"], **EXPLICIT)
    v = wgt.copy()
    v[one], v[two] = np.nan, (np.inf if one != two else np.nan)
    _check(gpu, f, v, prev, ms["half_pixel"], **EXPLICIT)
    for plane in range(3):
        q = prev.copy()
        q[(plane,) + one][0] = np.nan
        q[(plane,) + two][3 if plane < 2 else 1] = np.inf           # an infinite length, depth, position
        _check(gpu, f, wgt, q, ms["half_pixel"], **EXPLICIT)
    # no history: codes 0, 1, 4, the colour's bits, lengths 0, the weight below 1, or 1
    want, code = _check(gpu, f, wgt, None, None, **EXPLICIT)
    assert np.array_equal(_bits(want[0, ..., :3]), _bits(f["color"])) and set(np.unique(code)) <= {0, 1, 4}
    assert set(np.unique(want[0, ..., 3])) <= {0.0, 0.25, 1.0}
    # the output is the colour frame itself; a next_history and a code buffer of the caller's
    want, want_code = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], wgt, prev, ms["perspective"], **EXPLICIT)
    dev = {k: torch.from_numpy(a).cuda() for k, a in f.items()}
    dw = torch.from_numpy(wgt).cuda()
    hist = gpu.History(torch.from_numpy(prev).cuda(), ms["perspective"])
    mine = torch.empty((3, h, w, 4), dtype=torch.float32, device="cuda")
    now = np.arange(12, dtype=F)
    res, code = gpu.accumulate(dev["color"], dev["normal"], dev["position"], dev["depth"], dw, history=hist, world_to_pixel=now,
                               out=dev["color"], next_history=mine, **EXPLICIT)
    assert res.tensor is mine and np.array_equal(res.world_to_pixel, now)
    _same_result(mine.cpu().numpy(), dev["color"].cpu().numpy(), code.cpu().numpy(), want, want_code)
    assert np.array_equal(_bits(dw.cpu().numpy()), _bits(wgt))                         # the weights were only read
    # no code buffer
    dev["color"] = torch.from_numpy(f["color"]).cuda()
    res, code = gpu.accumulate(dev["color"], dev["normal"], dev["position"], dev["depth"], dw, history=hist, out_code=False, **EXPLICIT)
    assert code is None
    _same_result(res.tensor.cpu().numpy(), None, want_code, want, want_code)
    # numpy in, numpy out (the history and the codes too)
    res, code = gpu.accumulate(f["color"], f["normal"], f["position"], f["depth"], wgt, history=gpu.History(prev, ms["perspective"]),
                               **EXPLICIT)
    assert isinstance(res.tensor, np.ndarray) and isinstance(code, np.ndarray)
    _same_result(res.tensor, None, code, want, want_code)
    # a stream of the caller's
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res, code = gpu.accumulate(dev["color"], dev["normal"], dev["position"], dev["depth"], dw, history=hist, stream=side, **EXPLICIT)
    side.synchronize()
    _same_result(res.tensor.cpu().numpy(), None, code.cpu().numpy(), want, want_code)


@pytest.mark.gpu
@pytest.mark.parametrize("v", [1.0, 3.0])
def test_uniform_weights_are_the_temporal_library_and_either_continues_the_others_history(gpu, v):
    """67 x 5: every weight v gives temporal.accumulate(current_weight=v)'s history and output bit for bit; a history
    written by libvimg_wtemporal (with mixed weights) is continued by libvimg_temporal as the restatements say, and
    the other way round."""
    import torch
    from vimg_amd import temporal
    w, h = 67, 5
    f, prev = random_case(w, h)
    m = matrices(w, h)["half_pixel"]
    dev = [torch.from_numpy(f[k]).cuda() for k in ("color", "normal", "position", "depth")]
    hist = temporal.History(torch.from_numpy(prev).cuda(), m)
    out_t, out_w = torch.empty_like(dev[0]), torch.empty_like(dev[0])
    a = temporal.accumulate(*dev, history=hist, world_to_pixel=m, out=out_t, current_weight=v, **EXPLICIT)
    b, code = gpu.accumulate(*dev, torch.full((h, w), v, device="cuda"), history=hist, world_to_pixel=m, out=out_w, **EXPLICIT)
    assert torch.equal(a.tensor.view(torch.int32), b.tensor.view(torch.int32))
    assert torch.equal(out_t.view(torch.int32), out_w.view(torch.int32))
    assert (code == 2).any() and not (code >= 3).any()
    # wtemporal (mixed weights) -> temporal
    wgt = weights(w, h)
    mixed, _ = gpu.accumulate(*dev, torch.from_numpy(wgt).cuda(), history=hist, world_to_pixel=m, **EXPLICIT)
    want_mixed, _ = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], wgt, prev, m, **EXPLICIT)
    got = temporal.accumulate(*dev, history=mixed, world_to_pixel=m, current_weight=v, **EXPLICIT)
    want = TR.accumulate(f["color"], f["normal"], f["position"], f["depth"], want_mixed, m, current_weight=v, **EXPLICIT)
    L = want[0, ..., 3]
    _same(got.tensor.cpu().numpy()[0], want[0], ~((L == 0) | (L == 1))[..., None])
    _same(got.tensor.cpu().numpy()[1:], want[1:])
    # temporal -> wtemporal (mixed weights)
    got, code = gpu.accumulate(*dev, torch.from_numpy(wgt).cuda(), history=a, world_to_pixel=m, **EXPLICIT)
    first = TR.accumulate(f["color"], f["normal"], f["position"], f["depth"], prev, m, current_weight=v, **EXPLICIT)
    want, want_code = R.accumulate(f["color"], f["normal"], f["position"], f["depth"], wgt, first, m, **EXPLICIT)
    _same_result(got.tensor.cpu().numpy(), None, code.cpu().numpy(), want, want_code)


@pytest.mark.gpu
def test_what_the_binding_and_the_library_refuse(gpu):
    import torch
    from vimg_amd import hip
    f, prev = random_case(5, 3)
    dev = [torch.from_numpy(f[k]).cuda() for k in ("color", "normal", "position", "depth")]
    wgt = torch.ones((3, 5), device="cuda")
    hist = gpu.History(torch.from_numpy(prev).cuda(), TR.IDENTITY)
    with pytest.raises(ValueError, match="wtemporal normal"):
        gpu.accumulate(dev[0], dev[1][:, :4].contiguous(), dev[2], dev[3], wgt)
    with pytest.raises(ValueError, match=r"wtemporal weight: shape must be \(3, 5\)"):
        gpu.accumulate(*dev, torch.ones((3, 5, 1), device="cuda"))
    with pytest.raises(ValueError, match="wtemporal weight: dtype must be float32"):
        gpu.accumulate(*dev, wgt.double())
    with pytest.raises(ValueError, match="wtemporal out_code: out must be a contiguous torch.uint8"):
        gpu.accumulate(*dev, wgt, out_code=torch.zeros((3, 5), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="does not know its world_to_pixel"):
        gpu.accumulate(*dev, wgt, history=gpu.History(hist.tensor))
    with pytest.raises(ValueError, match="wtemporal history"):
        gpu.accumulate(*dev, wgt, history=gpu.History(hist.tensor[:, :2].contiguous(), TR.IDENTITY))
    with pytest.raises(TypeError, match="unknown parameters"):
        gpu.accumulate(*dev, wgt, current_weight=2)
    with pytest.raises(hip.HipError, match="max_history must be >= 1"):
        gpu.accumulate(*dev, wgt, max_history=0.5)
    with pytest.raises(hip.HipError, match="the next history overlaps the previous one"):
        gpu.accumulate(*dev, wgt, history=hist, next_history=hist.tensor)
    out = torch.empty_like(dev[0])
    with pytest.raises(hip.HipError, match="the output codes overlap the output"):
        gpu.accumulate(*dev, wgt, out=out, out_code=out.view(torch.uint8).reshape(-1)[:15].view(3, 5))
    with pytest.raises(hip.HipError, match="the output codes overlap the weight frame"):
        gpu.accumulate(*dev, wgt, out_code=wgt.view(torch.uint8).reshape(-1)[:15].view(3, 5))
    with pytest.raises(ValueError, match="fill_weight must be >= 0"):
        gpu.sparse_weights(torch.zeros((3, 5), dtype=torch.int64), torch.zeros((3, 5), dtype=torch.uint8), fill_weight=-1)
    # sparse_weights: batches where sampled, fill_weight where the fill is guided, 0 for a fallback and a hole
    count = torch.tensor([[4, 0, 0, 0, 8]])
    code = torch.tensor([[0, 1, 2, 3, 0]], dtype=torch.uint8)
    assert gpu.sparse_weights(count, code, fill_weight=0.25).tolist() == [[1.0, 0.25, 0.0, 0.0, 1.0]]
    assert gpu.sparse_weights(count, code, torch.tensor([[1, 0, 0, 0, 2]]), fill_weight=0.5).tolist() == [[1.0, 0.5, 0.0, 0.0, 2.0]]
    # the preview
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    scene = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    with pytest.raises(ValueError, match="sparse does not go with variance_guided"):
        scene.temporal_preview(p, sparse=2, variance_guided=True)
    for stride in (1, 5):
        with pytest.raises(ValueError, match="stride must be 2..4"):
            scene.temporal_preview(p, sparse=stride)
    with pytest.raises(ValueError, match="fill_weight"):
        scene.temporal_preview(p, fill_weight=0.5)
    with pytest.raises(ValueError, match="whole frames"):
        scene.temporal_preview(s.default_params(samples=4, tile_world=2, tile_rank=0), sparse=2)
    scene.close()


# ---- on the renderer ---------------------------------------------------------------------------------------------
def _ibits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.gpu
def test_a_sparse_frame_is_the_composition_of_the_public_pieces_and_the_phase_runs_on(gpu):
    """cornell_box_spheres 64 x 64, mis, temporal_preview(p, samples=4, sparse=2, denoise=False): a first frame, a moved
    frame, a standing frame, another moved one and more standing ones.  Each frame is bit for bit lattice_mask at the
    running phase -> Progressive.render(4, mask) -> infill.reconstruct(counts, cached guides, albedo, radius 2) ->
    sparse_weights(batches) -> wtemporal.accumulate against the history frozen at the last camera change.  The phase
    goes 0, 1, 2, 3, 0, 1, 2 whatever the camera does; after the four standing frames of the last camera the
    accumulator equals a plain Progressive after render(4) in every field.  sparse=None is the existing preview."""
    import torch
    from vimg_amd import hip, infill, temporal
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    preview = dev.temporal_preview(p, samples=4, sparse=2, denoise=False)
    assert preview.sparse == 2 and preview.fill_weight == gpu.FILL_WEIGHT and preview.phase is None
    acc = dev.progressive(p)
    cameras = [0, 1, None, 2, None, None, None]           # None: the camera stands
    frozen = last = guides = None
    phases = []
    for i, cam in enumerate(cameras):
        if cam is not None:
            dev.set_camera(*orbit_camera(cam))
            acc.reset()
            frozen, guides = last, dev.render_features(p, infill.GUIDES)
        got = preview.frame().clone()
        phases.append(preview.phase)
        noisy = acc.render(4, mask=infill.lattice_mask(RES, RES, 2, i % 4))
        filled, code = infill.reconstruct(noisy, guides["normal"], guides["position"], guides["depth"], acc.counts(),
                                          albedo=guides["albedo"], radius=2)
        wgt = gpu.sparse_weights(acc.counts(), code, acc.state()["batches"], fill_weight=gpu.FILL_WEIGHT)
        out = torch.empty_like(filled)
        last, what = gpu.accumulate(filled, guides["normal"], guides["position"], guides["depth"], wgt, history=frozen,
                                    world_to_pixel=temporal.world_to_pixel(dev.camera), out=out)
        assert torch.equal(_ibits(got), _ibits(out)), i
        assert torch.equal(_ibits(preview.history.tensor), _ibits(last.tensor)), i
        assert isinstance(preview.history, temporal.History)
        assert np.array_equal(preview.history.world_to_pixel, temporal.world_to_pixel(dev.camera))
        if i == 1:            # the moved frame: sampled and filled pixels alike found history, and some started over
            unsampled = acc.counts() == 0
            assert ((what == 2) & unsampled).any() and ((what == 2) & ~unsampled).any() and (what == 1).any()
            assert (wgt[unsampled] <= gpu.FILL_WEIGHT).all() and (wgt[~unsampled] == 1).all()
    assert phases == [0, 1, 2, 3, 0, 1, 2]
    assert preview.acc.launches == 4 == acc.launches          # each frame since the last reset: one render launch
    # the last camera has had phases 3, 0, 1, 2: every pixel its four samples
    plain = dev.progressive(p)
    plain.render(4, out=False)
    a, b = preview.acc.state(), plain.state()
    assert {k: bool(torch.equal(_ibits(a[k]), _ibits(b[k]))) for k in ("sum", "count", "batches", "m2")} == \
        dict(sum=True, count=True, batches=True, m2=True)
    assert preview.acc.samples == 4
    for x in (preview, acc, plain):
        x.close()
    # sparse=None: render + temporal.accumulate at current_weight 1, as before
    old = dev.temporal_preview(p, samples=4, denoise=False, sparse=None)
    hist = None
    for cam in (0, 1):
        dev.set_camera(*orbit_camera(cam))
        got = old.frame().clone()
        g = dev.render_features(p, ("normal", "position", "depth"))
        out = torch.empty_like(got)
        hist = temporal.accumulate(dev.render(p, stats=False), g["normal"], g["position"], g["depth"], history=hist,
                                   world_to_pixel=temporal.world_to_pixel(dev.camera), out=out, current_weight=1)
        assert torch.equal(_ibits(got), _ibits(out)) and torch.equal(_ibits(old.history.tensor), _ibits(hist.tensor))
    old.close()
    dev.close()


@pytest.mark.gpu
def test_on_the_orbit_the_sparse_preview_beats_a_sparse_render_alone(gpu):
    """The orbit of tests/test_temporal.py (cornell_box_spheres 64 x 64, 8 steps of 1.5 degrees, mis at 4 spp), a quarter
    of the pixels sampled per frame: on the last frame everything is finite and, against mis at 1024 spp,
    e(temporal_preview(sparse=2)) < e(dev.render_sparse(p, stride=2)) - the sparse picture the library could make
    before, at that camera and those 4 samples.  An ordering, not a size.
    Measured at fill_weight 1/16: sparse preview 0.02125, sparse render alone 0.04116 (at 1/8: 0.02106); on the orbit
    of tools/wtemporal_sweep.py 0.01311 against 0.03143."""
    from vimg_amd import hip
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    preview = dev.temporal_preview(p, samples=4, sparse=2, denoise=False)
    for i in range(STEPS + 1):
        dev.set_camera(*orbit_camera(i))
        frame = preview.frame()
    frame = frame.cpu().numpy()
    length = preview.history.length.cpu().numpy()
    alone = dev.render_sparse(p, stride=2).cpu().numpy()
    ref = dev.render(s.default_params(integrator="mis", samples=1024), stats=False).cpu().numpy()
    e_preview, e_alone = rse(frame, ref), rse(alone, ref)
    print(f"relative squared error: sparse preview {e_preview:.5f}, sparse render alone {e_alone:.5f}; "
          f"history length median {np.median(length):.2f}")
    preview.close()
    dev.close()
    assert np.isfinite(frame).all() and np.isfinite(length).all()
    assert e_preview < e_alone
