"""The sampling mask of a sparse preview on the GPU (libvimg_demand.so, include/vimg_demand.h):
vimg_demand_mask against the numpy restatement of its contract (tests/demand_ref.py) BIT FOR BIT - the mask, the lengths
and the four counts - at the sizes where the launch shape and its reduction can go wrong and with everything a lookup can
meet planted; its lengths against the ones libvimg_wtemporal carries; and ``demand=`` on DeviceScene.temporal_preview: a
frame is the composition of the public pieces, min_history 0 is the plain sparse preview, a standing camera ends at the
plain progressive accumulator, and on the orbit of tests/test_temporal.py the preview with demand is nearer the converged
frame than the one without."""
import numpy as np
import pytest

import demand_ref as R
import scenes
import temporal_ref as TR
from test_temporal import RES, STEPS, orbit_camera, rse

pytestmark = pytest.mark.gpu
F = np.float32
# every parameter explicit: the bit-level tests do not depend on the library's defaults
EXPLICIT = dict(min_history=1.5, sigma_normal=0.05, sigma_plane=0.02)
GUIDES = ("normal", "position", "depth")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ibits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module")
def gpu():
    from vimg_amd import demand, hip
    hip.init(0)
    return demand


def _check(dm, cur, prev, matrix, lengths=True, counts=True, **kw):
    """demand.mask on device copies against the restatement: the mask's bytes, the lengths' bits, the four counts.  The
    outputs are the caller's buffers, filled with something else first; the guides and the history are only read."""
    import torch
    from vimg_amd import temporal
    want_mask, want_length, want_counts = R.mask(cur["normal"], cur["position"], cur["depth"], prev, matrix, **kw)
    dev = {k: torch.from_numpy(cur[k]).cuda() for k in GUIDES}
    d_prev = None if prev is None else torch.from_numpy(prev).cuda()
    hist = None if prev is None else temporal.History(d_prev, matrix)
    h, w = want_mask.shape
    out = torch.full((h, w), 9, dtype=torch.uint8, device="cuda")
    out_length = torch.full((h, w), -7.0, device="cuda") if lengths else False
    out_counts = torch.full((4,), 77, dtype=torch.int32, device="cuda") if counts else False
    m, L, c = dm.mask(dev["normal"], dev["position"], dev["depth"], history=hist, out=out, out_length=out_length, counts=out_counts, **kw)
    assert m is out and (L is out_length if lengths else L is None) and (c is out_counts if counts else c is None)
    got = m.cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want_mask), np.argwhere(got != want_mask)[:4].tolist()
    if lengths:
        gl = L.cpu().numpy()
        diff = _bits(gl) != _bits(want_length)
        assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist(), gl[diff][:4], want_length[diff][:4])
    if counts:
        assert dm.read(c) == R.read(want_counts)
    for k in GUIDES:
        assert np.array_equal(_bits(dev[k].cpu().numpy()), _bits(cur[k]))
    if prev is not None:
        assert np.array_equal(_bits(d_prev.cpu().numpy()), _bits(prev))
    return want_mask, want_length, R.read(want_counts)


# 1 x 1; 7 x 5, less than a wave and more than a workgroup's four rows; 65 x 4, a ragged second wave per row; 130 x 67,
# 3 x 17 workgroups with ragged rows and columns
SIZES = [(1, 1), (7, 5), (65, 4), (130, 67)]


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_kernel_is_the_restatement_bit_for_bit(gpu, size):
    """demand_ref.planted: misses, NaN guides and depths, history lengths 0, negative, NaN and infinite, projections behind
    the old camera and off every edge, fx and fy in (-1, 0) and (w - 1, w) - at strides 0, 2, 3 and 4, explicit parameters
    and the defaults, with and without a history, with and without the optional outputs."""
    w, h = size
    cur, prev, matrix = R.planted(h, w, seed=w)
    for stride, phase in ((0, 0), (2, 1), (3, 7), (4, 10)):
        _, L, c = _check(gpu, cur, prev, matrix, stride=stride, phase=phase, **EXPLICIT)
        _check(gpu, cur, prev, matrix, stride=stride, phase=phase)
    if w * h > 100:
        assert 0 < c["needed"] < c["live"] < w * h and (L > 0).any()
    _check(gpu, cur, None, None, stride=2, phase=3, **EXPLICIT)
    _check(gpu, cur, prev, matrix, lengths=False, stride=3, phase=0, **EXPLICIT)
    _check(gpu, cur, prev, matrix, counts=False, stride=3, phase=0, **EXPLICIT)
    _check(gpu, cur, prev, matrix, lengths=False, counts=False, stride=0, phase=0, min_history=0.0)


def test_every_phase_of_every_stride_at_13_x_9(gpu):
    cur, prev, matrix = R.planted(9, 13, seed=2)
    seen = set()
    for stride in (2, 3, 4):
        for phase in range(stride * stride):
            m = _check(gpu, cur, prev, matrix, stride=stride, phase=phase, min_history=0.0)[0]
            assert np.array_equal(m.astype(bool), R.lattice(9, 13, stride, phase))
            seen.add(m.tobytes())
            _check(gpu, cur, prev, matrix, stride=stride, phase=phase, **EXPLICIT)
    assert len(seen) == 4 + 9 + 16


def test_the_length_is_the_one_wtemporal_carries_at_weight_0(gpu):
    """Across libraries, on the same device inputs: wtemporal.accumulate with weight 0 everywhere and max_history 3e38
    writes, as plane A's length, the reprojected length where it carries and 0 elsewhere - demand's lengths, bit for bit;
    and its code-4 pixels and carried lengths below min_history are demand's needed set."""
    import torch
    from vimg_amd import temporal, wtemporal
    cases = [R.planted(67, 130, seed=11, infinite=False)]      # (an infinite length is cut to max_history there, and kept here)
    seq = TR.synthetic_sequence(16, 32, frames=3, seed=2)
    prev = TR.accumulate(*(seq[1][k] for k in ("color",) + GUIDES), TR.accumulate(*(seq[0][k] for k in ("color",) + GUIDES), max_history=32,
                         current_weight=1, sigma_normal=0.1, sigma_plane=0.00005), seq[0]["matrix"], max_history=32, current_weight=1,
                         sigma_normal=0.1, sigma_plane=0.00005)
    cases.append(({k: seq[2][k] for k in GUIDES}, prev, seq[1]["matrix"]))
    for cur, prev, matrix in cases:
        dev = {k: torch.from_numpy(cur[k]).cuda() for k in GUIDES}
        hist = temporal.History(torch.from_numpy(prev).cuda(), matrix)
        h, w = cur["depth"].shape[:2]
        color = torch.rand((h, w, 3), device="cuda")
        for sigmas in (dict(sigma_normal=0.1, sigma_plane=0.00005), dict(sigma_normal=0.05, sigma_plane=0.02)):
            nxt, code = wtemporal.accumulate(color, dev["normal"], dev["position"], dev["depth"], torch.zeros((h, w), device="cuda"),
                                             history=hist, world_to_pixel=matrix, max_history=3e38, **sigmas)
            m, L, c = gpu.mask(dev["normal"], dev["position"], dev["depth"], history=hist, stride=0, phase=0, min_history=1.0, **sigmas)
            assert torch.equal(_ibits(L), _ibits(nxt.length.contiguous()))
            need = (code == 4) | ((code == 3) & (nxt.length < 1.0))
            assert torch.equal(m.bool(), need) and (code == 3).any() and (code == 4).any()
            assert gpu.read(c) == dict(masked=int(need.sum()), needed=int(need.sum()), extra=int(need.sum()), live=int((code != 0).sum()))


def test_numpy_frames_a_callers_stream_and_what_is_refused(gpu):
    import torch
    from vimg_amd import hip, moments, temporal
    cur, prev, matrix = R.planted(67, 130, seed=5)
    kw = dict(stride=2, phase=2, **EXPLICIT)
    want_mask, want_length, want_counts = R.mask(cur["normal"], cur["position"], cur["depth"], prev, matrix, **kw)
    # numpy in, numpy out; the counts stay on the device
    m, L, c = gpu.mask(cur["normal"], cur["position"], cur["depth"], history=temporal.History(prev, matrix), **kw)
    assert isinstance(m, np.ndarray) and isinstance(L, np.ndarray) and isinstance(c, torch.Tensor) and c.is_cuda
    assert np.array_equal(m, want_mask) and np.array_equal(_bits(L), _bits(want_length)) and gpu.read(c) == R.read(want_counts)
    # a caller's stream while the default one is current, and a moments.History, whose first three planes are read
    side = torch.cuda.Stream()
    dev = {k: torch.from_numpy(cur[k]).cuda() for k in GUIDES}
    four = torch.cat([torch.from_numpy(prev).cuda(), torch.full((1, 67, 130, 4), float("nan"), device="cuda")])
    torch.cuda.synchronize()
    m, L, c = gpu.mask(dev["normal"], dev["position"], dev["depth"], history=moments.History(four, matrix), stream=side, **kw)
    side.synchronize()
    assert np.array_equal(m.cpu().numpy(), want_mask) and np.array_equal(_bits(L.cpu().numpy()), _bits(want_length))
    assert gpu.read(c) == R.read(want_counts)
    # what the binding and the library refuse
    hist = temporal.History(torch.from_numpy(prev).cuda(), matrix)
    with pytest.raises(ValueError, match="demand normal: shape must be"):
        gpu.mask(dev["normal"][..., 0], dev["position"], dev["depth"])
    with pytest.raises(ValueError, match="demand depth"):
        gpu.mask(dev["normal"], dev["position"], dev["depth"][:, :5].contiguous())
    with pytest.raises(ValueError, match="demand: history must be a temporal.History or a moments.History"):
        gpu.mask(dev["normal"], dev["position"], dev["depth"], history=prev)
    with pytest.raises(ValueError, match="demand: the history does not know its world_to_pixel matrix"):
        gpu.mask(dev["normal"], dev["position"], dev["depth"], history=temporal.History(hist.tensor))
    with pytest.raises(ValueError, match="demand: out must be"):
        gpu.mask(dev["normal"], dev["position"], dev["depth"], out=torch.empty(67, 130, device="cuda"))
    with pytest.raises(ValueError, match="demand: counts must be a contiguous CUDA tensor of 16 bytes"):
        gpu.mask(dev["normal"], dev["position"], dev["depth"], counts=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(hip.HipError, match="stride must be 0 or 2..4, not 5"):
        gpu.mask(dev["normal"], dev["position"], dev["depth"], stride=5)
    with pytest.raises(hip.HipError, match="phase must be 0..3 at stride 2, not 4"):
        gpu.mask(dev["normal"], dev["position"], dev["depth"], phase=4)
    with pytest.raises(hip.HipError, match="the output lengths overlap the previous history"):
        gpu.mask(dev["normal"], dev["position"], dev["depth"], history=hist, out_length=hist.tensor.view(-1)[4:4 + 67 * 130].view(67, 130))


# ---- rendered frames ------------------------------------------------------------------------------------------------
def _scene():
    from vimg_amd import hip
    s = scenes.json_scene("cornell_box_spheres.json", res=(RES, RES))
    return s, hip.DeviceScene(s), s.default_params(integrator="mis", samples=4)


def test_min_history_0_is_the_plain_sparse_preview_and_demand_needs_sparse(gpu):
    """cornell_box_spheres 64 x 64, mis at 4 spp, sparse=2, denoise=False: with demand=dict(min_history=0) the first, a
    moved (1.5 degrees) and a standing frame are the plain sparse preview's bits - frame, history and accumulator."""
    import torch
    s, dev, p = _scene()
    plain = dev.temporal_preview(p, samples=4, sparse=2, denoise=False)
    none = dev.temporal_preview(p, samples=4, sparse=2, denoise=False, demand=None)
    zero = dev.temporal_preview(p, samples=4, sparse=2, denoise=False, demand=dict(min_history=0))
    assert plain.demand is None and plain.last_demand is None and none.demand is None and zero.demand == dict(min_history=0)
    assert zero.last_demand is None
    for i, cam in enumerate((0, 1, None)):
        if cam is not None:
            dev.set_camera(*orbit_camera(cam))
        want, same, got = (x.frame().clone() for x in (plain, none, zero))
        assert torch.equal(_ibits(same), _ibits(want)) and torch.equal(_ibits(got), _ibits(want)), i
        assert torch.equal(_ibits(zero.history.tensor), _ibits(plain.history.tensor)), i
        a, b = zero.acc.state(), plain.acc.state()
        assert all(torch.equal(_ibits(a[k]), _ibits(b[k])) for k in ("sum", "count", "batches", "m2")), i
        assert zero.phase == plain.phase == i
        c = gpu.read(zero.last_demand[2])
        assert c["needed"] == c["extra"] == 0 and c["masked"] == RES * RES // 4 and 0 < c["live"] <= RES * RES
    with pytest.raises(ValueError) as e:
        dev.temporal_preview(p, samples=4, demand=True)
    assert str(e.value) == "temporal_preview: demand chooses the pixels a sparse frame samples: it needs sparse"
    with pytest.raises(ValueError, match="temporal_preview: demand must be None, a bool or a dict"):
        dev.temporal_preview(p, sparse=2, demand=2)
    with pytest.raises(TypeError, match=r"demand: unknown parameters \['sigma_plane'\]"):
        dev.temporal_preview(p, sparse=2, demand=dict(sigma_plane=0.1))
    for x in (plain, none, zero):
        x.close()
    dev.close()


def test_a_frame_with_demand_is_the_composition_of_the_public_pieces(gpu):
    """The same scene with demand=True: a first frame, a moved frame and three standing ones.  The first frame leaves no
    live pixel at count 0.  Each frame is bit for bit the mask -> Progressive.render(4, mask) -> infill.reconstruct ->
    sparse_weights -> wtemporal.accumulate against the frozen history, the mask being demand.mask of the guides against
    that history at the frame's phase on the frame after a change and lattice & (count <= 4 (k // 4)) on standing frame
    k.  On the moved frame wtemporal's codes hold no code 4, and code 1 only at sampled pixels.  Every standing mask
    holds one count, every frame is one render launch, and after the four frames of the last camera the accumulator is a
    Progressive after render(4)."""
    import torch
    from vimg_amd import hip, infill, temporal, wtemporal
    s, dev, p = _scene()
    preview = dev.temporal_preview(p, samples=4, sparse=2, denoise=False, demand=True)
    assert preview.demand == {} and preview.sparse == 2
    acc = dev.progressive(p)
    cameras = [0, 1, None, None, None]
    frozen = last = guides = None
    k = 0
    for i, cam in enumerate(cameras):
        if cam is not None:
            dev.set_camera(*orbit_camera(cam))
            acc.reset()
            frozen, guides, k = last, dev.render_features(p, infill.GUIDES), 0
        got = preview.frame().clone()
        live = guides["depth"][..., 0] > 0
        lattice = infill.lattice_mask(RES, RES, 2, i % 4)
        if k == 0:
            mask, length, counts = gpu.mask(guides["normal"], guides["position"], guides["depth"], history=frozen, stride=2, phase=i % 4)
            assert torch.equal(preview.last_demand[0], mask) and torch.equal(_ibits(preview.last_demand[1]), _ibits(length))
            c = gpu.read(counts)
            assert gpu.read(preview.last_demand[2]) == c and c["live"] == int(live.sum())
            print(f"frame {i}: {c}")
        else:
            before = acc.counts()
            mask = lattice & (before <= 4 * (k // 4)).to(torch.uint8)
            assert len(torch.unique(before[mask.bool()])) == 1          # one count: one render launch
            assert int(mask.sum()) < int(lattice.sum())                  # some pixel was sampled on demand and skips its turn
        noisy = acc.render(4, mask=mask)
        filled, code = infill.reconstruct(noisy, guides["normal"], guides["position"], guides["depth"], acc.counts(),
                                          albedo=guides["albedo"], radius=2)
        wgt = wtemporal.sparse_weights(acc.counts(), code, acc.state()["batches"], fill_weight=wtemporal.FILL_WEIGHT)
        out = torch.empty_like(filled)
        last, what = wtemporal.accumulate(filled, guides["normal"], guides["position"], guides["depth"], wgt, history=frozen,
                                          world_to_pixel=temporal.world_to_pixel(dev.camera), out=out)
        assert torch.equal(_ibits(got), _ibits(out)), i
        assert torch.equal(_ibits(preview.history.tensor), _ibits(last.tensor)), i
        assert preview.phase == i % 4
        sampled = acc.counts() > 0
        if i == 0:            # no history: lattice and every live pixel
            assert c["needed"] == c["live"] and torch.equal(mask.bool(), lattice.bool() | live)
            assert not (live & ~sampled).any()
        if i == 1:            # the moved frame: most pixels found their history, the uncovered ones were sampled
            assert 0 < c["extra"] < c["needed"] < c["live"] and c["masked"] < RES * RES // 2
            assert not (what == 4).any() and (what == 1).any() and not ((what == 1) & ~sampled).any()
            assert ((what == 3) | (what == 2)).sum() > RES * RES // 2
        k += 1
    assert preview.acc.launches == 4 == acc.launches
    plain = dev.progressive(p)
    plain.render(4, out=False)
    a, b = preview.acc.state(), plain.state()
    assert {n: bool(torch.equal(_ibits(a[n]), _ibits(b[n]))) for n in ("sum", "count", "batches", "m2")} == \
        dict(sum=True, count=True, batches=True, m2=True)
    assert preview.acc.samples == 4
    # reset(): the next frame is a first frame again
    preview.reset()
    assert preview.last_demand is None
    preview.frame()
    c = gpu.read(preview.last_demand[2])
    assert c["needed"] == c["live"] > 0
    for x in (preview, acc, plain):
        x.close()
    dev.close()


def test_on_the_orbit_demand_is_nearer_the_converged_frame_than_the_lattice_alone(gpu):
    """The orbit of tests/test_temporal.py (cornell_box_spheres 64 x 64, 8 steps of 1.5 degrees, mis at 4 spp), sparse=2,
    with and without demand=True: e of the last frame against mis at 1024 spp.  Frame by frame the pixels sampled with
    demand are a superset of the lattice's, and a pixel's sample stream does not depend on which frame draws it.  An
    ordering, not a size."""
    s, dev, p = _scene()
    lattice, demand = dev.temporal_preview(p, samples=4, sparse=2, denoise=False), dev.temporal_preview(p, samples=4, sparse=2, denoise=False, demand=True)
    shares = []
    for i in range(STEPS + 1):
        dev.set_camera(*orbit_camera(i))
        a, b = lattice.frame(), demand.frame()
        shares.append(gpu.read(demand.last_demand[2])["masked"] / (RES * RES))
    a, b = a.cpu().numpy(), b.cpu().numpy()
    ref = dev.render(s.default_params(integrator="mis", samples=1024), stats=False).cpu().numpy()
    e_lattice, e_demand = rse(a, ref), rse(b, ref)
    print(f"relative squared error: lattice alone {e_lattice:.5f}, with demand {e_demand:.5f}; share of pixels sampled per frame "
          f"{' '.join(f'{x:.3f}' for x in shares)}")
    lattice.close()
    demand.close()
    dev.close()
    assert np.isfinite(b).all()
    assert all(x >= 0.25 for x in shares)          # a superset of the lattice's quarter
    assert e_demand < e_lattice
