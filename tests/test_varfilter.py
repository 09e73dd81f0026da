"""The variance-guided a-trous filter on the GPU (libvimg_varfilter.so, include/vimg_varfilter.h):
vimg_varfilter_atrous against the numpy restatement of its contract (tests/varfilter_ref.py) BIT FOR BIT, both outputs -
on random frames that hold every special pixel the contract names and every kind of variance, and on rendered frames
with an accumulator's variance - then vimg_varfilter_variance against the accumulator's own error, the compositions
built on the filter (Progressive.variance, Progressive.preview and DeviceScene.render_denoised with
variance_guided=True) and its use: a filtered frame is nearer the converged frame than the noisy one."""
import numpy as np
import pytest

import scenes
import varfilter_ref as R
from test_filter import random_frames

F = np.float32
# every parameter explicit: the bit-level tests do not depend on the library's defaults
EXPLICIT = dict(sigma_luminance=3.0, sigma_normal=0.3, sigma_plane=0.05, albedo_floor=0.02, variance_floor=1e-6)
ORDER = ("color", "normal", "position", "depth")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def variance_frames(f, seed=0):
    """The variance frames a call is checked with: None, all known (the luminance's own scale), and a mix of known,
    NaN, +inf, negative and 0 (which is known)."""
    h, w = f["color"].shape[:2]
    rng = np.random.default_rng(77 + 1000 * h + w + seed)
    lum = R.lum(np.nan_to_num(f["color"]).astype(F))
    known = (lum * lum * rng.uniform(0.05, 0.5, (h, w))).astype(F)
    mixed = known.copy()
    kind = rng.integers(0, 6, (h, w))
    for k, v in ((1, np.nan), (2, np.inf), (3, -1.0), (4, 0.0)):
        mixed[kind == k] = v
    return {"none": None, "known": known, "mixed": mixed}


@pytest.fixture(scope="module")
def gpu():
    from vimg_amd import hip, varfilter
    hip.init(0)
    return varfilter


def _check_against_the_restatement(vf, f, iterations, sigma_luminance=EXPLICIT["sigma_luminance"]):
    import torch
    dev = {k: torch.from_numpy(v).cuda() for k, v in f.items()}
    for vname, var in variance_frames(f).items():
        for use_albedo in (True, False):
            p = dict(EXPLICIT, iterations=iterations, sigma_luminance=sigma_luminance)
            want, want_v = R.atrous(*(f[k] for k in ORDER), f["albedo"] if use_albedo else None, var, **p)
            got, got_v = vf.atrous(*(dev[k] for k in ORDER), albedo=dev["albedo"] if use_albedo else None,
                                   variance=None if var is None else torch.from_numpy(var).cuda(), **p)
            _same(got.cpu().numpy(), want)
            _same(got_v.cpu().numpy(), want_v)
    return want, want_v, p, var          # (the last combination: the mixed variance, no albedo)


SHAPES = [(1, 1), (3, 5), (17, 33), (6, 130), (64, 96)]


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 2, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_the_filter_is_the_restatement_bit_for_bit(gpu, shape, iterations):
    """[H, W] = 1 x 1, 3 x 5, 17 x 33 (no multiple of the 64 x 4 workgroup), 6 x 130 (three waves per row, a ragged tail
    in both axes, two workgroup rows) and 64 x 96; no variance frame, all known, and known / NaN / +inf / negative /
    0 mixed; with and without albedo; with misses, a NaN depth, a NaN colour.  Both outputs."""
    _check_against_the_restatement(gpu, random_frames(*shape), iterations)


@pytest.mark.gpu
def test_an_infinite_sigma_luminance_is_the_restatement_too(gpu):
    _check_against_the_restatement(gpu, random_frames(17, 33, seed=1), 2, sigma_luminance=np.inf)


@pytest.mark.gpu
def test_seven_iterations_at_17_x_33_where_every_off_centre_tap_leaves_the_image(gpu):
    """Step 64 in the last iteration (and 32 before it: 2 x 32 > 33): only the centre tap is left."""
    _check_against_the_restatement(gpu, random_frames(17, 33), 7)


@pytest.mark.gpu
def test_aliased_outputs_side_stream_numpy_inputs_and_a_callers_workspace(gpu):
    import torch
    f = random_frames(17, 33, seed=3)
    var = variance_frames(f, seed=3)["mixed"]
    p = dict(EXPLICIT, iterations=2)
    want, want_v = R.atrous(*(f[k] for k in ORDER), f["albedo"], var, **p)
    args = [f[k] for k in ORDER]
    # numpy in, numpy out
    got, got_v = gpu.atrous(*args, albedo=f["albedo"], variance=var, **p)
    assert isinstance(got, np.ndarray) and isinstance(got_v, np.ndarray)
    _same(got, want)
    _same(got_v, want_v)
    # out is the colour buffer, out_variance the variance buffer, and the workspace is the caller's (exactly the size asked for)
    dev = [torch.from_numpy(a).cuda() for a in args]
    alb, dvar = torch.from_numpy(f["albedo"]).cuda(), torch.from_numpy(var).cuda()
    work = torch.empty(gpu.workspace_bytes(33, 17) // 4, dtype=torch.float32, device="cuda")
    assert work.numel() * 4 == 64 * 17 * 33
    res, res_v = gpu.atrous(*dev, albedo=alb, variance=dvar, out=dev[0], out_variance=dvar, workspace=work, **p)
    assert res is dev[0] and res_v is dvar
    _same(res.cpu().numpy(), want)
    _same(res_v.cpu().numpy(), want_v)
    # a stream of the caller's
    dev[0], dvar = torch.from_numpy(f["color"]).cuda(), torch.from_numpy(var).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got, got_v = gpu.atrous(*dev, albedo=alb, variance=dvar, stream=side, **p)
    side.synchronize()
    _same(got.cpu().numpy(), want)
    _same(got_v.cpu().numpy(), want_v)
    # what the binding and the library refuse
    from vimg_amd import hip
    with pytest.raises(ValueError, match="varfilter normal"):
        gpu.atrous(dev[0], dev[1][:, :5].contiguous(), dev[2], dev[3], **p)
    with pytest.raises(ValueError, match="varfilter variance"):
        gpu.atrous(*dev, variance=dvar[:, :5].contiguous(), **p)
    with pytest.raises(hip.HipError, match="iterations must be 1..12"):
        gpu.atrous(*dev, **dict(p, iterations=13))
    with pytest.raises(hip.HipError, match="variance_floor must be > 0"):
        gpu.atrous(*dev, **dict(p, variance_floor=0.0))
    with pytest.raises(hip.HipError, match="the workspace has"):
        gpu.atrous(*dev, workspace=work[:-1], **p)


# ---- the accumulator's variance ------------------------------------------------------------------------------------------
def _error_from(variance, state):
    """err of vimg_hip.h from the variance: sqrt(V) / (|Y(S) / float(N)| + 1e-3f), in float32."""
    S, N = state["sum"].cpu().numpy(), state["count"].cpu().numpy()
    with np.errstate(all="ignore"):
        m = R.lum(S) / N.astype(F)
        return (np.sqrt(variance) / (np.abs(m) + F(1e-3))).astype(F)


@pytest.fixture(scope="module")
def cornell(gpu):
    from vimg_amd import hip
    s = scenes.json_scene("cornell_box_spheres.json", res=(64, 64))
    return s, hip.DeviceScene(s)


@pytest.mark.gpu
def test_the_accumulators_variance_is_its_error_bit_for_bit(gpu, cornell):
    """cornell_box_spheres 64 x 64, mis, increments 4 + 4 + 4, then a masked one: wherever K >= 2 the error is
    sqrt(variance) / (|mean luminance| + 1e-3) to the bit, and the variance is NaN while K < 2."""
    import torch
    s, dev = cornell
    acc = dev.progressive(s.default_params(integrator="mis", samples=1))
    acc.render(4)
    v = acc.variance()
    assert v.dtype == torch.float32 and tuple(v.shape) == (64, 64) and bool(torch.isnan(v).all())
    assert bool(torch.isinf(acc.error()).all())
    for _ in range(2):
        acc.render(4)
        v, st = acc.variance().cpu().numpy(), acc.state()
        assert (st["batches"] >= 2).all() and R.known(v).all() and (v > 0).any()
        _same(_error_from(v, st), acc.error().cpu().numpy())
        _same(v, R.variance(st["count"].cpu().numpy(), st["batches"].cpu().numpy(), st["m2"].cpu().numpy()))
        _same(gpu.variance(st["count"].cpu().numpy().astype(np.uint32), st["batches"].cpu().numpy().astype(np.uint32),
                           st["m2"].cpu().numpy()), v)
    # a masked increment on a fresh accumulator: half the pixels at K = 2, the others at K = 1
    acc.reset()
    acc.render(4)
    mask = np.zeros((64, 64), np.uint8)
    mask[:, ::2] = 1
    acc.render(4, mask=mask)
    v, st = acc.variance().cpu().numpy(), acc.state()
    assert np.array_equal(st["batches"].cpu().numpy(), 1 + mask)
    assert np.isnan(v[mask == 0]).all() and R.known(v[mask == 1]).all()
    err = acc.error().cpu().numpy()
    assert np.isinf(err[mask == 0]).all()
    _same(_error_from(v, st)[mask == 1], err[mask == 1])
    acc.close()


# ---- rendered frames, the compositions, the use ---------------------------------------------------------------------------
RENDERED = ("cornell_box_spheres.json", "disney_spheres.json")


@pytest.mark.gpu
@pytest.mark.parametrize("name", RENDERED)
def test_rendered_frames_with_the_accumulators_variance_filter_to_the_restatements_bits(gpu, name):
    from vimg_amd import hip
    s = scenes.json_scene(name, res=(64, 64))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    g = dev.render_features(p, gpu.GUIDES)
    acc = dev.progressive(p)
    for _ in range(4):
        noisy = acc.render(4)
    var = acc.variance()
    assert R.known(var.cpu().numpy()).all()
    host = {k: v.cpu().numpy() for k, v in g.items()}
    assert (host["depth"][..., 0] > 0).any()
    q = {k: getattr(gpu.params(), k) for k in ("iterations",) + gpu.FLOATS}          # the library's defaults
    want, want_v = R.atrous(noisy.cpu().numpy(), host["normal"], host["position"], host["depth"], host["albedo"], var.cpu().numpy(), **q)
    got, got_v = gpu.atrous(noisy, g["normal"], g["position"], g["depth"], albedo=g["albedo"], variance=var)
    _same(got.cpu().numpy(), want)
    _same(got_v.cpu().numpy(), want_v)
    assert not np.array_equal(_bits(want), _bits(noisy.cpu().numpy()))
    acc.close()


@pytest.mark.gpu
def test_preview_and_render_denoised_are_the_manual_composition(gpu, cornell):
    import torch
    from vimg_amd import filter as flt
    s, dev = cornell
    p = s.default_params(integrator="mis", samples=4)
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    g = dev.render_features(p, gpu.GUIDES)
    args = lambda: (g["normal"], g["position"], g["depth"])
    q = dict(EXPLICIT, iterations=3)
    acc, twin = dev.progressive(p), dev.progressive(p)
    # the first preview: K = 1, every variance unknown; the second: K = 2
    for k in (1, 2):
        got = acc.preview(4, variance_guided=True, **q)
        noisy = twin.render(4)
        var = twin.variance()
        assert bool(torch.isnan(var).all()) == (k == 1)
        man, _ = gpu.atrous(noisy, *args(), albedo=g["albedo"], variance=var, **q)
        assert same(got, man) and not same(got, noisy)
    # with the library's defaults, into the caller's buffer
    buf = torch.empty_like(noisy)
    got = acc.preview(4, variance_guided=True, out=buf)
    noisy = twin.render(4)
    man, _ = gpu.atrous(noisy, *args(), albedo=g["albedo"], variance=twin.variance())
    assert got is buf and same(got, man)
    # the accumulator kept the unfiltered sums: its next render is the one-shot render's bits
    assert same(acc.render(4), dev.render(s.default_params(integrator="mis", samples=16), stats=False))
    # the default preview is the fixed filter's, as before
    got = acc.preview(4)
    twin.render(4)
    noisy = twin.render(4)
    assert same(got, flt.atrous(noisy, *args(), albedo=g["albedo"]))
    acc.close()
    twin.close()
    # a one-shot render has no variance: every pixel's is estimated
    noisy = dev.render(p, stats=False)
    man, _ = gpu.atrous(noisy, *args(), albedo=g["albedo"], **q)
    assert same(dev.render_denoised(p, variance_guided=True, **q), man)
    assert same(dev.render_denoised(p), flt.atrous(noisy, *args(), albedo=g["albedo"]))


@pytest.mark.gpu
def test_filtered_frames_are_nearer_the_converged_frame_than_the_noisy_ones(gpu, cornell):
    """cornell_box_spheres 64 x 64 against mis at 1024 spp, library defaults, e = mean((x - ref)^2 / (ref^2 + 0.01)):
    the 4 spp frame (one increment, every variance estimated) and the 16 spp frame (four increments, the accumulator's
    variance) both come out strictly nearer than they went in.  Measured: 4 spp 0.0724 noisy, 0.0207
    fixed filter, 0.0183 variance-guided; 16 spp 0.0194, 0.0166, 0.0063."""
    from vimg_amd import filter as flt
    s, dev = cornell
    p = s.default_params(integrator="mis", samples=4)
    ref = dev.render(s.default_params(integrator="mis", samples=1024), stats=False).cpu().numpy().astype(np.float64)
    g = dev.render_features(p, gpu.GUIDES)
    rse = lambda x: float((((x.cpu().numpy() - ref) ** 2) / (ref ** 2 + 0.01)).mean())
    acc = dev.progressive(p)
    for spp in (4, 16):
        while acc.samples < spp:
            noisy = acc.render(4)
        guided, _ = gpu.atrous(noisy, g["normal"], g["position"], g["depth"], albedo=g["albedo"], variance=acc.variance())
        fixed = flt.atrous(noisy, g["normal"], g["position"], g["depth"], albedo=g["albedo"])
        e = dict(noisy=rse(noisy), fixed=rse(fixed), guided=rse(guided))
        print(f"{spp} spp: " + ", ".join(f"{k} {v:.5f}" for k, v in e.items()))
        assert np.isfinite(guided.cpu().numpy()).all() and e["guided"] < e["noisy"], (spp, e)
    acc.close()
