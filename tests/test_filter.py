"""The a-trous filter on the GPU (libvimg_filter.so, include/vimg_filter.h): vimg_filter_atrous
against the numpy restatement of its contract (tests/atrous_ref.py) BIT FOR BIT - on random frames that hold every
special pixel the contract names, and on rendered frames with their feature frames - then the compositions built on
it (DeviceScene.render_denoised, Progressive.preview, the command line's -n) and its use: a 4 spp frame filtered
with the defaults is nearer the converged frame than the noisy one."""
import json
import os
import subprocess

import numpy as np
import pytest

import atrous_ref as R
import scenes

F = np.float32
# every parameter explicit: the bit-level tests do not depend on the library's defaults
EXPLICIT = dict(sigma_normal=0.3, sigma_plane=0.05, albedo_floor=0.02)
SIGMA_COLORS = (np.inf, 1.5)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def random_frames(h, w, seed=0):
    """Frames with structure (neighbours do match: smooth normals, positions near a plane, colours within reach of a
    finite sigma_color) and, from 3 x 5 on, every special pixel: misses (depth 0, with guides 0), a negative and a
    NaN depth, a NaN colour, a NaN normal, albedo at 0, below the floor and NaN."""
    rng = np.random.default_rng(1000 * h + w + seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    n = np.stack([0.3 * np.sin(xx / 5.0), 0.3 * np.cos(yy / 7.0), np.ones_like(xx)], -1) + 0.05 * rng.normal(size=(h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    z = 4.0 + 0.02 * xx + 0.03 * yy + 0.01 * rng.normal(size=(h, w))
    P = np.stack([0.05 * xx, 0.05 * yy, -z], -1) + 0.002 * rng.normal(size=(h, w, 3))
    albedo = rng.uniform(0.05, 0.9, (h, w, 3))
    color = albedo * rng.gamma(2.0, 0.5, (h, w, 3))
    f = {k: np.ascontiguousarray(v, dtype=F) for k, v in dict(color=color, normal=n, position=P, albedo=albedo,
                                                             depth=np.repeat(z[..., None], 3, -1)).items()}
    if h * w >= 15:
        cells = rng.permutation(h * w)
        at = lambda i: np.unravel_index(cells[i], (h, w))
        for i in range(max(1, h * w // 12)):              # misses: a twelfth of the frame
            for k in ("normal", "position", "depth", "albedo"):
                f[k][at(i)] = 0
        m = max(1, h * w // 12)
        f["depth"][at(m)] = -1.0
        f["depth"][at(m + 1)] = np.nan
        f["color"][at(m + 2)][1] = np.nan
        f["normal"][at(m + 3)][0] = np.nan
        f["albedo"][at(m + 4)] = (0.0, 0.01, np.nan)
        f["albedo"][at(m + 5)] = 0.0199
        f["depth"][at(m + 6)][1:] = (0.0, np.nan)        # only the first component is read: this pixel is live
    return f


@pytest.fixture(scope="module")
def gpu():
    from vimg_amd import filter as flt, hip
    hip.init(0)
    return flt


def _check_against_the_restatement(flt, f, iterations):
    import torch
    dev = {k: torch.from_numpy(v).cuda() for k, v in f.items()}
    for use_albedo in (True, False):
        for sc in SIGMA_COLORS:
            p = dict(EXPLICIT, iterations=iterations, sigma_color=sc)
            want = R.atrous(f["color"], f["normal"], f["position"], f["depth"], f["albedo"] if use_albedo else None, **p)
            got = flt.atrous(dev["color"], dev["normal"], dev["position"], dev["depth"],
                             albedo=dev["albedo"] if use_albedo else None, **p)
            _same(got.cpu().numpy(), want)
    return want, p          # (the last combination: no albedo, finite sigma_color)


SHAPES = [(1, 1), (3, 5), (17, 33), (64, 96)]


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 2, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_the_filter_is_the_restatement_bit_for_bit(gpu, shape, iterations):
    """[H, W] = 1 x 1, 3 x 5, 17 x 33 (no multiple of the 64 x 4 workgroup, one workgroup wide) and 64 x 96 (two
    waves wide, sixteen workgroups high); with and without albedo; sigma_color +inf and finite."""
    _check_against_the_restatement(gpu, random_frames(*shape), iterations)


@pytest.mark.gpu
def test_seven_iterations_at_17_x_33_where_every_off_centre_tap_leaves_the_image(gpu):
    """Step 64 in the last iteration (and 32 before it: 2 x 32 > 33): only the centre tap is left."""
    _check_against_the_restatement(gpu, random_frames(17, 33), 7)


@pytest.mark.gpu
def test_aliased_output_side_stream_numpy_inputs_and_a_callers_workspace(gpu):
    import torch
    f = random_frames(17, 33, seed=3)
    p = dict(EXPLICIT, iterations=2, sigma_color=1.5)
    want = R.atrous(f["color"], f["normal"], f["position"], f["depth"], f["albedo"], **p)
    args = [f[k] for k in ("color", "normal", "position", "depth")]
    # numpy in, numpy out
    got = gpu.atrous(*args, albedo=f["albedo"], **p)
    assert isinstance(got, np.ndarray)
    _same(got, want)
    # out is the colour buffer itself, and a workspace of the caller's (float32, exactly the size asked for)
    dev = [torch.from_numpy(a).cuda() for a in args]
    alb = torch.from_numpy(f["albedo"]).cuda()
    work = torch.empty(gpu.atrous_workspace_bytes(33, 17) // 4, dtype=torch.float32, device="cuda")
    assert work.numel() * 4 == 64 * 17 * 33
    res = gpu.atrous(*dev, albedo=alb, out=dev[0], workspace=work, **p)
    assert res is dev[0]
    _same(res.cpu().numpy(), want)
    # a stream of the caller's
    dev[0] = torch.from_numpy(f["color"]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = gpu.atrous(*dev, albedo=alb, stream=side, **p)
    side.synchronize()
    _same(got.cpu().numpy(), want)
    # what the binding and the library refuse
    from vimg_amd import hip
    with pytest.raises(ValueError, match="atrous normal"):
        gpu.atrous(dev[0], dev[1][:, :5].contiguous(), dev[2], dev[3], **p)
    with pytest.raises(hip.HipError, match="iterations must be 1..12"):
        gpu.atrous(*dev, **dict(p, iterations=13))
    with pytest.raises(hip.HipError, match="the workspace has"):
        gpu.atrous(*dev, workspace=work[:-1], **p)


# ---- rendered frames ------------------------------------------------------------------------------------------------
RENDERED = {"cornell": lambda: scenes.json_scene("cornell_box_spheres.json", res=(64, 64)),
            "feature": lambda: scenes.feature_scene(res=(96, 64))}


@pytest.fixture(scope="module")
def rendered(gpu):
    """name -> (scene, resident scene, 4 spp mis parameters, noisy frame, the four feature frames), rendered once."""
    from vimg_amd import hip
    out = {}
    for name, make in RENDERED.items():
        s = make()
        dev = hip.DeviceScene(s)
        p = s.default_params(integrator="mis", samples=4)
        noisy = dev.render(p, stats=False)
        guides = dev.render_features(p, gpu.GUIDES)
        out[name] = (s, dev, p, noisy, guides)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RENDERED))
def test_rendered_frames_filter_to_the_restatements_bits(gpu, rendered, name):
    s, dev, p, noisy, g = rendered[name]
    w, h = s.resolution
    assert tuple(noisy.shape) == (h, w, 3)
    host = {k: v.cpu().numpy() for k, v in g.items()}
    live = host["depth"][..., 0] > 0
    assert live.any()
    for sc in SIGMA_COLORS:
        q = dict(EXPLICIT, iterations=5, sigma_color=sc)
        want = R.atrous(noisy.cpu().numpy(), host["normal"], host["position"], host["depth"], host["albedo"], **q)
        got = gpu.atrous(noisy, g["normal"], g["position"], g["depth"], albedo=g["albedo"], **q)
        _same(got.cpu().numpy(), want)
        assert not np.array_equal(_bits(want), _bits(noisy.cpu().numpy()))


@pytest.mark.gpu
def test_render_denoised_and_preview_are_the_manual_composition(gpu, rendered):
    import torch
    s, dev, p, noisy, g = rendered["cornell"]
    q = dict(EXPLICIT, iterations=3, sigma_color=np.inf)
    want = gpu.atrous(noisy, g["normal"], g["position"], g["depth"], albedo=g["albedo"], **q)
    assert torch.equal(dev.render_denoised(p, **q).view(torch.int32), want.view(torch.int32))
    # with the library's defaults too
    dflt = gpu.atrous(noisy, g["normal"], g["position"], g["depth"], albedo=g["albedo"])
    assert torch.equal(dev.render_denoised(p).view(torch.int32), dflt.view(torch.int32))
    # preview: render(n) + the filter on guides rendered once (at feature_samples) and kept
    acc = dev.progressive(p)
    pg = s.default_params(integrator="mis", samples=2)
    g2 = dev.render_features(pg, gpu.GUIDES)
    first = acc.preview(3, feature_samples=2, **q)
    one_shot3 = dev.render(s.default_params(integrator="mis", samples=3), stats=False)
    man = gpu.atrous(one_shot3, g2["normal"], g2["position"], g2["depth"], albedo=g2["albedo"], **q)
    assert torch.equal(first.view(torch.int32), man.view(torch.int32))
    kept = acc._guides[1]
    second = acc.preview(1, feature_samples=2, **q)
    assert acc._guides[1] is kept and acc.samples == 4
    man = gpu.atrous(noisy, g2["normal"], g2["position"], g2["depth"], albedo=g2["albedo"], **q)
    assert torch.equal(second.view(torch.int32), man.view(torch.int32))
    # the accumulator kept the unfiltered sums: its next render is the one-shot render's bits
    nxt = acc.render(4)
    assert torch.equal(nxt.view(torch.int32), dev.render(s.default_params(integrator="mis", samples=8), stats=False).view(torch.int32))
    # an edit of the scene renders the guides again
    dev.set_camera(s.view.contents.camera)
    acc.reset()
    acc.preview(4, feature_samples=2, **q)
    assert acc._guides[1] is not kept
    acc.close()
    with pytest.raises(ValueError, match="whole frames"):
        dev.render_denoised(s.default_params(samples=4, tile_world=2, tile_rank=0))


@pytest.mark.gpu
def test_a_filtered_4_spp_frame_is_nearer_the_converged_frame_than_the_noisy_one(gpu, rendered):
    """cornell_box_spheres 64 x 64, mis at 4 spp filtered with the library's defaults, against mis at 1024 spp: the
    relative squared error mean((x - ref)^2 / (ref^2 + 0.01)) falls.  (Measured ratio: DESIGN.md 4.18.)"""
    s, dev, p, noisy, g = rendered["cornell"]
    ref = dev.render(s.default_params(integrator="mis", samples=1024), stats=False).cpu().numpy().astype(np.float64)
    out = gpu.atrous(noisy, g["normal"], g["position"], g["depth"], albedo=g["albedo"]).cpu().numpy()
    rse = lambda x: float((((x - ref) ** 2) / (ref ** 2 + 0.01)).mean())
    before, after = rse(noisy.cpu().numpy()), rse(out)
    print(f"relative squared error: noisy {before:.5f}, filtered {after:.5f}, ratio {before / after:.2f}")
    assert np.isfinite(out).all() and after < before


@pytest.mark.gpu
def test_cli_writes_the_filtered_frame(gpu, tmp_path):
    """vimg-amd -n 5 -s 4: the PNG is post_rgb8(render_denoised(...)), not the plain run's; with -p 2 the final file
    is the same bytes."""
    import vimg_amd
    from vimg_amd import hip, host
    exe = os.path.join(vimg_amd.abi.PKG_DIR, "bin", "vimg-amd")
    with open(os.path.join(scenes.SCENES, "cornell_box_spheres.json")) as f:
        d = json.load(f)
    d["camera"]["resolution"] = [64, 64]
    scene = tmp_path / "cornell_64.json"
    scene.write_text(json.dumps(d))
    runs = {"plain": [], "filtered": ["-n", "5"], "progressive": ["-n", "5", "-p", "2"]}
    for name, extra in runs.items():
        r = subprocess.run([exe, "-f", str(scene), "-s", "4", "-b", "1", "-o", str(tmp_path / f"{name}.png")] + extra,
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
    s = scenes.json_scene("cornell_box_spheres.json", res=(64, 64))
    dev = hip.DeviceScene(s)
    img = dev.render_denoised(s.default_params(samples=4), iterations=5)
    host.write_png(tmp_path / "want.png", hip.post_rgb8(img, 0).cpu().numpy())
    want = (tmp_path / "want.png").read_bytes()
    assert (tmp_path / "filtered.png").read_bytes() == want
    assert (tmp_path / "progressive.png").read_bytes() == want
    assert (tmp_path / "plain.png").read_bytes() != want
