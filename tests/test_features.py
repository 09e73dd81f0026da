"""The first-hit feature integrators (albedo, normal, depth, position, uv, coverage; include/vimg_hip.h beside
vimg_hip_render).  A numpy sampler - the oracle's PCG and R2 jitter, the library's camera_rays and
trace_rays - is first pinned to s_normal, which the oracle pins; the features are then bit for bit that sampler's
composition of the query results, albedo the host scene's colour tables (image textures: the oracle's BSDF
probe), and the new integrators reach everything an integrator reaches: progressive and masked increments, shards,
trace_pixel, generation checks, statistics, render_features."""
import numpy as np
import pytest

import oracle_lib as O
import scenes
from test_scene_update_host import deformed

pytestmark = pytest.mark.gpu

F32 = np.float32
MAX_SPP = 5
SCENES = {
    "feature": lambda: scenes.feature_scene(res=(96, 64)),                           # TEX build, thin lens, every material
    "cornell": lambda: scenes.json_scene("cornell_box_spheres.json", res=(64, 64)),  # untextured build
    "40x24": lambda: scenes.json_scene("disney_spheres.json", res=(40, 24)),
    "ragged": lambda: scenes.json_scene("cornell_box_spheres.json", res=(42, 27)),   # edge tiles 2 and 3 pixels wide
}
_cache = {}


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


class _Sampled:
    """One scene, resident, with the first MAX_SPP samples of every pixel traced through the ray queries once:
    arrays [H, W, MAX_SPP, ...] in the image's layout (row 0 = top)."""

    def __init__(self, name):
        from vimg_amd import hip
        self.s = s = SCENES[name]()
        self.dev = hip.DeviceScene(s)
        w, h = s.resolution
        smp = np.empty((h, w, MAX_SPP, 4), dtype=F32)
        for py in range(h):
            for px in range(w):
                rng = O.Pcg(px + (h - 1 - py) * w)          # the pixel's stream: seeded with the image index
                for k in range(MAX_SPP):
                    ox, oy = O.r2(px + py + k)
                    rand2 = rng.rand_float()                # rand2 before rand1
                    rand1 = rng.rand_float()
                    smp[h - 1 - py, px, k] = (F32(px) + F32(ox), F32(py) + F32(oy), rand1, rand2)
        self.rays = self.dev.camera_rays(smp.reshape(-1, 4))
        r = self.dev.trace_rays(self.rays, info=True)
        shp = (h, w, MAX_SPP)
        self.hit = (r.prim != -1).reshape(shp)
        self.t, self.mat = r.t.reshape(shp), r.mat.reshape(shp)
        self.p, self.ns, self.uv = r.p.reshape(shp + (3,)), r.ns.reshape(shp + (3,)), r.uv.reshape(shp + (2,))
        self.dir = self.rays[:, 4:7].reshape(shp + (3,))

    def compose(self, values, n):
        """The pixel a kernel makes of per-sample values [H, W, MAX_SPP, 3]: 0 on a miss, the float32 sum of the
        first n in sample order, one division."""
        v = np.where(self.hit[..., None], values, F32(0)).astype(F32)
        acc = np.zeros(v.shape[:2] + (3,), dtype=F32)
        for k in range(n):
            acc = acc + v[:, :, k]
        return acc / F32(n)

    def feature(self, name):
        z = np.zeros_like(self.t)
        return {"normal": self.ns, "depth": np.stack([self.t] * 3, -1), "position": self.p,
                "uv": np.stack([self.uv[..., 0], self.uv[..., 1], z], -1),
                "coverage": np.ones_like(self.p)}[name]

    def render(self, integrator, n, **kw):
        return self.dev.render(self.s.default_params(integrator=integrator, samples=n, **kw), stats=False)


def _sampled(name):
    if name not in _cache:
        _cache[name] = _Sampled(name)
    return _cache[name]


# ---- 1. the harness is the normal integrator's sampler -----------------------------------------------------------
@pytest.mark.parametrize("scene", ["feature", "cornell"])
def test_the_sampler_reproduces_s_normal_bit_for_bit(scene):
    """(ns + 1) / 2 on a hit, the sky gradient of the ray's direction on a miss (render_kernels.h, the normal
    integrators' block; reference src/integrators/normals.cpp): 4 spp of s_normal, every pixel, every bit."""
    q = _sampled(scene)
    on_hit = (q.ns + F32(1)) / F32(2)
    d = q.dir
    unit = d * (F32(1) / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]))[..., None]
    a = (0.5 * (unit[..., 1].astype(np.float64) + 1.0)).astype(F32)[..., None]      # float a = 0.5 * (y + 1.0)
    sky = (F32(1) - a) * np.ones(3, F32) + a * np.array([0.5, 0.7, 1.0], F32)
    v = np.where(q.hit[..., None], on_hit, sky).astype(F32)
    acc = np.zeros(v.shape[:2] + (3,), dtype=F32)
    for k in range(4):
        acc = acc + v[:, :, k]
    assert q.hit.any() and (scene != "cornell" or not q.hit.all())      # (cornell: a tenth of the samples see the sky)
    assert np.array_equal(_bits(acc / F32(4)), _bits(q.render("s_normal", 4)))


# ---- 2. the features are the queries' bits -------------------------------------------------------------------------
@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("name", ["normal", "depth", "position", "uv", "coverage"])
def test_features_are_the_composition_of_the_query_results(scene, name):
    q = _sampled(scene)
    for n in (1, 4, 5):
        got = q.render(name, n).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(q.compose(q.feature(name), n))), (scene, name, n)
        if name == "coverage":
            hits = got * F32(n)
            assert np.array_equal(hits, np.round(hits)) and np.array_equal(hits[..., 0], q.hit[:, :, :n].sum(-1))


# ---- 3. albedo -------------------------------------------------------------------------------------------------------
def _table_albedo(q):
    """(per-sample colour [H, W, MAX_SPP, 3], known [H, W, MAX_SPP]) from the host scene's material and texture
    tables: constant and checkerboard base colours, Dielectric 1, DiffuseLight its emission; image textures unknown."""
    from vimg_amd import abi
    mats, texs = q.s.materials(), q.s.textures()
    col = np.zeros(q.p.shape, dtype=F32)
    known = ~q.hit
    for i, m in enumerate(mats):
        sel = q.hit & (q.mat == i)
        if m.type == abi.MAT_DIELECTRIC:
            col[sel], known = F32(1), known | sel
        elif m.type == abi.MAT_DIFFUSE_LIGHT:
            col[sel], known = np.array(list(m.emit), F32), known | sel
        else:
            t = texs[m.tex]
            a, b = np.array(list(t.col_a), F32), np.array(list(t.col_b), F32)
            if t.type == abi.TEX_CONST:
                col[sel], known = a, known | sel
            elif t.type == abi.TEX_CHECKER:
                # reference include/texture/texture_RGB.h:73-79: uint32_t u_board = std::floor(uv[0] * width), v_board
                # likewise; (u_board + v_board) % 2 == 0 ? col_a : col_b
                ub = np.floor(q.uv[..., 0] * F32(t.width)).astype(np.int64) & 0xFFFFFFFF
                vb = np.floor(q.uv[..., 1] * F32(t.height)).astype(np.int64) & 0xFFFFFFFF
                even = (((ub + vb) & 0xFFFFFFFF) % 2 == 0)[..., None]
                col[sel], known = np.where(even, a, b)[sel], known | sel
    return col, known


@pytest.mark.parametrize("scene", ["feature", "cornell", "ragged"])
def test_albedo_of_constant_and_checkerboard_colours_is_the_host_tables_bits(scene):
    from vimg_amd import abi
    q = _sampled(scene)
    col, known = _table_albedo(q)
    seen = {int(q.s.materials()[i].type) for i in np.unique(q.mat[q.hit])}
    # the camera sees every material type between the scenes: the glass sphere here, the emitter in the box
    assert seen == ({abi.MAT_LAMBERTIAN, abi.MAT_DIELECTRIC, abi.MAT_PRINCIPLED} if scene == "feature"
                    else {abi.MAT_LAMBERTIAN, abi.MAT_DIFFUSE_LIGHT})
    for n in (1, 4, 5):
        px = known[:, :, :n].all(-1)                     # pixels none of whose samples read an image texture
        assert px.mean() > 0.5
        got = q.render("albedo", n).cpu().numpy()
        assert np.array_equal(_bits(got[px]), _bits(q.compose(col, n)[px])), (scene, n)


def test_albedo_of_an_image_texture_is_the_colour_in_the_oracles_bsdf():
    """Lambertian hits on the mip-mapped image texture of feature_scene at 1 spp.  Lambertian::eval_pdf_pair gives
    f = colour * c with c = float(max(0, dot(wo, ns)) / pi) (src/material/lambertian.cpp:47-54), so with wo = ns the
    colour is f / c: PROBE_BSDF_EVAL of the oracle for the same ray and the cone of the first vertex,
    {|spread * distance|, spread} - the flat mesh has no curvature, which the oracle's hit records are asked.  Tolerance: the probes' (rtol 2e-5, atol 1e-6,
    test_probes_bsdf_and_lights); the recovery f / c adds two roundings, 2^-23 relative, far inside it."""
    from vimg_amd import abi
    q = _sampled("feature")
    mats, texs = q.s.materials(), q.s.textures()
    img = [i for i, m in enumerate(mats) if m.type == abi.MAT_LAMBERTIAN and texs[m.tex].type == abi.TEX_IMAGE]
    assert len(img) == 1
    sel = q.hit[:, :, 0] & (q.mat[:, :, 0] == img[0])
    assert sel.sum() >= 32
    h, w = sel.shape
    rays = q.rays.reshape(h, w, MAX_SPP, 8)[:, :, 0][sel]
    o, d = rays[:, 0:3], rays[:, 4:7]
    p, ns = q.p[:, :, 0][sel], q.ns[:, :, 0][sel]
    # (PROBE_CLOSEST_HIT, column 25: the mean curvature behind the surface term of the cone)
    assert np.all(O.probe(q.s, O.PROBE_CLOSEST_HIT, np.concatenate([o, d], 1))[:, 25] == 0)
    spread = O.probe(q.s, O.PROBE_CAMERA_RAY, np.array([[1.0, 1.0, 0.5, 0.5]], F32))[0, 7]
    e = o - p
    dist = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    cone = np.stack([np.abs(spread * dist + F32(0)), np.full_like(dist, spread)], 1)
    probe_in = np.concatenate([o, d, ns, cone, np.zeros((len(o), 1), F32)], 1).astype(F32)
    ref = O.probe(q.s, O.PROBE_BSDF_EVAL, probe_in)
    assert np.all(ref[:, 0] == 1)
    dot = (ns[:, 0] * ns[:, 0] + ns[:, 1] * ns[:, 1]) + ns[:, 2] * ns[:, 2]
    c = (np.maximum(F32(0), dot).astype(np.float64) / np.pi).astype(F32)
    want = ref[:, 1:4] / c[:, None]
    got = q.render("albedo", 1).cpu().numpy()[sel]
    err = np.abs(got - want) - (1e-6 + 2e-5 * np.abs(want))
    print(f"image-texture albedo: {sel.sum()} pixels, max |got - want| {np.abs(got - want).max():.3e}, "
          f"worst margin to the tolerance {err.max():.3e}")
    assert np.allclose(got, want, rtol=2e-5, atol=1e-6)
    assert got.std() > 0.01        # a texture, not a constant


# ---- 4. reach ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["feature", "ragged"])
@pytest.mark.parametrize("name", ["albedo", "depth"])
def test_progressive_masked_sharded_and_single_pixel_renders_equal_the_one_shot(scene, name):
    import torch
    q = _sampled(scene)
    d, s = q.dev, q.s
    w, h = s.resolution
    shot = {n: q.render(name, n) for n in (1, 2, 4, 5, 8)}
    p = s.default_params(integrator=name, samples=1)
    # increments 1 + 3 + 4
    acc = d.progressive(p)
    for inc, total in ((1, 1), (3, 4), (4, 8)):
        assert torch.equal(acc.render(inc), shot[total]), (scene, name, total)
    # a masked increment on a checkerboard mask
    acc.reset()
    acc.render(2)
    yy, xx = np.mgrid[0:h, 0:w]
    mask = ((yy + xx) % 2 == 0)
    img = acc.render(3, mask=mask.astype(np.uint8)).cpu().numpy()
    assert np.array_equal(_bits(img[~mask]), _bits(shot[2])[~mask]), (scene, name, "unselected")
    assert np.array_equal(_bits(img[mask]), _bits(shot[5])[mask]), (scene, name, "selected")
    assert np.array_equal(acc.counts().cpu().numpy(), np.where(mask, 5, 2))
    err, (sel, active) = acc.error(), acc.select(0.0, 8)
    assert err.shape == (h, w) and sel.shape == (h, w) and 0 < active <= h * w
    acc.close()
    # after update_geometry (on a device scene of its own: the shared one stays as it was sampled) the accumulator
    # refuses until it is reset, and then renders the moved scene
    from vimg_amd import hip
    d2 = hip.DeviceScene(s)
    acc = d2.progressive(p)
    assert torch.equal(acc.render(2), shot[2])
    v, nrm, sp = deformed(s, 3)
    d2.update_geometry(vertices=v if len(v) else None, spheres=sp if len(sp) else None)
    with pytest.raises(hip.HipError, match="reset"):
        acc.render(2)
    acc.reset()
    moved = acc.render(4)
    assert torch.equal(moved, d2.render(s.default_params(integrator=name, samples=4), stats=False))
    assert not torch.equal(moved, shot[4])
    acc.close()
    d2.close()
    # 3 shards, assembled
    world = 3
    stride = max(d.shard_pixels(s.default_params(tile_rank=r, tile_world=world)) for r in range(world))
    gathered = torch.zeros((world, stride, 3), dtype=torch.float32, device="cuda")
    for r in range(world):
        slab = d.render(s.default_params(integrator=name, samples=4, tile_rank=r, tile_world=world), stats=False)
        gathered[r, :slab.shape[0]] = slab
    assert torch.equal(d.assemble_shards(gathered, world, stride), shot[4]), (scene, name, "shards")
    # trace_pixel
    full = shot[4].cpu().numpy()
    for (x, y) in ((0, 0), (w // 2, h // 3), (w - 1, h - 1)):
        one = d.trace_pixel(s.default_params(integrator=name, samples=4), x, y)
        assert np.array_equal(_bits(one), _bits(full[h - 1 - y, x])), (scene, name, x, y)


# ---- 5. statistics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["feature", "ragged"])
def test_statistics_are_those_of_the_normal_integrators_rays(scene):
    q = _sampled(scene)
    w, h = q.s.resolution
    _, st = q.dev.render(q.s.default_params(integrator="depth", samples=4))
    _, ref = q.dev.render(q.s.default_params(integrator="s_normal", samples=4))
    assert st.paths == st.closest_rays == w * h * 4 and st.shadow_rays == 0 and st.nan_samples == 0
    assert st.internal_visits > 0 and st.prim_tests > 0
    assert st.as_dict() == ref.as_dict()


# ---- 6. nothing else moved ---------------------------------------------------------------------------------------------
def test_feature_launches_leave_the_renderer_alone_and_unknown_integrators_are_refused():
    from vimg_amd import abi, hip
    q = _sampled("feature")
    p = q.s.default_params(integrator="mis", samples=4)
    before = q.dev.render(p, stats=False).cpu().numpy()
    acc = q.dev.progressive(p)
    acc.render(2)
    for name in abi.FEATURES:
        q.render(name, 3)
        q.render(name, 2, tile_rank=1, tile_world=2)
    assert np.array_equal(_bits(q.dev.render(p, stats=False)), _bits(before))
    assert np.array_equal(_bits(acc.render(2)), _bits(before))
    acc.close()
    assert q.dev.kernel_for(q.s.default_params(integrator="depth")) == "feature_kernel<true>"
    assert _sampled("cornell").dev.kernel_for(q.s.default_params(integrator="albedo")) == "feature_kernel<false>"
    assert q.dev.kernel_for(p) == q.dev.kernel
    with pytest.raises(hip.HipError, match="unknown integrator"):
        q.dev.render(q.s.default_params(integrator=10))
    # the scheduler option is not read: the lane-bound library gives the same features
    lane = hip.DeviceScene(q.s, scheduler="lane")
    for name in ("albedo", "uv"):
        pf = q.s.default_params(integrator=name, samples=3)
        assert np.array_equal(_bits(lane.render(pf, stats=False)), _bits(q.dev.render(pf, stats=False)))
    lane.close()


# ---- 7. render_features ------------------------------------------------------------------------------------------------
def test_render_features_is_the_separate_renders_on_any_stream():
    """The dict equals the separate renders, for the default names, a caller's buffer, a shard, and a launch asked
    onto a side stream.  (That the stream is the one that runs the launch is _Launch's business, which
    render_features reaches through render; tests/test_stream_rule.py checks it there.  Here only the results count.)"""
    import torch
    q = _sampled("feature")
    p = q.s.default_params(integrator="mis", samples=4)
    want = {n: q.render(n, 4) for n in ("albedo", "normal", "depth", "uv")}
    got = q.dev.render_features(p)
    assert sorted(got) == ["albedo", "depth", "normal"]
    for n, t in got.items():
        assert t.shape == (64, 96, 3) and t.dtype == torch.float32 and torch.equal(t, want[n]), n
    side = torch.cuda.Stream()
    mine = torch.full((64, 96, 3), -1.0, device="cuda")
    got = q.dev.render_features(p, features=("uv", "depth"), out={"uv": mine}, stream=side)
    side.synchronize()
    assert got["uv"] is mine and torch.equal(mine, want["uv"]) and torch.equal(got["depth"], want["depth"])
    shard = q.s.default_params(samples=4, tile_rank=1, tile_world=3)
    slab = q.dev.render_features(shard, features=("depth",))["depth"]
    assert torch.equal(slab, q.render("depth", 4, tile_rank=1, tile_world=3))
    with pytest.raises(ValueError, match="render_features"):
        q.dev.render_features(p, features=("beauty",))
    with pytest.raises(ValueError, match="out must be"):
        q.dev.render_features(p, features=("depth",), out={"depth": torch.zeros((64, 96), device="cuda")})


# ---- 8. the command line ------------------------------------------------------------------------------------------------
def test_cli_writes_the_three_feature_images_beside_the_picture(tmp_path):
    """vimg-amd -a prefix: prefix_albedo.png, prefix_normal.png as (n + 1) / 2 and prefix_depth.png divided by the
    image's largest depth, each through the clamp tonemapper - the bytes of the same mapping of dev.render's frames."""
    import json
    import os
    import subprocess
    import vimg_amd
    from vimg_amd import host
    exe = os.path.join(vimg_amd.abi.PKG_DIR, "bin", "vimg-amd")
    with open(os.path.join(scenes.SCENES, "cornell_box_spheres.json")) as f:
        d = json.load(f)
    d["camera"]["resolution"] = [64, 64]
    scene = tmp_path / "cornell_64.json"
    scene.write_text(json.dumps(d))
    r = subprocess.run([exe, "-f", str(scene), "-s", "3", "-b", "1", "-a", str(tmp_path / "aux"), "-o", str(tmp_path / "img.png")],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    q = _sampled("cornell")
    want = {n: q.render(n, 3).cpu().numpy() for n in ("albedo", "normal", "depth")}
    want["normal"] = (want["normal"] + F32(1)) / F32(2)
    want["depth"] = want["depth"] / want["depth"].max()
    for n, img in want.items():
        ref = tmp_path / f"ref_{n}.png"
        host.write_png(ref, host.tonemap_to_rgb8(img, 0))
        assert (tmp_path / f"aux_{n}.png").read_bytes() == ref.read_bytes(), n
