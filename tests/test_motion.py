"""The motion library on the GPU: vimg_motion_previous_position against its numpy restatement (tests/motion_ref.py) bit
for bit on synthetic tables with indices out of range, on a scene with a translated mesh and sphere, and inside
DeviceScene.temporal_preview(motion=...): a camera-only sequence is what it is without ``motion``, and a moving panel
keeps its history.  One test needs no GPU: the panel's placement, by a float64 brute-force intersector."""
import ctypes as C

import numpy as np
import pytest

import geom_ref as G
import motion_ref as R
import scenes
from test_temporal import orbit_camera, rse

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def gpu():
    from vimg_amd import hip, motion
    hip.init(0)
    return motion


# ---- 1. the kernel is the restatement, bit for bit -----------------------------------------------------------------
NV, NT, NS = 37, 23, 5


def synthetic(w, h, seed=0, spheres=True):
    """Random frames, hits and tables for a w x h picture.  About 5 % of the indices are out of range at each level: the
    hit's prim, a triangle's index, a vertex row, a sphere's index, a primitive's type.  Half of the vertices and three
    of the five spheres move - one only translates, one only scales, one gets radius 0 - so moved and static
    primitives, and triangles with one or two moved corners, all occur.  ``spheres`` False: num_spheres = 0, every sphere
    primitive is out of range and no ray is needed."""
    rng = np.random.default_rng(1234 + seed)
    n = w * h
    ns = NS if spheres else 0
    tris = rng.integers(0, NV, (NT, 3)).astype(np.uint32)
    bad = rng.random(NT) < 0.05
    bad[3] = True
    tris[bad, rng.integers(0, 3, bad.sum())] = rng.choice(np.array([NV, NV + 7, 0xFFFFFFF0], np.uint32), bad.sum())
    prims = [(R.TRIANGLE, t) for t in range(NT)] + [(R.SPHERE, k) for k in range(NS)]
    prims += [(R.TRIANGLE, NT), (R.TRIANGLE, 0x80000000), (R.SPHERE, NS), (R.SPHERE, 0xFFFFFFFF), (2, 0), (77, 1)]
    prims = np.array(prims, np.uint32)[rng.permutation(len(prims))]
    prim = rng.integers(0, len(prims), n).astype(np.uint32)
    u = rng.random(n)
    prim[u < 0.2] = R.NO_HIT
    beyond = (u >= 0.2) & (u < 0.25)
    prim[beyond] = rng.choice(np.array([len(prims), len(prims) + 5, 0xFFFFFFFE], np.uint32), beyond.sum())
    b1 = rng.random(n).astype(F)
    b2 = (rng.random(n).astype(F) * (F(1) - b1)).astype(F)
    hits = R.hit_records(rng.uniform(0.5, 20.0, n).astype(F), prim, b1, b2)
    rays = rng.normal(0, 3, (n, 8)).astype(F)
    position = rng.normal(0, 5, (h, w, 3)).astype(F)
    position[rng.random((h, w)) < 0.1, 0] = F(-0.0)
    old_v = rng.normal(0, 4, (NV, 3)).astype(F)
    new_v = old_v.copy()
    moved = rng.random(NV) < 0.5
    new_v[moved] += rng.normal(0, 1, (moved.sum(), 3)).astype(F)
    old_s = np.concatenate([rng.normal(0, 4, (NS, 3)), rng.uniform(0.5, 2.0, (NS, 1))], axis=1).astype(F)
    new_s = old_s.copy()
    new_s[0, :3] += np.array([1, -2, 0.5], F)
    new_s[1, 3] *= F(1.7)
    new_s[2] = np.array([0.25, 0.5, -1, 0], F)
    return dict(position=position, hits=hits, rays=rays, prims=prims, tris=tris, nv=NV, ns=ns, old_v=old_v, new_v=new_v,
                old_s=old_s[:ns], new_s=new_s[:ns])


def _want(c, vertices=True, spheres=True):
    return R.previous_position(c["position"], c["hits"], c["rays"], c["prims"], c["tris"], c["nv"], c["ns"],
                               c["old_v"] if vertices else None, c["new_v"] if vertices else None,
                               c["old_s"] if spheres else None, c["new_s"] if spheres else None)


def _tables(mo, c):
    import torch
    return mo.SceneTables(torch.from_numpy(c["prims"].view(np.int32)).cuda(), torch.from_numpy(c["tris"].view(np.int32)).cuda(), c["nv"],
                          c["ns"])


def _same(got, want, what):
    q, code = got
    q, code = (q.cpu().numpy(), None if code is None else code.cpu().numpy()) if not isinstance(q, np.ndarray) else (q, code)
    assert q.shape == want[0].shape and q.dtype == F
    assert np.array_equal(_bits(q), _bits(want[0])), (what, int((_bits(q) != _bits(want[0])).sum()))
    if code is not None:
        assert code.dtype == np.uint8 and np.array_equal(code, want[1]), what


SIZES = [(1, 1), (65, 3), (64, 4), (130, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_kernel_is_the_restatement_bit_for_bit(gpu, size):
    """W x H = 1 x 1, 65 x 3 (a one-lane second wave, a partial workgroup), 64 x 4 (exactly one workgroup) and 130 x 9
    (three workgroups in both directions), with both table pairs, each pair alone, neither, no rays and no spheres, no
    code output, outputs of the caller's, numpy in and out, and on a stream of the caller's.  About a quarter of the
    hits name an index that is out of range at some level: they get code 3 and the position's bits, and the call ends
    clean."""
    import torch
    w, h = size
    c = synthetic(w, h, seed=w)
    t = _tables(gpu, c)
    dev = {k: torch.from_numpy(c[k]).cuda() for k in ("position", "hits", "rays", "old_v", "new_v", "old_s", "new_s")}
    old, new = gpu.Positions(dev["old_v"], dev["old_s"]), gpu.Positions(dev["new_v"], dev["new_s"])
    want = _want(c)
    if w * h >= 192:
        assert all((want[1] == k).any() for k in range(4))                       # all four codes occur
        out_of_range = want[1] == R.OUT_OF_RANGE
        assert out_of_range.mean() > 0.1 and np.array_equal(_bits(want[0][out_of_range]), _bits(c["position"][out_of_range]))
        static = want[1] == R.STATIC
        assert np.array_equal(_bits(want[0][static]), _bits(c["position"][static])) and (_bits(want[0][static]) == 0x80000000).any()
    _same(gpu.previous_position(dev["position"], dev["hits"], dev["rays"], t, old, new), want, "both pairs")
    assert np.array_equal(_bits(dev["position"].cpu().numpy()), _bits(c["position"]))          # the frame was only read
    _same(gpu.previous_position(dev["position"], dev["hits"], dev["rays"], t, (dev["old_v"], None), (dev["new_v"], None)),
          _want(c, spheres=False), "vertices alone")
    _same(gpu.previous_position(dev["position"], dev["hits"], dev["rays"], t, (None, dev["old_s"]), (None, dev["new_s"])),
          _want(c, vertices=False), "spheres alone")
    none = _want(c, vertices=False, spheres=False)
    assert np.array_equal(_bits(none[0]), _bits(c["position"])) and set(np.unique(none[1])) <= {R.STATIC, R.OUT_OF_RANGE}
    _same(gpu.previous_position(dev["position"], dev["hits"], dev["rays"], t, gpu.Positions(), gpu.Positions()), none, "no pair")
    # a scene without spheres: every sphere primitive is out of range, and no ray is given
    c0 = synthetic(w, h, seed=w, spheres=False)
    _same(gpu.previous_position(dev["position"], dev["hits"], None, _tables(gpu, c0), (dev["old_v"], None), (dev["new_v"], None)),
          _want(c0, spheres=False), "no spheres, no rays")
    # no code output; outputs of the caller's
    q, code = gpu.previous_position(dev["position"], dev["hits"], dev["rays"], t, old, new, out_code=False)
    assert code is None
    _same((q, None), want, "no code")
    mine, mine_code = torch.full((h, w, 3), -7.0, device="cuda"), torch.full((h, w), 9, dtype=torch.uint8, device="cuda")
    q, code = gpu.previous_position(dev["position"], dev["hits"], dev["rays"], t, old, new, out=mine, out_code=mine_code)
    assert q is mine and code is mine_code
    _same((q, code), want, "the caller's outputs")
    # numpy in, numpy out
    q, code = gpu.previous_position(c["position"], c["hits"], c["rays"], t, (c["old_v"], c["old_s"]), (c["new_v"], c["new_s"]))
    assert isinstance(q, np.ndarray) and isinstance(code, np.ndarray)
    _same((q, code), want, "numpy")
    # a stream of the caller's
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    q, code = gpu.previous_position(dev["position"], dev["hits"], dev["rays"], t, old, new, stream=side)
    side.synchronize()
    _same((q, code), want, "side stream")


# ---- 2. on a scene -----------------------------------------------------------------------------------------------
D_MESH = np.array([8, 0, -24], F)            # new - old of the second mesh's vertices
D_SPHERE = np.array([-512, 1024, 256], F)    # ... of the third sphere's centre


def _centre_hits(mo, dev, h, w):
    """(rays [H W, 8], hit records [H W, 4], RayHits with info) of the pixel-centre rays, as CUDA tensors."""
    import torch
    rays = dev.camera_rays(torch.from_numpy(mo.centre_samples(h, w)).cuda())
    hits, info = torch.empty((h * w, 4), device="cuda"), torch.empty((h * w, 12), device="cuda")
    return rays, hits, dev.trace_rays(rays, info=True, out=(hits, info))


@pytest.mark.gpu
def test_a_translated_mesh_and_sphere_on_a_scene(gpu):
    """scenes.feature_scene at 72 x 48 without the lens, as it stands, is the NEW scene; under the OLD positions its
    second mesh stood at - (8, 0, -24) and its third sphere at - (-512, 1024, 256).  The position frame is the hit
    point of each pixel's centre ray (trace_rays' record).  Every pixel whose centre hit is a moved primitive has
    Q - P = -d within 4 * 2^-23 * |d|inf per component (the roundings of w0 and of the weighted sum, at the size of d);
    every other pixel has P's bits and code 0; and a moved sphere's Q lies on the old sphere within 1e-3 (eight
    roundings of at most half an ulp at magnitude 1024).  The rendered `position` feature frame agrees with the centre
    hits to a pixel's footprint: the rays are in frame-array order."""
    import torch
    from vimg_amd import hip
    W, H = 72, 48
    s = scenes.feature_scene(res=(W, H), lens=False)
    dev = hip.DeviceScene(s)
    tables = gpu.SceneTables.from_host(s)
    v = s.view.contents
    assert (tables.num_prims, tables.num_tris, tables.num_vertices, tables.num_spheres) == (v.num_prims, v.num_tris, v.num_vertices, 3)
    new_v, _, new_s = s.geometry()
    mesh = 4                                                     # three quads, the textured grid, then this flat grid
    first, count = v.meshes[mesh].first_vertex, v.meshes[mesh].num_vertices
    old_v, old_s = new_v.copy(), new_s.copy()
    old_v[first:first + count] -= D_MESH
    old_s[2, :3] -= D_SPHERE
    rays, hits, rh = _centre_hits(gpu, dev, H, W)
    P = rh.p.reshape(H, W, 3).contiguous()
    Q, code = gpu.previous_position(P, hits, rays, tables, (torch.from_numpy(old_v).cuda(), torch.from_numpy(old_s).cuda()),
                                    tables.positions)
    P, Q, code, prim = P.cpu().numpy(), Q.cpu().numpy(), code.cpu().numpy(), rh.prim.cpu().numpy().reshape(H, W)
    prims = gpu.prim_records(s).astype(np.int64)
    tri_mesh = np.ctypeslib.as_array(v.tri_mesh, (v.num_tris,))
    kind, index = prims[np.maximum(prim, 0), 0], prims[np.maximum(prim, 0), 1]
    on_mesh = (prim >= 0) & (kind == R.TRIANGLE) & (tri_mesh[np.minimum(index, v.num_tris - 1)] == mesh)
    on_sphere = (prim >= 0) & (kind == R.SPHERE) & (index == 2)
    assert on_mesh.sum() > 20 and on_sphere.sum() > 20, (on_mesh.sum(), on_sphere.sum())          # (the walls leave no miss)
    assert (code[on_mesh] == R.MOVED_TRIANGLE).all() and (code[on_sphere] == R.MOVED_SPHERE).all()
    rest = ~(on_mesh | on_sphere)
    assert (code[rest] == R.STATIC).all() and np.array_equal(_bits(Q[rest]), _bits(P[rest]))
    err = np.abs((Q[on_mesh].astype(np.float64) - P[on_mesh]) + D_MESH.astype(np.float64)).max()
    print(f"moved mesh: max |(Q - P) + d| = {err:.3e}, bound {4 * 2.0 ** -23 * 24:.3e}")
    assert err <= 4 * 2.0 ** -23 * 24
    c_old = old_s[2, :3].astype(np.float64)
    off = np.abs(np.linalg.norm(Q[on_sphere].astype(np.float64) - c_old, axis=1) - float(old_s[2, 3])).max()
    print(f"moved sphere: max | |Q - c_old| - r_old | = {off:.3e}")
    assert off < 1e-3
    # the restatement, bit for bit, on the scene's own tables too
    want = R.previous_position(P, hits.cpu().numpy(), rays.cpu().numpy(), prims, gpu.tri_vertex_rows(s), v.num_vertices, 3, old_v, new_v,
                               old_s, new_s)
    assert np.array_equal(_bits(Q), _bits(want[0])) and np.array_equal(code, want[1])
    # the rendered position frame is these hits' up to the jitter inside a pixel: the scene spans about 8 units over 72
    # pixels, so 0.15 is more than a pixel's footprint on any surface that is not seen at a grazing angle
    feat = dev.render_features(s.default_params(samples=1), ("position", "coverage"))
    live = (feat["coverage"].cpu().numpy()[..., 0] == 1) & (prim >= 0)
    gap = np.abs(feat["position"].cpu().numpy() - P).max(axis=-1)[live]
    print(f"position frame against the centre hits: median {np.median(gap):.4f}, {100 * (gap < 0.15).mean():.1f} % below 0.15")
    assert live.mean() > 0.5 and np.median(gap) < 0.15


# ---- 3. a camera-only sequence is what it is without motion --------------------------------------------------------
CONFIGS = {"plain": dict(), "variance_guided": dict(variance_guided=True), "sparse": dict(sparse=2), "antilag": dict(antilag=True)}


def _state_bits(acc):
    import torch
    return {k: (v.view(torch.int32) if v.dtype == torch.float32 else v).cpu().numpy() for k, v in acc.state().items()}


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
def test_a_camera_only_sequence_is_bit_for_bit_the_preview_without_motion(gpu, config):
    """cornell_box_spheres at 64 x 64, three steps of test_temporal's orbit, then a material edit and rebuild_bvh: no
    position table changed, so no motion call is made (last_motion_code stays None) and frames, histories and the
    accumulator's records are those of the preview without ``motion``."""
    from vimg_amd import hip
    s = scenes.json_scene("cornell_box_spheres.json", res=(64, 64))
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    a, b = dev.temporal_preview(p, samples=4, **CONFIGS[config]), dev.temporal_preview(p, samples=4, motion=s, **CONFIGS[config])
    edits = [lambda i=i: dev.set_camera(*orbit_camera(i)) for i in range(3)]
    edits += [lambda: dev.update_materials(materials=s.materials()), lambda: dev.rebuild_bvh()]
    for edit in edits:
        edit()
        fa, fb = a.frame().cpu().numpy(), b.frame().cpu().numpy()
        assert np.array_equal(_bits(fa), _bits(fb))
        assert np.array_equal(_bits(a.history.tensor.cpu().numpy()), _bits(b.history.tensor.cpu().numpy()))
        assert b.last_motion_code is None and b._previous is None
    sa, sb = _state_bits(a.acc), _state_bits(b.acc)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    assert float(b.history.length.max()) > 1          # (there was a history to reproject)
    a.close()
    b.close()


# ---- 4. a moving object ------------------------------------------------------------------------------------------
RES = 96
PANEL_CENTRE, PANEL_HALF = np.array([200.0, 350.0, 140.0]), 75.0
STEP = np.array([36, 0, -24], F)
MOVES = 4


def panel_scene(res=RES):
    """cornell_box_spheres plus a 150 x 150 panel that faces the camera, in front of the spheres (the white one fills
    z = 160 .. 340 where the box's middle is), as the LAST mesh: its four vertices are the last four rows."""
    s = scenes.json_scene("cornell_box_spheres.json", res=(res, res))
    m = s.add_material("lambertian", tex=s.add_texture_const((0.2, 0.3, 0.7)))
    xf = np.diag([PANEL_HALF, -PANEL_HALF, -1.0, 1.0])            # scale, then half a turn about x: the normal looks at -z
    xf[:3, 3] = PANEL_CENTRE
    s.add_quad(xf.T.reshape(16).astype(F), m)
    s.build_bvh()
    return s


def panel_prims(s):
    v = s.view.contents
    prims = np.ctypeslib.as_array(C.cast(v.prims, C.POINTER(C.c_uint32)), (v.num_prims, 2))
    tri_mesh = np.ctypeslib.as_array(v.tri_mesh, (v.num_tris,))
    return np.array([i for i, (kind, index) in enumerate(prims) if kind == R.TRIANGLE and tri_mesh[index] == v.num_meshes - 1])


def moved_vertices(s, k):
    verts = s.geometry()[0]
    verts[-4:] += F(k) * STEP
    return verts


def erode(mask, r=2):
    out = mask.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            shifted = np.zeros_like(mask)
            ys, yd = (slice(dy, None), slice(None, mask.shape[0] - dy)) if dy >= 0 else (slice(None, dy), slice(-dy, None))
            xs, xd = (slice(dx, None), slice(None, mask.shape[1] - dx)) if dx >= 0 else (slice(None, dx), slice(-dx, None))
            shifted[yd, xd] = mask[ys, xs]
            out &= shifted
    return out


def dilate(mask, r=2):
    return ~erode(~mask, r)


def pinhole_rays(camera, h, w):
    """The pixel-centre rays of an abi.Camera in frame-array order, from temporal.world_to_pixel alone: a world point
    X has (hx, hy, hw) = A X + b, so the eye is -A^-1 b and pixel (c, r) is seen along A^-1 (c, r, 1)."""
    from vimg_amd import temporal
    m = temporal.world_to_pixel(camera).astype(np.float64).reshape(3, 4)
    inv = np.linalg.inv(m[:, :3])
    eye = -inv @ m[:, 3]
    rr, cc = np.mgrid[0:h, 0:w]
    d = np.stack([cc + 0.5, rr + 0.5, np.ones_like(cc, float)], -1).reshape(-1, 3) @ inv.T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((h * w, 8), F)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = eye, 1e-4, d, np.inf
    return rays


def test_the_panels_placement_alone_gives_an_interior_of_at_least_50_pixels():
    """No GPU: a float64 brute-force closest hit (tests/geom_ref.py) of the pixel-centre rays against the scene after
    the four moves.  The panel's pixels, eroded by 2, are the interior the GPU test measures on; the panel is the
    nearest surface on all of them at every step, and it stays inside the picture."""
    s = panel_scene()
    v = s.view.contents
    assert np.array_equal(s.geometry()[0][-4:, 2], np.full(4, PANEL_CENTRE[2], F)) and v.meshes[v.num_meshes - 1].num_vertices == 4
    rays, panel = pinhole_rays(v.camera, RES, RES), panel_prims(s)
    assert len(panel) == 2
    for k in (0, MOVES):
        near = G.sweep(rays, G.Geometry.of_scene(s, verts=moved_vertices(s, k)))["prim_near"].reshape(RES, RES)
        on = np.isin(near, panel)
        inner = erode(on)
        print(f"after {k} moves: {on.sum()} panel pixels, {inner.sum()} after eroding by 2")
        assert inner.sum() >= 50 and not (on[0].any() or on[-1].any() or on[:, 0].any() or on[:, -1].any())


@pytest.fixture(scope="module")
def moving_panel(gpu):
    """Frame 0 stands, then four frames, each after update_geometry has moved the panel by (36, 0, -24); mis at 4 spp,
    denoise=False; one resident scene, walked by a preview with ``motion`` and one without."""
    from vimg_amd import hip
    s = panel_scene()
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    with_m, without = dev.temporal_preview(p, samples=4, denoise=False, motion=s), dev.temporal_preview(p, samples=4, denoise=False)
    panel = panel_prims(s)
    o = dict(scene=s, dev=dev, on=[], codes=[], hist=[], lengths=[])
    for k in range(MOVES + 1):
        if k:
            dev.update_geometry(vertices=moved_vertices(s, k))
        fm, fw = with_m.frame().cpu().numpy(), without.frame().cpu().numpy()
        prim = _centre_hits(gpu, dev, RES, RES)[2].prim.cpu().numpy().reshape(RES, RES)
        o["on"].append(np.isin(prim, panel))
        o["codes"].append(None if with_m.last_motion_code is None else with_m.last_motion_code.cpu().numpy().copy())
        o["hist"].append((with_m.history.tensor.cpu().numpy(), without.history.tensor.cpu().numpy()))
    o["frames"] = (fm, fw)
    o["ref"] = dev.render(s.default_params(integrator="mis", samples=1024), stats=False).cpu().numpy()
    o["interior"] = erode(o["on"][-1])
    with_m.close()
    without.close()
    return o


@pytest.mark.gpu
def test_a_moving_panel_keeps_its_history_with_motion_and_loses_it_without(moving_panel):
    """Over the interior - the pixels whose centre hit is the panel in the last frame, eroded by 2 px - the median
    history length is 5 with ``motion`` (all four taps of each of the four reprojections lie on the panel, have length k
    and blend to k + 1) and below 2 without (the history at the place where the surface now is belongs to the panel
    24 units further back or to the box: the plane test rejects it and the pixel starts over).
    Measured on the MI355X: 361 interior pixels; median length 5.0000 with motion, 1.0000 without, which
    is the behaviour before ``motion`` existed; per frame 1, 2, 3, 4, 5 against 1, 1, 1, 1, 1."""
    o = moving_panel
    inner = o["interior"]
    assert inner.sum() >= 50
    assert o["codes"][0] is None and all(c is not None for c in o["codes"][1:])
    for k in range(1, MOVES + 1):          # the motion call marks exactly the panel's pixels
        assert np.array_equal(o["codes"][k] == R.MOVED_TRIANGLE, o["on"][k]) and set(np.unique(o["codes"][k])) <= {0, 1}
    lm, lw = (float(np.median(h[0, ..., 3][inner])) for h in o["hist"][-1])
    per_frame = [tuple(float(np.median(h[0, ..., 3][erode(on)])) for h in pair) for pair, on in zip(o["hist"], o["on"])]
    print(f"interior: {inner.sum()} pixels; median history length with motion {lm:.4f}, without {lw:.4f}; per frame {per_frame}")
    assert abs(lm - (MOVES + 1)) <= 1e-3
    assert lw < 2


@pytest.mark.gpu
def test_the_moving_panel_is_closer_to_the_reference_with_motion(moving_panel):
    """Against mis at 1024 spp of the final scene, e = mean((x - ref)^2 / (ref^2 + 0.01)) over the interior is strictly
    smaller with ``motion`` than without.  Measured on the MI355X: 0.00025 with motion, 0.00040 without,
    a ratio of 1.62."""
    o = moving_panel
    inner = o["interior"]
    em, ew = (rse(f[inner], o["ref"][inner]) for f in o["frames"])
    print(f"interior relative squared error: with motion {em:.5f}, without {ew:.5f}, ratio {ew / em:.2f}")
    assert np.isfinite(o["frames"][0]).all() and em < ew


@pytest.mark.gpu
def test_static_pixels_away_from_the_panel_have_the_same_history_in_both_runs(moving_panel):
    """A pixel that has code 0 in every frame and is more than 2 px from every footprint of the panel, old or new, gets
    P's bits as Q and taps that no moved pixel touches: its history - colour, length, guides - is bit for bit that of
    the run without ``motion``, in every frame; plane G1 holds the current positions in both."""
    o = moving_panel
    near = np.zeros((RES, RES), bool)
    for on in o["on"]:
        near |= on
    static = ~dilate(near, 3)
    for c in o["codes"][1:]:
        static &= c == 0
    assert static.mean() > 0.5
    for k, (hm, hw) in enumerate(o["hist"]):
        assert np.array_equal(_bits(hm[:, static]), _bits(hw[:, static])), k
        assert np.array_equal(_bits(hm[2]), _bits(hw[2])), k          # G1: the current world, everywhere


# ---- 5. two updates, then one frame --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_updates_then_one_frame_are_one_displacement_and_the_callers_tensor_is_not_aliased(gpu):
    """Two update_geometry calls between two frames displace by their sum: Q is bit for bit that of one update by the
    sum, because the old positions are those of the frozen history's frame.  The table the caller handed over - a
    CUDA tensor, overwritten in place after the call - is not what is remembered."""
    import torch
    from vimg_amd import hip
    s = panel_scene()
    p = s.default_params(integrator="mis", samples=4)
    runs = {}
    for name in ("two", "one"):
        dev = hip.DeviceScene(s)
        pre = dev.temporal_preview(p, samples=4, denoise=False, motion=s)
        pre.frame()
        if name == "two":
            dev.update_geometry(vertices=moved_vertices(s, 1))
        mine = torch.from_numpy(moved_vertices(s, 2)).cuda()
        dev.update_geometry(vertices=mine)
        given = dev.vertices_given
        assert given is not mine and given.data_ptr() != mine.data_ptr()
        mine.zero_()                                            # the caller's tensor, overwritten in place
        pre.frame()
        runs[name] = (pre._previous.cpu().numpy(), pre.last_motion_code.cpu().numpy())
        # ... and a third update with the SAME values is a new table object: a motion call, displacement zero
        dev.update_geometry(vertices=moved_vertices(s, 2))
        assert dev.vertices_given is not given
        pre.frame()
        assert pre.last_motion_code is not None and not pre.last_motion_code.any().item()
        assert torch.equal(pre._previous.view(torch.int32), pre._guides.held[1]["position"].view(torch.int32))
        pre.close()
    assert np.array_equal(_bits(runs["two"][0]), _bits(runs["one"][0])) and np.array_equal(runs["two"][1], runs["one"][1])
    assert (runs["one"][1] == R.MOVED_TRIANGLE).sum() > 100


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["variance_guided", "sparse", "antilag"])
def test_the_other_previews_follow_a_moving_panel_too(gpu, config):
    """variance_guided, sparse=2 and antilag with ``motion``: frame 0, then two moving frames.  Outputs are finite and the
    interior's history grows from frame to frame."""
    from vimg_amd import hip
    s = panel_scene()
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    pre = dev.temporal_preview(p, samples=4, motion=s, **CONFIGS[config])
    panel, medians = panel_prims(s), []
    for k in range(3):
        if k:
            dev.update_geometry(vertices=moved_vertices(s, k))
        frame = pre.frame()
        assert bool(np.isfinite(frame.cpu().numpy()).all())
        on = np.isin(_centre_hits(gpu, dev, RES, RES)[2].prim.cpu().numpy().reshape(RES, RES), panel)
        medians.append(float(np.median(pre.history.length.cpu().numpy()[erode(on)])))
    print(f"{config}: median interior history length per frame {medians}")
    assert medians[0] < medians[1] < medians[2]
    pre.close()


# ---- 6. what the binding refuses -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_what_the_binding_refuses(gpu):
    import torch
    from vimg_amd import hip
    s = panel_scene(res=32)
    dev = hip.DeviceScene(s)
    p = s.default_params(integrator="mis", samples=4)
    with pytest.raises(ValueError, match="motion must be the HostScene"):
        dev.temporal_preview(p, motion=dev)
    with pytest.raises(ValueError, match="motion's host scene has"):
        dev.temporal_preview(p, motion=scenes.json_scene("cornell_box_spheres.json", res=(32, 32)))
    with pytest.raises(ValueError, match="tile_world must be 1"):
        dev.temporal_preview(s.default_params(integrator="mis", samples=4, tile_world=2), motion=s)
    c = synthetic(5, 3)
    t = _tables(gpu, c)
    with pytest.raises(ValueError, match="vertices must be given in both old and new"):
        gpu.previous_position(c["position"], c["hits"], c["rays"], t, (c["old_v"], None), (None, None))
    with pytest.raises(ValueError, match="rays may be None only for a scene without spheres"):
        gpu.previous_position(c["position"], c["hits"], None, t, (None, None), (None, None))
    with pytest.raises(ValueError, match="motion hits"):
        gpu.previous_position(c["position"], c["hits"][:-1], c["rays"], t, (None, None), (None, None))
    with pytest.raises(ValueError, match="motion old vertices"):
        gpu.previous_position(c["position"], c["hits"], c["rays"], t, (c["old_v"][:-1], None), (c["new_v"], None))
    with pytest.raises(ValueError, match="tables must be a motion.SceneTables"):
        gpu.previous_position(c["position"], c["hits"], c["rays"], None, (None, None), (None, None))
    pos = torch.from_numpy(c["position"]).cuda()
    with pytest.raises(hip.HipError, match="the previous-position output overlaps the position frame"):
        gpu.previous_position(pos, c["hits"], c["rays"], t, (None, None), (None, None), out=pos)
