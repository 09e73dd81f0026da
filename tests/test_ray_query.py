"""Ray queries on a resident scene (vimg_hip_trace_rays, _occluded, _camera_rays; DeviceScene.trace_rays, .occluded,
.camera_rays): the render's walk on the caller's rays.  Closest hits and their records equal the oracle's
PROBE_CLOSEST_HIT, occlusion its PROBE_OCCLUDED, camera rays the GPU probe's PROBE_CAMERA_RAY; the answer does not
depend on the launch shape; the queries leave renders and progressive accumulators as they were."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import scenes
from test_gpu_parity import _ulp_diff
from test_scene_update_host import apply_host, deformed

pytestmark = pytest.mark.gpu

T_MIN = np.float32(0.0001)


def _dev(s, **opts):
    from vimg_amd import hip
    return hip.DeviceScene(s, **opts)


def _rays(o, d, t_min=T_MIN, t_max=np.inf):
    n = len(o)
    r = np.empty((n, 8), dtype=np.float32)
    r[:, 0:3], r[:, 4:7] = o, d
    r[:, 3], r[:, 7] = t_min, t_max
    return r


def _bounds(s):
    v, _, sp = s.geometry()
    pts = [v] if len(v) else []
    if len(sp):
        pts += [sp[:, :3] - sp[:, 3:4], sp[:, :3] + sp[:, 3:4]]
    p = np.concatenate(pts)
    return p.min(0), p.max(0)


def _prim_types(s, prim):
    P = s.view.contents.prims
    return np.array([P[int(i)].type for i in prim], dtype=np.int64)


def _query_rays(s, n_cam, n_rand, seed):
    """Camera rays of random pixel and lens samples, plus random rays from points inside the scene's box."""
    rng = np.random.default_rng(seed)
    w, h = s.resolution
    cam_in = np.stack([rng.uniform(0, w, n_cam), rng.uniform(0, h, n_cam), rng.random(n_cam), rng.random(n_cam)],
                      1).astype(np.float32)
    cam = O.probe(s, O.PROBE_CAMERA_RAY, cam_in)
    lo, hi = _bounds(s)
    o = rng.uniform(lo, hi, (n_rand, 3)).astype(np.float32)
    d = rng.normal(size=(n_rand, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return np.concatenate([_rays(cam[:, 0:3], cam[:, 3:6]), _rays(o, d)])


def _check_closest(d, s, rays, what, info=True):
    """trace_rays (numpy in, numpy out) against PROBE_CLOSEST_HIT on the same rays (t_min 1e-4, t_max inf)."""
    r = d.trace_rays(rays, info=info)
    ref = O.probe(s, O.PROBE_CLOSEST_HIT, rays[:, [0, 1, 2, 4, 5, 6]])
    hit = ref[:, 0] == 1
    assert np.array_equal(r.prim != -1, hit), what
    assert np.array_equal(r.t[hit].view(np.uint32), ref[hit, 1].view(np.uint32)), what
    assert np.array_equal(r.prim[hit], ref[hit, 2].astype(np.int32)), what
    assert np.all(np.isinf(r.t[~hit])) and np.all(r.bary[~hit] == 0), what
    if info:
        assert np.array_equal(r.mat[hit], ref[hit, 3].astype(np.int32)), what
        got = np.concatenate([r.p, r.ns, r.ng], 1)[hit]
        assert _ulp_diff(got, ref[hit, 4:13]).max(initial=0) == 0, what          # p, n_s, n_g
        assert _ulp_diff(r.uv[hit], ref[hit, 13:15]).max(initial=0) <= 4, what  # uv (acos / atan2)
        assert np.all(r.p[~hit] == 0) and np.all(r.mat[~hit] == 0), what
    return r, hit


# ---- caller-built trees (as in test_gpu_parity.py: leaves over 127 primitives, a caterpillar deeper than 32) -------
def _builder_type():
    from vimg_amd import abi
    return C.CFUNCTYPE(C.c_int, C.c_uint32, abi.Pf32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                       C.c_void_p, abi.Pf32, C.POINTER(C.c_uint32))


def big_leaves_builder(leaf_cap):
    def big_leaves(n, bounds6, num_nodes, max_depth, nodes_p, bb_p, obj_p):
        b = np.ctypeslib.as_array(bounds6, (n, 6)).copy()
        nodes = np.ctypeslib.as_array(C.cast(nodes_p, C.POINTER(C.c_uint32)), (2 * n - 1, 2))
        bb = np.ctypeslib.as_array(bb_p, (2 * (2 * n - 1) + 3, 3))
        obj = np.ctypeslib.as_array(obj_p, (n,))
        centre = (b[:, :3] + b[:, 3:]) * 0.5
        state = {"next": 1, "pos": 0, "depth": 0}

        def box(ids):
            return b[ids, :3].min(0), b[ids, 3:].max(0)

        def build(node, ids, dep):
            state["depth"] = max(state["depth"], dep)
            if len(ids) <= leaf_cap:
                nodes[node] = (state["pos"], len(ids))
                obj[state["pos"]:state["pos"] + len(ids)] = ids
                state["pos"] += len(ids)
                return
            lo, hi = box(ids)
            axis = int(np.argmax(hi - lo))
            order = ids[np.argsort(centre[ids, axis], kind="stable")]
            halves = (order[:len(ids) // 2], order[len(ids) // 2:])
            first = state["next"]
            state["next"] += 2
            nodes[node] = (first, 0)
            for k in (0, 1):
                c_lo, c_hi = box(halves[k])
                bb[2 * first + 2 + k], bb[2 * first + 4 + k] = c_lo, c_hi
            build(first, halves[0], dep + 1)
            build(first + 1, halves[1], dep + 1)

        ids = np.arange(n)
        bb[0], bb[2] = box(ids)
        build(0, ids, 1)
        num_nodes[0], max_depth[0] = state["next"], state["depth"]
        return 0
    return _builder_type()(big_leaves)


def caterpillar_builder():
    def caterpillar(n, bounds6, num_nodes, max_depth, nodes_p, bb_p, obj_p):
        b = np.ctypeslib.as_array(bounds6, (n, 6)).copy()
        nodes = np.ctypeslib.as_array(C.cast(nodes_p, C.POINTER(C.c_uint32)), (2 * n - 1, 2))
        bb = np.ctypeslib.as_array(bb_p, (2 * (2 * n - 1) + 3, 3))
        obj = np.ctypeslib.as_array(obj_p, (n,))
        order = np.argsort((b[:, 0] + b[:, 3]) + 0.37 * (b[:, 2] + b[:, 5]), kind="stable")
        obj[:] = order
        bb[0], bb[2] = b[:, :3].min(0), b[:, 3:].max(0)
        node, nxt = 0, 1
        for i in range(n - 1):              # node: leaf {order[i]} | everything behind it
            first = nxt
            nxt += 2
            nodes[node] = (first, 0)
            rest = order[i + 1:]
            bb[2 * first + 2], bb[2 * first + 4] = b[order[i], :3], b[order[i], 3:]
            bb[2 * first + 3], bb[2 * first + 5] = b[rest, :3].min(0), b[rest, 3:].max(0)
            nodes[first] = (i, 1)
            node = first + 1
        nodes[node] = (n - 1, 1)
        num_nodes[0], max_depth[0] = nxt, n
        return 0
    return _builder_type()(caterpillar)


def _with_builder(s, cb):
    s.build_bvh_with(C.cast(cb, C.c_void_p))
    return s


def big_leaves_scene(leaf_cap):
    s = _with_builder(scenes.big_mesh_scene(res=(64, 48), n=14), big_leaves_builder(leaf_cap))
    bvh = s.view.contents.bvh
    assert max(bvh.nodes[i].obj_count for i in range(bvh.num_nodes)) > 127
    return s


def caterpillar_scene():
    s = _with_builder(scenes.big_mesh_scene(res=(64, 48), n=4), caterpillar_builder())
    assert 32 < s.view.contents.bvh.max_depth <= 92
    return s


CLOSEST_CASES = {
    "feature env+lens": lambda: scenes.feature_scene(res=(96, 64)),
    "feature plain": lambda: scenes.feature_scene(res=(96, 64), envmap=False, lens=False),
    "disney_spheres": lambda: scenes.json_scene("disney_spheres.json", res=(120, 56)),
    "glass_in_box": lambda: scenes.json_scene("glass_in_box.json", res=(96, 72)),
    "cornell_box_spheres": lambda: scenes.json_scene("cornell_box_spheres.json", res=(80, 80)),
    "sphere_light_small": lambda: scenes.json_scene("MIS_light_tests/sphere_light_small_mis.json", res=(64, 64)),
    "odyssey quads": lambda: scenes.odyssey_without_monolith(res=(64, 48)),
    "one leaf of all primitives": lambda: big_leaves_scene(10 ** 9),
    "leaves of ~250": lambda: big_leaves_scene(300),
    "caterpillar": caterpillar_scene,
}


# ---- 1. closest hit against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CLOSEST_CASES))
def test_closest_hit_is_the_oracles(case):
    s = CLOSEST_CASES[case]()
    d = _dev(s)
    rays = _query_rays(s, 3000, 3000, seed=len(case))
    _, hit = _check_closest(d, s, rays, case)
    assert hit.sum() > 500, (case, hit.sum())
    # the lean build (no record) gives the same hits
    lean = d.trace_rays(rays)
    full = d.trace_rays(rays, info=True)
    assert lean.p is None
    for k in ("t", "prim", "bary"):
        assert np.array_equal(getattr(lean, k).view(np.uint32), getattr(full, k).view(np.uint32)), (case, k)


def test_closest_hit_on_a_tree_beyond_lds():
    s = scenes.config5_scene(res=(256, 144))
    d = _dev(s)
    assert "deep" in d.kernel, d.kernel           # the tree does not fit in LDS
    rays = _query_rays(s, 2000, 2000, seed=5)
    _, hit = _check_closest(d, s, rays, "config 5 stand-in")
    assert hit.sum() > 1000


def _triangle_corners(s, prim):
    """Positions [N, 3, 3] of the hit triangles' vertices in VimgScene order (tri_indices are mesh-local)."""
    v = s.view.contents
    verts = s.geometry()[0].astype(np.float64)
    prims = [v.prims[int(i)] for i in prim]
    out = np.empty((len(prim), 3, 3))
    for k, pr in enumerate(prims):
        t = pr.index
        first = v.meshes[v.tri_mesh[t]].first_vertex
        out[k] = verts[[first + v.tri_indices[3 * t + j] for j in range(3)]]
    return out


def test_barycentrics_rebuild_the_hit_point():
    """b1, b2 are tri_hit_info's weights of the triangle's 2nd and 3rd vertex: (1 - b1 - b2) p0 + b1 p1 + b2 p2, with
    the vertices looked up in the host scene, is the record's hit point up to rounding.  The same sum with the two
    weights swapped, or with the first vertex's weight in place of one of them, is not.  Spheres have none."""
    s = scenes.feature_scene(res=(96, 64))
    d = _dev(s)
    rays = _query_rays(s, 3000, 3000, seed=3)
    r = d.trace_rays(rays, info=True)
    assert r.bary.min() >= -1e-6 and r.bary.max() <= 1 + 1e-6
    hit = r.prim >= 0
    sph = hit.copy()
    sph[hit] = _prim_types(s, r.prim[hit]) == 1
    assert np.all(r.bary[sph] == 0)
    tri = hit & ~sph
    assert tri.sum() > 1000
    c = _triangle_corners(s, r.prim[tri])
    b1, b2 = r.bary[tri, 0].astype(np.float64), r.bary[tri, 1].astype(np.float64)
    b0 = 1.0 - b1 - b2
    p = r.p[tri].astype(np.float64)
    tol = 1e-5 * max(1.0, np.abs(p).max())

    def err(w0, w1, w2):
        return np.abs(w0[:, None] * c[:, 0] + w1[:, None] * c[:, 1] + w2[:, None] * c[:, 2] - p).max(axis=1)

    assert err(b0, b1, b2).max() < tol
    for wrong in ((b0, b2, b1), (b1, b0, b2), (b2, b1, b0)):      # swapped, e0 for e1, e0 for e2
        assert np.median(err(*wrong)) > 10 * tol


# ---- 2. occlusion against the oracle ---------------------------------------------------------------------------------
def test_occlusion_is_the_oracles():
    s = scenes.feature_scene(res=(96, 64))
    d = _dev(s)
    rng = np.random.default_rng(2)
    rays = _query_rays(s, 3000, 3000, seed=9)
    rays[:, 7] = rng.uniform(0.05, 8.0, len(rays)).astype(np.float32)
    got = d.occluded(rays)
    ref = O.probe(s, O.PROBE_OCCLUDED, rays[:, [0, 1, 2, 4, 5, 6, 7]])[:, 0] == 1
    assert got.dtype == np.bool_ and np.array_equal(got, ref)
    assert 0.1 < ref.mean() < 0.9


def test_axis_aligned_and_box_plane_rays():
    """test_axis_aligned_rays_take_the_exact_slab_path's rays: zero direction components and origins on box planes."""
    s = scenes.json_scene("disney_spheres.json")
    d = _dev(s)
    rng = np.random.default_rng(11)
    dirs = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0],
                     [0, 0.6, -0.8], [0.6, 0, -0.8], [0.6, 0.8, 0]], dtype=np.float32)
    planes = np.array([-650, 650, -277.5, 277.5, 277, -77.5, -300, 300, 0, -177.5, -200, 40], dtype=np.float32)
    o = rng.uniform(-600, 600, (3000, 3)).astype(np.float32)
    o[:, 1] = rng.uniform(-270, 270, 3000)
    o[:, 2] = rng.uniform(-270, 270, 3000)
    snap = rng.random((3000, 3)) < 0.4
    o[snap] = rng.choice(planes, snap.sum())
    rays = _rays(o, dirs[rng.integers(0, len(dirs), 3000)])
    _, hit = _check_closest(d, s, rays, "axis-aligned", info=False)
    assert hit.sum() > 1000
    rays[:, 7] = rng.uniform(1, 1500, 3000).astype(np.float32)
    ref = O.probe(s, O.PROBE_OCCLUDED, rays[:, [0, 1, 2, 4, 5, 6, 7]])[:, 0] == 1
    assert np.array_equal(d.occluded(rays), ref)


# ---- 3. the t range ---------------------------------------------------------------------------------------------------
def test_the_t_range():
    """[t_min, t_max] is the walk's range.  Every test in the walk is monotone in t_max, so a hit found within a
    cut range is the full range's hit.  Where the box tests and the sphere test decide, cutting t_max to the closest
    hit t* keeps that hit and one ulp below loses it: they compare t itself with t_max.  The watertight triangle test
    compares in the scaled space instead (t_scaled against t_max * det, then t = t_scaled * (1 / det); oracle and
    kernel alike), so at t_max = t* or one ulp below, whether a triangle is kept is the rounding of t_max * det
    against t_scaled, not t* against t_max.  On those rays the answer must be the oracle's occlusion over the same
    range, and a hit still the same hit."""
    s = scenes.feature_scene(res=(96, 64))
    d = _dev(s)
    rays = _query_rays(s, 3000, 3000, seed=4)
    full = d.trace_rays(rays)
    hit = full.prim >= 0
    hr = rays[hit].copy()
    t_star, prim = full.t[hit], full.prim[hit]
    sphere = _prim_types(s, prim) == 1
    assert sphere.sum() > 100 and (~sphere).sum() > 100
    for what, t_max, keeps in (("t_max = t*", t_star, True),
                               ("t_max = t* - 1 ulp", np.nextafter(t_star, np.float32(0)), False)):
        hr[:, 7] = t_max
        r = d.trace_rays(hr)
        occ = d.occluded(hr)
        ref = O.probe(s, O.PROBE_OCCLUDED, hr[:, [0, 1, 2, 4, 5, 6, 7]])[:, 0] == 1
        got_hit = r.prim >= 0
        assert np.array_equal(got_hit, ref) and np.array_equal(occ, ref), what
        # a hit within the cut range is the same hit
        assert np.array_equal(r.t[got_hit].view(np.uint32), t_star[got_hit].view(np.uint32)), what
        assert np.array_equal(r.prim[got_hit], prim[got_hit]), what
        assert np.all(got_hit[sphere] == keeps), what            # t compared as it is
        odd = got_hit[~sphere] != keeps
        print(f"{what}: {odd.sum()} of {(~sphere).sum()} triangle hits decided by the scaled comparison")
    # empty and NaN ranges are misses, not errors
    bad = rays[:64].copy()
    bad[:16, 3], bad[:16, 7] = 2.0, 1.0
    bad[16:32, 3] = np.nan
    bad[32:48, 7] = np.nan
    bad[48:, 3], bad[48:, 7] = np.nan, np.nan
    r = d.trace_rays(bad, info=True)
    assert np.all(r.prim == -1) and np.all(np.isinf(r.t)) and np.all(r.mat == 0)
    assert not d.occluded(bad).any()
    # closest hit within range <=> occluded, on finite ranges
    rng = np.random.default_rng(8)
    fin = rays.copy()
    fin[:, 7] = rng.uniform(0.01, 6.0, len(fin)).astype(np.float32)
    assert np.array_equal(d.trace_rays(fin).prim >= 0, d.occluded(fin))


# ---- 4. launch shapes ---------------------------------------------------------------------------------------------------
def _bits_of(res):
    import torch
    return torch.cat([res.t.view(torch.int32)[:, None], res.prim[:, None], res.bary.contiguous().view(torch.int32)], 1)


def test_launch_shapes_give_the_same_bytes(monkeypatch):
    import torch
    s = scenes.json_scene("disney_spheres.json", res=(180, 80))
    d = _dev(s)                                # the launch policy's shape
    monkeypatch.setenv("VIMG_HIP_QUERY_BLOCKS", "1")
    d_persistent = _dev(s)                     # the persistent grid (read at upload)
    monkeypatch.setenv("VIMG_HIP_QUERY_BLOCKS", "0")
    d_blocks = _dev(s)                         # one workgroup per 256 rays
    monkeypatch.delenv("VIMG_HIP_QUERY_BLOCKS")
    big = _query_rays(s, 20000, 20000, seed=12)
    rng = np.random.default_rng(13)
    n_big = 3 * 1024 * 1024 + 17
    rays_all = _cuda(big[rng.integers(0, len(big), n_big)])
    for n in (1, 63, 64, 65, 4097, n_big):
        rays = rays_all[:n]
        one = d.trace_rays(rays, info=True)
        ref = _bits_of(one).clone()
        info = torch.cat([one.p, one.ns, one.ng, one.uv], 1).contiguous().view(torch.int32)
        assert torch.equal(_bits_of(d.trace_rays(rays, info=True)), ref), n                  # twice
        occ = d.occluded(rays)
        for other in (d_persistent, d_blocks):
            assert torch.equal(_bits_of(other.trace_rays(rays)), ref), n
            b2 = other.trace_rays(rays, info=True)
            assert torch.equal(torch.cat([b2.p, b2.ns, b2.ng, b2.uv], 1).contiguous().view(torch.int32), info), n
            assert torch.equal(other.occluded(rays), occ), n
        cuts = sorted({0, n, *[int(c) for c in rng.integers(0, n + 1, 3)]})
        parts = [_bits_of(d.trace_rays(rays[a:b])) for a, b in zip(cuts, cuts[1:]) if b > a]
        assert torch.equal(torch.cat(parts), ref), (n, cuts)
        occ_parts = [d.occluded(rays[a:b]) for a, b in zip(cuts, cuts[1:]) if b > a]
        assert torch.equal(torch.cat(occ_parts), occ), (n, cuts)
    # numpy in, numpy out: the same answers
    r = d.trace_rays(big[:5000])
    assert np.array_equal(r.prim, d.trace_rays(_cuda(big[:5000])).prim.cpu().numpy())
    # n == 0
    empty = d.trace_rays(np.zeros((0, 8), np.float32), info=True)
    assert empty.t.shape == (0,) and d.occluded(np.zeros((0, 8), np.float32)).shape == (0,)


def test_bad_inputs_raise_value_error():
    import torch
    s = scenes.json_scene("disney_spheres.json", res=(32, 16))
    d = _dev(s)
    with pytest.raises(ValueError, match="float32"):
        d.trace_rays(np.zeros((4, 8), np.float64))
    with pytest.raises(ValueError, match="shape"):
        d.trace_rays(np.zeros((4, 7), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        d.occluded(torch.zeros((8, 16), device="cuda")[:, ::2])
    with pytest.raises(ValueError, match="CUDA device"):
        d.camera_rays(torch.zeros((4, 4)))
    with pytest.raises(ValueError, match="aligned"):
        d.trace_rays(torch.zeros(8 * 4 + 1, device="cuda")[1:].view(4, 8))


# ---- 5. after update_geometry ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [lambda: scenes.feature_scene(res=(96, 64)),
                                  lambda: scenes.json_scene("MIS_light_tests/sphere_light_small_mis.json", res=(64, 64))],
                         ids=["feature", "sphere json"])
def test_queries_after_update_geometry_are_the_refit_host_scene(make):
    s = make()
    d = _dev(s)
    rays = _query_rays(s, 2000, 2000, seed=21)
    before = d.trace_rays(rays)
    v, n, sp = deformed(s, 5, 0.05)
    d.update_geometry(vertices=v, normals=n, spheres=sp if len(sp) else None)
    h = apply_host(make(), v, n, sp)
    r, _ = _check_closest(d, h, rays, "after update_geometry")
    assert not np.array_equal(r.t.view(np.uint32), before.t.view(np.uint32))
    rng = np.random.default_rng(22)
    occ_rays = rays.copy()
    occ_rays[:, 7] = rng.uniform(0.05, 8.0, len(rays)).astype(np.float32)
    ref = O.probe(h, O.PROBE_OCCLUDED, occ_rays[:, [0, 1, 2, 4, 5, 6, 7]])[:, 0] == 1
    assert np.array_equal(d.occluded(occ_rays), ref)


# ---- 6. camera rays and picking -----------------------------------------------------------------------------------------
def test_camera_rays_are_the_probes_and_picking_is_the_oracles():
    s = scenes.feature_scene(res=(96, 64))          # thin lens on
    d = _dev(s)
    rng = np.random.default_rng(6)
    n = 4096
    smp = np.stack([rng.uniform(0, 96, n), rng.uniform(0, 64, n), rng.random(n), rng.random(n)], 1).astype(np.float32)
    rays = d.camera_rays(smp)
    probe = d.probe(O.PROBE_CAMERA_RAY, smp)
    assert np.array_equal(rays[:, [0, 1, 2, 4, 5, 6]].view(np.uint32), probe[:, 0:6].view(np.uint32))
    assert np.all(rays[:, 3] == T_MIN) and np.all(np.isinf(rays[:, 7]))
    assert _ulp_diff(rays[:, [0, 1, 2, 4, 5, 6]], O.probe(s, O.PROBE_CAMERA_RAY, smp)[:, 0:6]).max() <= 2
    # picking: pixel centres through the camera, then the closest hit
    ys, xs = np.mgrid[0:64, 0:96]
    centres = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5, np.full(xs.size, 0.5), np.full(xs.size, 0.5)],
                       1).astype(np.float32)
    pick_rays = d.camera_rays(_cuda(centres))
    picked = d.trace_rays(pick_rays, info=True)
    _check_closest(d, s, pick_rays.cpu().numpy(), "picking")
    assert (picked.prim >= 0).sum().item() > centres.shape[0] // 2
    # after set_camera the rays follow the new camera
    cam = dict(look_from=(0.4, 1.6, 5.5), look_at=(0.1, 0.5, 0.0), up=(0, 1, 0), vfov_deg=35.0,
               aperture_radius=0.05, focal_dist=5.0)
    d.set_camera(**cam)
    moved = d.camera_rays(smp)
    assert not np.array_equal(moved, rays)
    assert np.array_equal(moved[:, [0, 1, 2, 4, 5, 6]].view(np.uint32),
                          d.probe(O.PROBE_CAMERA_RAY, smp)[:, 0:6].view(np.uint32))
    h = scenes.feature_scene(res=(96, 64))
    h.set_camera(cam["look_from"], cam["look_at"], cam["up"], cam["vfov_deg"], (96, 64), cam["aperture_radius"],
                 cam["focal_dist"])
    assert _ulp_diff(moved[:, [0, 1, 2, 4, 5, 6]], O.probe(h, O.PROBE_CAMERA_RAY, smp)[:, 0:6]).max() <= 2


# ---- 7. no side effects --------------------------------------------------------------------------------------------------
def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _queries(d, rays):
    r = d.trace_rays(rays, info=True)
    return r, d.occluded(rays)


def test_queries_leave_renders_and_accumulators_as_they_were():
    import torch
    s = scenes.feature_scene(res=(96, 64))
    p = s.default_params(samples=8, depth=6)
    d = _dev(s)
    rays = _cuda(_query_rays(s, 4000, 4000, seed=31))
    first = d.render(p, stats=False).clone()
    r0, o0 = _queries(d, rays)
    r0 = (_bits_of(r0).clone(), o0.clone())
    second = d.render(p, stats=False)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    # a progressive frame keeps going across queries, without a reset, and ends at the one-shot bits
    acc = d.progressive(p)
    acc.render(3, out=False)
    _queries(d, rays)
    img = acc.render(5)
    assert acc.samples == 8
    torch.cuda.synchronize()
    assert torch.equal(img.view(torch.int32), first.view(torch.int32))
    # on a non-default torch stream: the same answers
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        r1, o1 = _queries(d, rays)
        b1 = _bits_of(r1).clone()
    side.synchronize()
    assert torch.equal(b1, r0[0]) and torch.equal(o1, r0[1])
    # and with stream= given while another stream is current
    r2 = d.trace_rays(rays, stream=side)
    side.synchronize()
    assert torch.equal(_bits_of(r2), r0[0])
