"""Host side of changing a resident scene (vimg_host_set_vertices / _set_spheres / _refit_bvh): the refit is
the reference for the GPU refit of vimg_hip_scene_update_geometry, so it is pinned here bit for bit against an
independent numpy restatement with the same selects and fold order.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import scenes
from test_host_and_abi import _check_tree
from vimg_amd import abi, host

BUILDER = C.CFUNCTYPE(C.c_int, C.c_uint32, abi.Pf32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                      C.c_void_p, abi.Pf32, C.POINTER(C.c_uint32))

JSON_SCENES = ["cornell_box_spheres.json", "disney_spheres.json", "empty_box.json", "glass_in_box.json",
               "MIS_light_tests/sphere_light_small_mis.json", "MIS_light_tests/sphere_light_medium_mis.json"]


def median_split_builder(leaf_cap):
    """A vimg_bvh_builder_fn in Python (the pattern of test_build_bvh_with_a_supplied_builder): median splits
    along the widest axis of the centres' box until a node holds at most `leaf_cap` primitives."""
    def build_fn(n, bounds6, num_nodes, max_depth, nodes_p, bb_p, obj_p):
        b = np.ctypeslib.as_array(bounds6, (n, 6)).copy()
        nodes = np.ctypeslib.as_array(C.cast(nodes_p, C.POINTER(C.c_uint32)), (2 * n - 1, 2))
        bb = np.ctypeslib.as_array(bb_p, (2 * (2 * n - 1) + 3, 3))
        obj = np.ctypeslib.as_array(obj_p, (n,))
        centre = (b[:, :3] + b[:, 3:]) * 0.5
        state = {"next": 1, "pos": 0, "depth": 0}

        def box(ids):
            return b[ids, :3].min(0), b[ids, 3:].max(0)

        def build(node, ids, d):
            state["depth"] = max(state["depth"], d)
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
            build(first, halves[0], d + 1)
            build(first + 1, halves[1], d + 1)

        ids = np.arange(n)
        bb[0], bb[2] = box(ids)
        build(0, ids, 1)
        num_nodes[0], max_depth[0] = state["next"], state["depth"]
        return 0

    return BUILDER(build_fn)


def with_python_tree(s, leaf_cap):
    cb = median_split_builder(leaf_cap)
    s.build_bvh_with(C.cast(cb, C.c_void_p))
    s._keep.append(cb)
    return s


def chained_scene(res=(64, 48)):
    """big_mesh_scene split once, into two leaves of ~210 primitives (> 127: the upload chains them)."""
    s = with_python_tree(scenes.big_mesh_scene(res=res, n=14), 300)
    assert max(s.view.contents.bvh.nodes[i].obj_count for i in range(s.view.contents.bvh.num_nodes)) > 127
    return s


def single_prim_scene(res=(40, 32)):
    """One emissive sphere: the root is a leaf."""
    s = host.HostScene()
    lt = s.add_material("diffuse_light", emit=(5, 5, 5))
    s.add_sphere((0, 0, 0), 1.0, lt)
    s.set_camera((0, 1, 6), (0, 0.5, 0), (0, 1, 0), 40, res)
    s.set_render_defaults("mis", 4, 8)
    s.build_bvh()
    return s


def deformed(s, seed, scale=0.05):
    """Seeded new positions for every vertex, normal and sphere of `s` (same shapes)."""
    rng = np.random.default_rng(seed)
    v, n, sp = s.geometry()
    v = (v + rng.normal(0.0, scale, v.shape)).astype(np.float32)
    n = n + rng.normal(0.0, 0.2, n.shape)
    n = (n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-6)).astype(np.float32)
    sp = sp.copy()
    if len(sp):
        sp[:, :3] += rng.normal(0.0, scale, (len(sp), 3)).astype(np.float32)
        sp[:, 3] *= rng.uniform(0.9, 1.1, len(sp)).astype(np.float32)
    return v, n, sp.astype(np.float32)


def apply_host(s, v=None, n=None, sp=None):
    if v is not None:
        s.set_vertices(v, n)
    if sp is not None and len(sp):
        s.set_spheres(sp)
    s.refit_bvh()
    return s


# ---- the numpy restatement ----------------------------------------------------------------------------------
def _sel_min(a, b):
    return np.where(b < a, b, a)          # std::min / glm::min: b < a ? b : a


def _sel_max(a, b):
    return np.where(a < b, b, a)          # a < b ? b : a


def prim_bounds_np(s):
    """prim_bounds (host/bvh_build.cpp): triangles vmin(v0, vmin(v1, v2)), spheres c -/+ r, float32."""
    v = s.view.contents
    n = v.num_prims
    prims = np.ctypeslib.as_array(C.cast(v.prims, C.POINTER(C.c_uint32)), (n, 2))
    lo = np.zeros((n, 3), np.float32)
    hi = np.zeros((n, 3), np.float32)
    tri = prims[:, 0] == abi.PRIM_TRIANGLE
    if tri.any():
        verts = np.ctypeslib.as_array(v.vertices, (v.num_vertices, 3))
        idx = np.ctypeslib.as_array(v.tri_indices, (v.num_tris, 3)).astype(np.int64)
        mesh_of = np.ctypeslib.as_array(v.tri_mesh, (v.num_tris,))
        first = np.array([v.meshes[i].first_vertex for i in range(v.num_meshes)], np.int64)
        t = prims[tri, 1]
        gid = idx[t] + first[mesh_of[t]][:, None]
        p0, p1, p2 = verts[gid[:, 0]], verts[gid[:, 1]], verts[gid[:, 2]]
        lo[tri] = _sel_min(p0, _sel_min(p1, p2))
        hi[tri] = _sel_max(p0, _sel_max(p1, p2))
    for i in np.nonzero(~tri)[0]:
        sp = v.spheres[int(prims[i, 1])]
        c = np.array(list(sp.center), np.float32)
        r = np.float32(sp.radius)
        lo[i], hi[i] = c - r, c + r
    return lo, hi


def refit_np(s):
    """The bb table vimg_host_refit_bvh must give: leaves folded over obj_indices order from the first,
    internal nodes grow(left, right), the root at triples 0 / 2, triple 1 untouched."""
    nodes, bb, obj, _ = s.bvh_arrays()
    plo, phi = prim_bounds_np(s)
    order, head = [0], 0
    while head < len(order):
        first, count = nodes[order[head]]
        if count == 0:
            order += [int(first), int(first) + 1]
        head += 1
    lo = np.zeros((len(nodes), 3), np.float32)
    hi = np.zeros((len(nodes), 3), np.float32)
    out = bb.copy()
    for i in reversed(order):
        first, count = int(nodes[i][0]), int(nodes[i][1])
        if count:
            ids = obj[first:first + count]
            a, b = plo[ids[0]], phi[ids[0]]
            for j in ids[1:]:
                a, b = _sel_min(a, plo[j]), _sel_max(b, phi[j])
        else:
            a, b = _sel_min(lo[first], lo[first + 1]), _sel_max(hi[first], hi[first + 1])
            base = 2 * first + 2
            out[base], out[base + 1], out[base + 2], out[base + 3] = lo[first], lo[first + 1], hi[first], hi[first + 1]
        lo[i], hi[i] = a, b
    out[0], out[2] = lo[0], hi[0]
    return out


SCENE_MAKERS = {**{name: (lambda name=name: scenes.json_scene(name, res=(48, 32))) for name in JSON_SCENES},
                "json binned": lambda: scenes.json_scene("cornell_box_spheres.json", res=(48, 32), bvh=abi.BVH_BINNED),
                "feature": lambda: scenes.feature_scene(res=(48, 32)),
                "chained leaves": chained_scene,
                "single primitive": single_prim_scene}


@pytest.mark.parametrize("name", list(SCENE_MAKERS))
def test_refit_after_displacement_is_the_numpy_restatement(name):
    s = SCENE_MAKERS[name]()
    v, n, sp = deformed(s, seed=11)
    apply_host(s, v, n, sp)
    got_v, got_n, got_sp = s.geometry()
    assert np.array_equal(got_v, v) and np.array_equal(got_sp, sp)
    # normals are taken only for the rows of meshes that have them
    view = s.view.contents
    for i in range(view.num_meshes):
        m = view.meshes[i]
        rows = slice(m.first_vertex, m.first_vertex + m.num_vertices)
        assert np.array_equal(got_n[rows], n[rows] if m.has_normals else np.zeros_like(n[rows])), (name, i)
    _, bb, _, _ = s.bvh_arrays()
    want = refit_np(s)
    assert np.array_equal(bb.view(np.uint32), want.view(np.uint32)), name
    # the boxes still hold what hangs below them
    leaf_max = max(int(c) for _, c in s.bvh_arrays()[0])
    _check_tree(s, leaf_max=leaf_max)


@pytest.mark.parametrize("builder", ["sweep", "binned", "python", "python big leaves"])
def test_refit_of_unmoved_geometry_is_the_builders_own_boxes(builder):
    if builder in ("sweep", "binned"):
        s = scenes.feature_scene(res=(48, 32))
        if builder == "binned":
            s.build_bvh(abi.BVH_BINNED)
        leaf_max = 8 if builder == "sweep" else 1 << 30
    elif builder == "python":
        s = with_python_tree(scenes.json_scene("cornell_box_spheres.json", res=(48, 32)), 2)
        leaf_max = 2
    else:
        s = chained_scene()
        leaf_max = 300
    nodes0, bb0, obj0, depth0 = s.bvh_arrays()
    s.refit_bvh()
    nodes1, bb1, obj1, depth1 = s.bvh_arrays()
    assert np.array_equal(nodes0, nodes1) and np.array_equal(obj0, obj1) and depth0 == depth1
    assert np.array_equal(bb1, bb0)           # numerically: another fold order may only flip the sign of a zero
    assert _check_tree(s, leaf_max=leaf_max) == depth0


def test_refit_moves_boxes_with_the_geometry():
    """A sphere moved far away: its leaf's box, every box above it and the root follow."""
    s = scenes.json_scene("cornell_box_spheres.json", res=(48, 32))
    _, _, sp = s.geometry()
    sp[0, :3] += 1000.0
    s.set_spheres(sp)
    before = s.bvh_arrays()[1]
    s.refit_bvh()
    after = s.bvh_arrays()[1]
    assert after[2].max() >= sp[0, :3].max() and before[2].max() < sp[0, :3].max()
    assert np.array_equal(after, refit_np(s))


def test_wrong_lengths_and_missing_tree_raise():
    s = scenes.json_scene("cornell_box_spheres.json", res=(48, 32))
    v, n, sp = s.geometry()
    with pytest.raises(host.HostError, match="set_vertices"):
        s.set_vertices(v[:-1])
    with pytest.raises(host.HostError, match="normals"):
        s.set_vertices(v, n[:-1])
    with pytest.raises(host.HostError, match="set_spheres"):
        s.set_spheres(sp[:, :3])
    assert np.array_equal(s.geometry()[0], v)        # nothing was taken
    bare = host.HostScene()
    m = bare.add_material("lambertian", tex=bare.add_texture_const((0.5, 0.5, 0.5)))
    bare.add_sphere((0, 0, 0), 1.0, m)
    with pytest.raises(host.HostError, match="no BVH"):
        bare.refit_bvh()
    with pytest.raises(host.HostError):
        bare.set_spheres(np.zeros((1, 4), np.float32))
    lib = abi.host_lib()
    assert lib.vimg_host_refit_bvh(None) == -1
    assert lib.vimg_host_set_vertices(None, None, None) == -1
    assert lib.vimg_host_set_spheres(s._h, None) == -1


def test_camera_lookat_is_what_set_camera_stores():
    s = scenes.json_scene("cornell_box_spheres.json", res=(48, 32))
    s.set_camera((1, 2, 9), (0, 0.5, 0), (0, 1, 0), 35.0, (48, 32), aperture_radius=0.1, focal_dist=8.0)
    cam = host.camera_lookat((1, 2, 9), (0, 0.5, 0), (0, 1, 0), 35.0, (48, 32), 0.1, 8.0)
    # the scene's view carries the new camera at once (a renderer uploading it sees it without a rebuild)
    assert bytes(s.view.contents.camera) == bytes(cam)

