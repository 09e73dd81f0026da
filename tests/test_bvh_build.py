"""The GPU BVH builders (v-img_amd/csrc/bvh_build.hip) against their contract restated in numpy (tests/bvh_build_ref.py).

Without a GPU, the restatement is pinned on its own: Morton codes worked out by hand, the radix tree against a
top-down definition of the same tree, the PLOC tree against the layout's invariants, its leaf decisions re-derived in
float64, its cut, its cost against the LBVH's, and the number of clustering rounds on inputs whose unions tie.

On the GPU (-m gpu), vimg_hip_build_lbvh and vimg_hip_build_ploc are called directly on a bounds array and must give
the restatement's arrays byte for byte: num_nodes, max_depth, nodes, the box table, obj_indices."""
import ctypes as C

import numpy as np
import pytest

import bvh_build_ref as R
import scenes
from test_gpu_parity import _tree_cost
from test_host_and_abi import _check_tree
from vimg_amd import abi

F = np.float32
BUILDER = C.CFUNCTYPE(C.c_int, C.c_uint32, abi.Pf32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p, abi.Pf32,
                      C.POINTER(C.c_uint32))


# ---- inputs: all synthetic, fixed seeds --------------------------------------------------------------------------------
def random_boxes(n, seed=None):
    """Centres of both signs in [-10, 10]^3, half extents from 0.001 to 1."""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    c = rng.uniform(-10, 10, (n, 3)).astype(F)
    e = (10.0 ** rng.uniform(-3, 0, (n, 3))).astype(F)
    return np.concatenate([c - e, c + e], axis=1)


def centred_boxes(n, free_axes, seed):
    """Boxes -e .. +e on the axes not in `free_axes` (their centres are exactly 0 there), random on the others."""
    b = random_boxes(n, seed)
    e = (b[:, 3:] - b[:, :3]) * F(0.5)
    for a in range(3):
        if a not in free_axes:
            b[:, a], b[:, 3 + a] = -e[:, a], e[:, a]
    return b


def flat_boxes(n, seed, line):
    """Boxes of no volume: rectangles in the plane y = 0.25 or, `line`, segments on the line y = 0.25, z = -1.5."""
    b = random_boxes(n, seed)
    b[:, 1] = b[:, 4] = F(0.25)
    if line:
        b[:, 2] = b[:, 5] = F(-1.5)
    return b


def seven_cells(n=3000, seed=77):
    """Point boxes whose centres fall in 7 Morton cells: two corners and five cell middles, jittered by 1e-4."""
    rng = np.random.default_rng(seed)
    q = np.array([[0, 0, 0], [1024, 1024, 1024], [100.5, 700.5, 30.5], [100.5, 700.5, 31.5], [511.5, 512.5, 3.5], [900.5, 2.5, 1000.5],
                  [512.5, 512.5, 512.5]]) / 1024.0
    c = (q[rng.integers(0, 7, n)] + rng.uniform(0, 1e-4, (n, 3))).astype(F)
    return np.concatenate([c, c + F(1e-3)], axis=1)


def quad_grid(m):
    """An m x m grid of quads of side 1 / m in the plane y = 0, two triangles per quad: both have the quad's box."""
    i = np.arange(m, dtype=F)
    x0, z0 = np.meshgrid(i / F(m), i / F(m))
    x1, z1 = np.meshgrid((i + F(1)) / F(m), (i + F(1)) / F(m))
    zero = np.zeros(m * m, F)
    quad = np.stack([x0.ravel(), zero, z0.ravel(), x1.ravel(), zero, z1.ravel()], axis=1)
    return np.repeat(quad, 2, axis=0)


def row_of_boxes(n):
    """n equal boxes in a row: spacing 0.25, half-width 0.1."""
    c = np.zeros((n, 3), F)
    c[:, 0] = np.arange(n, dtype=F) * F(0.25)
    return np.concatenate([c - F(0.1), c + F(0.1)], axis=1)


def identical_boxes(n):
    return np.tile(np.array([[-1, -2, -3, 1, 2, 3]], F), (n, 1))


def pairs_at_equality(pairs=24):
    """Unit cubes in overlapping pairs, the pairs far apart along x: [0, 1]^3 and [0, 1]^2 x [0.5, 1.5] have half area 3
    each and 4 together, so a pair's split costs 0.5 + 0.75 + 0.75 = 2.0 exactly: what its leaf of 2 costs.  "No
    dearer": a leaf."""
    b = np.zeros((2 * pairs, 6), F)
    b[:, 3:] = 1
    b[1::2, 2] += F(0.5)
    b[1::2, 5] += F(0.5)
    b[:, 0] += np.repeat(np.arange(pairs, dtype=F) * F(64), 2)
    b[:, 3] += np.repeat(np.arange(pairs, dtype=F) * F(64), 2)
    return b


SIZES = (1, 2, 3, 16, 17, 18, 63, 64, 65, 255, 256, 257, 1000, 5000)
INPUTS = {f"random {n}": (lambda n=n: random_boxes(n)) for n in SIZES}
INPUTS.update({
    "centres equal on y": lambda: centred_boxes(300, (0, 2), 11),
    "centres equal on all axes": lambda: centred_boxes(300, (), 12),
    "flat boxes in a plane": lambda: flat_boxes(300, 13, line=False),
    "flat boxes on a line": lambda: flat_boxes(300, 14, line=True),
    "3000 centres in 7 cells": seven_cells,
    "pairs at leaf = split": pairs_at_equality,
    "64 x 64 quads": lambda: quad_grid(64),
    "row of 5000": lambda: row_of_boxes(5000),
    "4200 identical": lambda: identical_boxes(4200),
    "row of 14500": lambda: row_of_boxes(14500),
})
TIED = {"row of 5000": 21, "4200 identical": 13, "64 x 64 quads": 13}      # rounds the restatement takes on them
# (input, ploc(...) arguments, environment)
KNOBS = [(f"random {n}", dict(cut=t), {"VIMG_PLOC_TOP": str(t)}) for n in (257, 1000) for t in (4, 8, 100)]
KNOBS += [("16 x 16 quads", dict(cut=t), {"VIMG_PLOC_TOP": str(t)}) for t in (6, 10)]   # (cuts of 8 and 16: keys tie at the threshold)
KNOBS += [("random 65", dict(radius=r), {"VIMG_PLOC_R": str(r)}) for r in (1, 2, 12, 40)]
KNOBS += [("random 1000", dict(top=False), {"VIMG_PLOC_NO_TOP": "1"})]
INPUTS["16 x 16 quads"] = lambda: quad_grid(16)


# ---- the restatement, pinned without a GPU ----------------------------------------------------------------------------
def _points(c):
    c = np.asarray(c, dtype=F)
    return np.concatenate([c, c], axis=1)


def test_morton_codes_worked_out_by_hand():
    """10 bits per axis, x on the highest bit of each three, clamped at the far corner; no extent on an axis: code 0.
    Bit k of an axis' cell lands on bit 3 k + {2, 1, 0} for x, y, z."""
    x_all, y_all = 0x24924924, 0x12492492                                     # cell 1023 on x, on y
    cube = [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0.5, 0.25, 0.75)]    # cells (512, 256, 768) for the last
    want = [0, 0x3FFFFFFF, x_all, y_all, (1 << 29) | (1 << 25) | (1 << 27) | (1 << 24)]
    assert R.morton_codes(_points(cube)).tolist() == want
    flat = [(0, 0, 0.5), (1, 1, 0.5), (1 / 1024, 0, 0.5), (0, 1, 0.5), (0.125, 0.75, 0.5)]   # cells (128, 768, -) for the last
    want = [0, x_all | y_all, 1 << 2, y_all, (1 << 23) | (1 << 28) | (1 << 25)]
    assert R.morton_codes(_points(flat)).tolist() == want
    keys, order = R.morton_keys(_points(cube))
    assert order.tolist() == [0, 3, 2, 4, 1] and [int(k) >> 32 for k in keys] == sorted(R.morton_codes(_points(cube)).tolist())


def _top_down(keys, a, b):
    """The radix tree by definition: split a sorted range at the highest bit in which its first and last key differ."""
    if a == b:
        return a
    bit = 1 << ((keys[a] ^ keys[b]).bit_length() - 1)
    s = next(i for i in range(a, b + 1) if keys[i] & bit)
    return (_top_down(keys, a, s - 1), _top_down(keys, s, b))


def test_radix_tree_is_the_top_down_split_at_the_highest_differing_bit():
    rng = np.random.default_rng(5)
    for n, codes in ((2, 1), (3, 2), (700, 5), (2000, 40), (1500, 1500)):
        high = rng.integers(0, 1 << 30, codes)[rng.integers(0, codes, n)]    # heavy duplication in the high word
        keys = np.sort((high.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64))
        left, right = R.radix_tree(keys)

        def nested(c):
            return c if c < n else (nested(int(left[c - n])), nested(int(right[c - n])))
        assert nested(n) == _top_down([int(k) for k in keys], 0, n - 1)


def test_lbvh_of_one_primitive_is_a_single_leaf():
    b = random_boxes(1)
    num, depth, nodes, bb, obj = R.lbvh(b)
    assert (num, depth, nodes.tolist(), obj.tolist()) == (1, 1, [[0, 1]], [0])
    assert np.array_equal(bb, np.array([b[0, :3], [0, 0, 0], b[0, 3:], [0, 0, 0]], F))


def _restated_scene(s, **kw):
    """`s` with the restatement's PLOC tree (or, lbvh=True, its LBVH), installed through build_bvh_with; also the
    bounds the host handed over."""
    seen = {}

    def build(n, bounds6, num_nodes, max_depth, nodes_p, bb_p, obj_p):
        b = seen["bounds"] = np.ctypeslib.as_array(bounds6, (n, 6)).copy()
        num, depth, nodes, bb, obj = R.lbvh(b) if kw.get("lbvh") else R.ploc(b, **kw)[:5]
        np.ctypeslib.as_array(C.cast(nodes_p, C.POINTER(C.c_uint32)), (num, 2))[:] = nodes
        np.ctypeslib.as_array(bb_p, (2 * num + 2, 3))[:] = bb
        np.ctypeslib.as_array(obj_p, (n,))[:] = obj
        num_nodes[0], max_depth[0] = num, depth
        return 0
    s.build_bvh_with(C.cast(BUILDER(build), C.c_void_p))
    return seen["bounds"]


@pytest.fixture(scope="module")
def config4_bounds():
    s = scenes.config4_scene(res=(96, 54), n_lat=48, env=(64, 32))
    bounds = _restated_scene(s)
    return s, bounds


def test_restated_ploc_keeps_the_layouts_invariants_and_costs_less_than_the_lbvh(config4_bounds):
    s, bounds = config4_bounds
    _check_tree(s, leaf_max=8)                                               # (leaf sizes <= 8 among the invariants)
    ploc_cost = _tree_cost(s)
    nodes = s.bvh_arrays()[0]
    assert nodes[:, 1].max() > 1                                             # some leaves were collapsed
    _restated_scene(s, lbvh=True)
    _check_tree(s, leaf_max=1)
    lbvh_cost = _tree_cost(s)
    print(f"config 4 (n_lat 48, {len(bounds)} primitives): restated PLOC {ploc_cost:.4f}, restated LBVH {lbvh_cost:.4f}")
    assert ploc_cost < lbvh_cost
    small = scenes.big_mesh_scene(res=(48, 32), n=14)                        # (~420 primitives, spheres among them)
    for kw in (dict(), dict(top=False), dict(cut=8), dict(radius=1)):
        _restated_scene(small, **kw)
        _check_tree(small, leaf_max=8)


def _area64(box):
    d = box[..., 3:].astype(np.float64) - box[..., :3].astype(np.float64)
    return d[..., 0] * d[..., 1] + d[..., 0] * d[..., 2] + d[..., 1] * d[..., 2]


MARGIN = 1e-5   # relative distance from leaf == split inside which float32 may decide either way: a decision is a dozen
#                 float32 operations (2^-24 each) on costs that carry at most three levels of the same, well below 1e-5


@pytest.mark.parametrize("name", ["config4", "random 5000", "64 x 64 quads"])
def test_leaf_decisions_rederived_in_float64(name, config4_bounds):
    """Every merge of the agglomeration ends as one leaf exactly when it has at most 8 primitives and
    float(primitives) <= 0.5 + sum over children of area_child / area x cost_child, the children's costs being what
    their own decisions left.  Recomputed in float64 from the tree's boxes; decisions within MARGIN of equality are
    left out, and they are under 1 % of the decisions.  The emitted arrays then show the same: a leaf holds a whole
    ended subtree, and no node with children of at most 8 primitives is one that should have ended."""
    b = config4_bounds[1] if name == "config4" else INPUTS[name]()
    tree, order, _, _ = R.ploc_tree(b, top=False)
    n = tree.n
    cost = np.ones(2 * n - 1)
    decided = close = 0
    for tid in range(n, 2 * n - 1):                                           # creation order: children first
        c = [int(tree.left[tid - n]), int(tree.right[tid - n])]
        area = _area64(tree.box[tid])
        split = 0.5 + sum((_area64(tree.box[k]) / area if area > 0 else 1.0) * cost[k] for k in c)
        prims = int(tree.nprims[c[0]] + tree.nprims[c[1]])
        assert prims == tree.nprims[tid]
        cost[tid] = prims if tree.as_leaf[tid] else split
        if prims > 8:
            assert not tree.as_leaf[tid]
            continue
        decided += 1
        if abs(prims - split) <= MARGIN * split:
            close += 1
            continue
        assert bool(tree.as_leaf[tid]) == (prims <= split), (tid, prims, split)
    print(f"{name}: {decided} decisions, {close} within {MARGIN} of equality ({100.0 * close / decided:.3f} %)")
    assert decided > n // 4 and close < 0.01 * decided
    # the emitted tree: children after parents, so costs bottom-up in reverse
    num, _, nodes, bb, _ = R.emit(tree, order)
    ecost, eprims, earea = np.zeros(num), np.zeros(num, np.int64), np.zeros(num)
    earea[0] = _area64(np.concatenate([bb[0], bb[2]]))
    for k in range(num):
        first, count = int(nodes[k, 0]), int(nodes[k, 1])
        if count == 0:
            base = 2 * first + 2
            earea[first], earea[first + 1] = _area64(np.concatenate([bb[base], bb[base + 2]])), _area64(np.concatenate([bb[base + 1], bb[base + 3]]))
    for k in range(num - 1, -1, -1):
        first, count = int(nodes[k, 0]), int(nodes[k, 1])
        if count:
            ecost[k], eprims[k] = count, count
            continue
        eprims[k] = eprims[first] + eprims[first + 1]
        ecost[k] = 0.5 + sum((earea[j] / earea[k] if earea[k] > 0 else 1.0) * ecost[j] for j in (first, first + 1))
        assert eprims[k] > 8 or eprims[k] > ecost[k] * (1 - MARGIN), (k, eprims[k], ecost[k])
    assert nodes[:, 1].max() <= 8 and eprims[0] == n


def test_a_leaf_that_costs_what_its_split_costs_is_a_leaf():
    """leaf <= split, not <: the reference's builders end a subtree where a leaf is no dearer."""
    _, _, nodes, _, obj, _ = R.ploc(pairs_at_equality())
    leaves = nodes[nodes[:, 1] > 0]
    assert len(leaves) == 24 and (leaves[:, 1] == 2).all()
    assert all(sorted(obj[f:f + 2]) == [2 * (min(obj[f:f + 2]) // 2), 2 * (min(obj[f:f + 2]) // 2) + 1] for f in leaves[:, 0])


def _leaves_under(tree, tid):
    out, stack = [], [int(tid)]
    while stack:
        r = stack.pop()
        if r < tree.n:
            out.append(r)
        else:
            stack += [int(tree.right[r - tree.n]), int(tree.left[r - tree.n])]
    return out


@pytest.mark.parametrize("name, cut", [("random 1000", 16384), ("random 1000", 100), ("random 257", 4), ("16 x 16 quads", 6),
                                       ("64 x 64 quads", 16384)])
def test_the_cut_is_a_partition_of_the_primitives(name, cut):
    """The cut's subtrees are pairwise disjoint and hold every primitive once, in the order of their first sorted
    position; it has the requested size unless keys tie at the threshold (the duplicated quads) or fewer nodes can
    be opened."""
    tree, _, _, members = R.ploc_tree(INPUTS[name](), cut=cut)
    assert members is not None and len(members) >= 3
    below = [_leaves_under(tree, m) for m in members]
    assert sorted(sum(below, [])) == list(range(tree.n))
    firsts = [min(x) for x in below]
    assert firsts == sorted(firsts)
    print(f"{name}, cut {cut}: {len(members)} subtrees")
    if name == "16 x 16 quads":
        assert len(members) == 8 > cut                                       # the four quarters' keys are equal: all opened
    elif cut < 200:
        assert len(members) == cut


@pytest.mark.parametrize("name", list(TIED) + ["row of 14500"])
def test_tied_unions_do_not_serialise_the_rounds(name):
    """Equal boxes at equal spacing, coincident boxes, duplicated quads: every union ties with its neighbours'.  The
    pair order of ploc_nearest still merges a share of the array per round: at most 64 rounds (one pair per round,
    as under "ties go to the lower index", is 1 488, 4 199 and 43 rounds on the first three, and no tree at all from
    about 4 100 primitives: the builder stops at 4 096 rounds)."""
    rounds = R.ploc(INPUTS[name]())[5]
    print(f"{name}: {rounds} rounds")
    assert rounds <= 64
    assert name not in TIED or rounds == TIED[name]


# ---- the builders on the GPU --------------------------------------------------------------------------------------------
def _gpu_build(builder, b):
    """vimg_hip_build_lbvh / _ploc on the bounds `b`: (num_nodes, max_depth, nodes, bb, obj_indices), the buffers cut
    to what the builder says it wrote."""
    lib = abi.hip_lib()
    b = np.ascontiguousarray(b, dtype=F)
    n = len(b)
    nodes = np.full((2 * n - 1, 2), 0xDEADBEEF, np.uint32)
    bb = np.full(((2 * (2 * n - 1) + 2), 3), np.nan, F)
    obj = np.full(n, 0xDEADBEEF, np.uint32)
    num, depth = C.c_uint32(0), C.c_uint32(0)
    fn = lib.vimg_hip_build_lbvh if builder == "lbvh" else lib.vimg_hip_build_ploc
    rc = fn(n, b.ctypes.data_as(abi.Pf32), C.byref(num), C.byref(depth), nodes.ctypes.data_as(C.c_void_p), bb.ctypes.data_as(abi.Pf32),
            obj.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0, lib.vimg_hip_last_error().decode()
    assert 1 <= num.value <= 2 * n - 1
    return num.value, depth.value, nodes[:num.value], bb[:2 * num.value + 2], obj


def _assert_same_tree(got, want, what):
    assert got[:2] == want[:2], (what, "num_nodes, max_depth", got[:2], want[:2])
    for g, w, part in zip(got[2:], want[2:5], ("nodes", "bb", "obj_indices")):
        g, w = np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)
        assert g.shape == w.shape, (what, part)
        bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
        assert len(bad) == 0, (what, part, f"{len(bad)} rows differ, the first at {bad[0]}", g[bad[0]], w[bad[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["lbvh", "ploc"])
@pytest.mark.parametrize("name", [k for k in INPUTS if k != "16 x 16 quads"])
def test_gpu_builder_gives_the_restatements_bytes(name, builder, monkeypatch):
    """Both exported builders on every input, the knobs at their defaults.  The row of 14 500 and the 4 200 identical
    boxes are the inputs on which build_ploc used to run out of rounds: VIMG_OK and the restatement's tree."""
    for var in ("VIMG_PLOC_R", "VIMG_PLOC_TOP", "VIMG_PLOC_NO_TOP"):
        monkeypatch.delenv(var, raising=False)
    b = INPUTS[name]()
    if name == "3000 centres in 7 cells":
        assert len(np.unique(R.morton_codes(b))) == 7
    want = R.lbvh(b) if builder == "lbvh" else R.ploc(b)
    _assert_same_tree(_gpu_build(builder, b), want, (name, builder))


@pytest.mark.gpu
@pytest.mark.parametrize("name, kw, env", KNOBS, ids=[f"{n}, {e}" for n, _, e in KNOBS])
def test_gpu_ploc_reads_its_knobs_like_the_restatement(name, kw, env, monkeypatch):
    """VIMG_PLOC_TOP makes the cut smaller than the tree at a small size (and the duplicated quads put several keys
    at its threshold), VIMG_PLOC_R = 40 clamps the search at both ends of a 65-cluster array, VIMG_PLOC_NO_TOP keeps
    the agglomeration's own top."""
    for var in ("VIMG_PLOC_R", "VIMG_PLOC_TOP", "VIMG_PLOC_NO_TOP"):
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    b = INPUTS[name]()
    _assert_same_tree(_gpu_build("ploc", b), R.ploc(b, **kw), (name, env))


@pytest.mark.gpu
def test_gpu_ploc_through_the_scene_is_the_restatement_on_the_hosts_bounds():
    """build_bvh_with(ploc_builder()) on a moved host scene: the bounds the host hands the builder are the primitives'
    boxes at the new positions, and the scene's arrays are the restatement's on them.  DeviceScene.rebuild_bvh("ploc")
    after the same move (its bounds come from scene_rebuild_bounds, on the device) then reads as that scene's upload:
    image and all event counters, node visits among them."""
    from test_scene_rebuild import _upd, large_deformation
    from test_scene_update import _dev, _same
    make = lambda: scenes.big_mesh_scene(res=(48, 32), n=14)          # noqa: E731  (~420 primitives)
    v, nrm, sp = large_deformation(make(), seed=21)
    h = make()
    if len(v):
        h.set_vertices(v, nrm)
    if len(sp):
        h.set_spheres(sp)
    seen = {}
    real = abi.hip_lib().vimg_hip_build_ploc

    def through(n, bounds6, num_nodes, max_depth, nodes_p, bb_p, obj_p):
        seen["bounds"] = np.ctypeslib.as_array(bounds6, (n, 6)).copy()
        return real(n, bounds6, num_nodes, max_depth, nodes_p, bb_p, obj_p)
    h.build_bvh_with(C.cast(BUILDER(through), C.c_void_p))
    b = seen["bounds"]
    assert 200 < len(b) < 1000
    view = h.view.contents
    verts = np.ctypeslib.as_array(view.vertices, (view.num_vertices, 3))
    for i in range(len(b)):                                                  # the boxes of the MOVED primitives
        pr = view.prims[i]
        if pr.type == abi.PRIM_TRIANGLE:
            m = view.meshes[view.tri_mesh[pr.index]]
            t = verts[[m.first_vertex + view.tri_indices[pr.index * 3 + k] for k in range(3)]]
            lo, hi = t.min(0), t.max(0)
        else:
            s = view.spheres[pr.index]
            c = np.array(list(s.center), F)
            lo, hi = c - F(s.radius), c + F(s.radius)
        assert np.array_equal(b[i], np.concatenate([lo, hi])), i
    nodes, bb, obj, depth = h.bvh_arrays()
    want = R.ploc(b)
    _assert_same_tree((len(nodes), depth, nodes, bb[:2 * len(nodes) + 2], obj), want, "build_bvh_with(ploc_builder())")
    d = _dev(make())
    _upd(d, v, nrm, sp)
    d.rebuild_bvh("ploc")
    p = h.default_params(samples=4)
    _same(d.render_to_host(p), _dev(h).render_to_host(p), "rebuild_bvh after the move")
