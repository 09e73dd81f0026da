"""A new tree for a resident scene (vimg_hip_scene_rebuild_bvh, vimg_hip_scene_bvh_cost; DeviceScene.rebuild_bvh and
.bvh_cost): after a rebuild a launch reads exactly what an upload of the host scene with the same positions and a
build_bvh_with(hip.ploc_builder()) tree reads - image, all eight event counters (node visits among them: the TREE
is the same, not just the picture), heatmap, trace_pixel, ray queries, scene bytes - on every scheduler
configuration, and the image is the oracle's on that host scene.  "fresh" below is that upload.  That the device
layout made by kernels (breadth-first rank by a scan, node records, leaf slots) is the upload's renumbering is
not assumed anywhere: every test compares with the upload."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import scenes
from test_gpu_parity import SCHEDULES, _compare_images, _tree_cost, scheduler_scene
from test_progressive import STATS_FIELDS, _bits
from test_ray_query import _query_rays
from test_scene_update import UPDATE_CASES, _cuda, _dev, _same, _update
from test_scene_update_host import apply_host, chained_scene, deformed, single_prim_scene, with_python_tree

pytestmark = pytest.mark.gpu


def twist(points, turns):
    """`points` [N, 3] rotated about the vertical axis through their centroid by an angle that grows linearly with
    height: 2 pi turns (y - y_min) / (y_max - y_min); x and z rotated, float32."""
    p = np.asarray(points, dtype=np.float64)
    if len(p) == 0:
        return np.asarray(points, dtype=np.float32)
    c = p.mean(0)
    y0, y1 = p[:, 1].min(), p[:, 1].max()
    ang = 2.0 * np.pi * turns * (p[:, 1] - y0) / max(y1 - y0, 1e-30)
    x, z = p[:, 0] - c[0], p[:, 2] - c[2]
    out = p.copy()
    out[:, 0] = c[0] + np.cos(ang) * x - np.sin(ang) * z
    out[:, 2] = c[2] + np.sin(ang) * x + np.cos(ang) * z
    return out.astype(np.float32)


def large_deformation(s, seed, turns=2.0):
    """New positions a refit tree fits badly: the twist of two turns on the vertices and on the spheres' centres,
    then `deformed`'s jitter with its normal and radius changes (deformed(scale=0.02) alone barely changes a tree)."""
    v, n, sp = deformed(s, seed, 0.02)
    jitter_v = v - s.geometry()[0]
    v = (twist(s.geometry()[0], turns) + jitter_v).astype(np.float32)
    if len(sp):
        sp = sp.copy()
        sp[:, :3] = twist(sp[:, :3], turns)
    return v, n, sp


def fresh_host(s, v=None, n=None, sp=None, builder="ploc"):
    """The host scene `s` with these positions and a tree of the GPU builder: what rebuild_bvh must equal."""
    from vimg_amd import hip
    if v is not None and len(v):
        s.set_vertices(v, n)
    if sp is not None and len(sp):
        s.set_spheres(sp)
    return s.build_bvh_with(hip.ploc_builder() if builder == "ploc" else hip.lbvh_builder())


def _upd(d, v, n, sp):
    _update(d, v if len(v) else None, n if len(v) else None, sp)


# ---- 1. every feature -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(UPDATE_CASES))
def test_rebuilt_scene_is_the_fresh_upload_on_every_feature(case):
    make = lambda: UPDATE_CASES[case]()[0]              # noqa: E731
    kw = UPDATE_CASES[case]()[1]
    s = make()                                            # (the host's sweep tree)
    d = _dev(s)
    v, n, sp = large_deformation(s, seed=5)
    _upd(d, v, n, sp)
    d.rebuild_bvh()
    h = fresh_host(make(), v, n, sp)
    p = h.default_params(**kw)
    got = d.render_to_host(p)
    _same(got, _dev(h).render_to_host(p), case)
    cpu, cst, _ = O.render(h, p)
    _compare_images(got[0], cpu, f"{case}, rebuilt")
    assert got[1].paths == cst.paths


# ---- 2. every schedule ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_name", ["disney_spheres.json", "feature"])
def test_rebuilt_scene_on_every_schedule_heatmap_and_trace_pixel(scene_name):
    s0, p = scheduler_scene(scene_name)
    make = lambda: scheduler_scene(scene_name)[0]       # noqa: E731
    v, n, sp = large_deformation(s0, seed=9)
    h = fresh_host(make(), v, n, sp)
    for name in ("lane", "cu", "cu/nolds", "cu/stack1", "cu/early"):
        d, fresh = _dev(make(), **SCHEDULES[name]), _dev(h, **SCHEDULES[name])
        _upd(d, v, n, sp)
        d.rebuild_bvh()
        _same(d.render_to_host(p), fresh.render_to_host(p), (scene_name, name))
        assert np.array_equal(_bits(d.render_to_host(p, stats=False)), _bits(fresh.render_to_host(p, stats=False)))
        assert np.array_equal(_bits(d.trace_pixel(p, 17, 23)), _bits(fresh.trace_pixel(p, 17, 23))), (scene_name, name)
        assert np.array_equal(_bits(d.render_heatmap(p)), _bits(fresh.render_heatmap(p))), (scene_name, name)
        d.close()
        fresh.close()


# ---- 3. without an update -------------------------------------------------------------------------------------------
def test_rebuild_of_an_untouched_upload_twice_and_with_the_lbvh():
    make = lambda: scenes.feature_scene(res=(72, 48))    # noqa: E731
    p = make().default_params(samples=6, depth=7)
    d = _dev(make())
    sweep = d.render_to_host(p)
    d.rebuild_bvh()
    want = _dev(fresh_host(make())).render_to_host(p)
    first = d.render_to_host(p)
    _same(first, want, "ploc of the scene as uploaded")
    assert first[1].internal_visits != sweep[1].internal_visits       # (another tree than the upload's)
    d.rebuild_bvh()
    _same(d.render_to_host(p), first, "a second rebuild")
    d.rebuild_bvh(builder="lbvh")
    lb = _dev(fresh_host(make(), builder="lbvh"))
    _same(d.render_to_host(p), lb.render_to_host(p), "lbvh")
    assert d.bytes == lb.bytes
    d.rebuild_bvh(builder="ploc")
    _same(d.render_to_host(p), first, "back to ploc")


# ---- 4. the tree changes size -----------------------------------------------------------------------------------------
def _root_chain_scene():
    """All ~420 primitives of big_mesh_scene in ONE leaf: one chain, a handful of records."""
    return with_python_tree(scenes.big_mesh_scene(res=(64, 48), n=14), 10 ** 9)


@pytest.mark.parametrize("name,make", [("root chain", _root_chain_scene), ("chained leaves", chained_scene)])
def test_a_chained_upload_rebuilt_into_hundreds_of_nodes_and_refitted_afterwards(name, make):
    for sched in ("lane", "cu"):
        s = make()
        p = s.default_params(samples=4)
        d = _dev(s, scheduler=sched)
        before = d.bytes
        v, n, sp = large_deformation(s, seed=3, turns=0.5)
        _upd(d, v, n, sp)
        d.rebuild_bvh()
        h = fresh_host(make(), v, n, sp)
        assert h.view.contents.bvh.num_nodes > 100
        fresh = _dev(h, scheduler=sched)
        _same(d.render_to_host(p), fresh.render_to_host(p), (name, sched))
        assert d.bytes == fresh.bytes and d.bytes > before
        # a refit over the new level ranges, no chain records left
        v2, n2, sp2 = deformed(h, seed=4)
        _upd(d, v2, n2, sp2)
        _same(d.render_to_host(p), _dev(apply_host(h, v2, n2, sp2), scheduler=sched).render_to_host(p), (name, sched, "refit"))


def test_a_root_that_is_a_leaf_stays_one():
    for sched in ("lane", "cu"):
        s = single_prim_scene()
        p = s.default_params(samples=4)
        d = _dev(s, scheduler=sched)
        v, n, sp = deformed(s, seed=3)
        _upd(d, v, n, sp)
        d.rebuild_bvh()
        h = fresh_host(single_prim_scene(), v, n, sp)
        assert h.view.contents.bvh.num_nodes == 1
        fresh = _dev(h, scheduler=sched)
        _same(d.render_to_host(p), fresh.render_to_host(p), sched)
        assert d.bytes == fresh.bytes and d.bvh_cost() == pytest.approx(1.0, rel=1e-9)


# ---- 5. queries -------------------------------------------------------------------------------------------------------
def _queries(d, rays, occ_rays):
    r = d.trace_rays(rays, info=True)
    return [getattr(r, k) for k in r.FIELDS] + [d.occluded(occ_rays)]


@pytest.mark.parametrize("make,partly", [(lambda: scenes.config5_scene(res=(96, 54), n=64, tex=64), True),
                                         (lambda: scenes.feature_scene(res=(96, 64)), False)], ids=["config 5 stand-in", "feature"])
def test_queries_after_a_rebuild_are_the_fresh_uploads(make, partly):
    s = make()
    d = _dev(s)
    if partly:    # ~13 700 node records of 64 B: beyond any LDS budget, so the queries stage the top of the tree only
        assert "deep" in d.kernel and s.view.contents.bvh.num_nodes // 2 * 64 > 160 * 1024, d.kernel
    rays = _query_rays(s, 2000, 2000, seed=21)
    occ_rays = rays.copy()
    occ_rays[:, 7] = np.random.default_rng(22).uniform(0.05, 8.0, len(rays)).astype(np.float32)
    before = _queries(d, rays, occ_rays)                   # (the cached query set-up exists now)
    v, n, sp = large_deformation(s, seed=5, turns=0.5)
    _upd(d, v, n, sp)
    d.rebuild_bvh()
    fresh = _dev(fresh_host(make(), v, n, sp))
    got, want = _queries(d, rays, occ_rays), _queries(fresh, rays, occ_rays)
    for a, b in zip(got, want):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    assert not np.array_equal(got[0].view(np.uint32), before[0].view(np.uint32))
    assert (got[1] != -1).sum() > 500


# ---- 6. accumulators --------------------------------------------------------------------------------------------------
def test_progressive_accumulators_refuse_a_rebuilt_scene_until_reset():
    from vimg_amd import hip
    make = lambda: scenes.json_scene("disney_spheres.json", res=(96, 48))   # noqa: E731
    s = make()
    p = s.default_params(samples=1)
    d = _dev(s)
    acc = d.progressive(p)
    acc.render(2)
    d.rebuild_bvh()
    with pytest.raises(hip.HipError, match="scene changed"):
        acc.render(1)
    assert acc.samples == 2
    acc.reset()
    q = p.__class__.from_buffer_copy(p)
    q.samples = 5
    want = d.render(q, stats=False)
    acc.render(2)
    assert np.array_equal(_bits(acc.render(3)), _bits(want))
    assert np.array_equal(_bits(want), _bits(_dev(fresh_host(make())).render(q, stats=False)))


# ---- 7. cost ----------------------------------------------------------------------------------------------------------
def _cost_is(d, host_scene, what):
    want = _tree_cost(host_scene)
    got = d.bvh_cost()
    print(f"{what}: bvh_cost {got!r}, _tree_cost {want!r}")
    assert got == pytest.approx(want, rel=1e-9), what
    assert np.float64(d.bvh_cost()).view(np.uint64) == np.float64(got).view(np.uint64), what     # two calls, the same bits
    return got


def test_cost_of_uploaded_chained_refitted_and_rebuilt_trees():
    make = lambda: scenes.feature_scene(res=(72, 48))    # noqa: E731
    s = make()
    d = _dev(s)
    _cost_is(d, s, "uploaded sweep tree")
    v, n, sp = large_deformation(s, seed=7, turns=0.5)
    _upd(d, v, n, sp)
    _cost_is(d, apply_host(make(), v, n, sp), "after update_geometry")
    d.rebuild_bvh()
    _cost_is(d, fresh_host(make(), v, n, sp), "after rebuild_bvh")
    for name, mk in (("chained leaves", chained_scene), ("root chain", _root_chain_scene)):
        c = mk()
        dc = _dev(c)
        _cost_is(dc, c, name)
        vc, nc, spc = deformed(c, seed=2)
        _upd(dc, vc, nc, spc)
        _cost_is(dc, apply_host(mk(), vc, nc, spc), name + ", refitted")


def test_a_rebuild_undoes_what_a_two_turn_twist_does_to_the_cost():
    """The point of the feature, as an inequality with no measured constant: cost(refit) > cost(rebuilt).
    scenes.config4_scene(res=(96, 54), n_lat=96, env=(64, 32)) (41 667 vertices, the scene of the builder-quality
    test), twisted by two turns about the vertical axis through the vertices' centroid.  With the host's sweep
    builder standing in for PLOC, on the CPU: _tree_cost 8.33 as uploaded, 18.96 after the refit, 9.41 for a fresh
    sweep build of the twisted scene (ratio 2.01).  PLOC is held within 1.05 x the sweep on the undeformed scene by
    an existing test; on the twisted scene the test asserts only the strict inequality."""
    make = lambda: scenes.config4_scene(res=(96, 54), n_lat=96, env=(64, 32))   # noqa: E731
    s = make()
    d = _dev(s)
    v0, n0, _ = s.geometry()
    v = twist(v0, 2.0)
    d.update_geometry(vertices=_cuda(v))
    refit = _cost_is(d, apply_host(make(), v), "config 4, two turns, refit")
    d.rebuild_bvh()
    rebuilt = _cost_is(d, fresh_host(make(), v), "config 4, two turns, rebuilt")
    print(f"config 4, two turns: as uploaded {_tree_cost(s):.4f}, refit {refit:.4f}, rebuilt (PLOC) {rebuilt:.4f}")
    assert refit > rebuilt, (refit, rebuilt)


# ---- 8. a failed call changes nothing ------------------------------------------------------------------------------------
def test_a_refused_rebuild_leaves_the_scene_and_its_accumulators_as_they_were():
    from vimg_amd import abi, hip
    lib = hip._lib()
    s = scenes.json_scene("cornell_box_spheres.json", res=(64, 64))
    p = s.default_params(samples=4)
    d = _dev(s)
    before, cost, size = d.render_to_host(p), d.bvh_cost(), d.bytes
    acc = d.progressive(p)
    acc.render(1)
    bad = abi.RebuildOptions(builder=7)
    assert lib.vimg_hip_scene_rebuild_bvh(d._h, C.byref(bad), None) == -1
    assert b"unknown builder" in lib.vimg_hip_last_error()
    short = abi.RebuildOptions()
    short.struct_size = 4
    assert lib.vimg_hip_scene_rebuild_bvh(d._h, C.byref(short), None) == -1
    with pytest.raises(ValueError):
        d.rebuild_bvh(builder="sweep")
    _same(d.render_to_host(p), before, "after refused rebuilds")
    assert d.bvh_cost() == cost and d.bytes == size
    acc.render(1)                                           # nothing changed: the accumulator goes on
    assert acc.samples == 2
    # NULL options: the PLOC builder
    assert lib.vimg_hip_scene_rebuild_bvh(d._h, None, None) == 0
    _same(d.render_to_host(p), _dev(fresh_host(scenes.json_scene("cornell_box_spheres.json", res=(64, 64)))).render_to_host(p), "NULL options")


# ---- 9. scene bytes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["ploc", "lbvh"])
def test_scene_bytes_after_a_rebuild_are_the_fresh_uploads(builder):
    make = lambda: scenes.big_mesh_scene(res=(96, 64))   # noqa: E731
    s = make()
    d = _dev(s)
    v, n, sp = large_deformation(s, seed=11)
    _upd(d, v, n, sp)
    d.rebuild_bvh(builder=builder)
    fresh = _dev(fresh_host(make(), v, n, sp, builder=builder))
    assert d.bytes == fresh.bytes
    p = s.default_params(samples=2)
    _same(d.render_to_host(p), fresh.render_to_host(p), builder)
