"""Changing a resident scene (vimg_hip_scene_update_geometry, vimg_hip_scene_set_camera; DeviceScene.update_geometry
and .set_camera): after an update a launch reads exactly what an upload of the host scene with the same positions
and a refit tree (HostScene.set_vertices / set_spheres / refit_bvh) reads - so image, event counts, heatmap and
trace_pixel are that upload's bits on every scheduler configuration - and the image is the oracle's on that host
scene.  "fresh" below is that upload."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import scenes
from test_gpu_parity import FEATURE_CASES, SCHEDULES, _compare_images, scheduler_scene
from test_progressive import STATS_FIELDS, _bits
from test_scene_update_host import apply_host, chained_scene, deformed, single_prim_scene, with_python_tree

pytestmark = pytest.mark.gpu

UPDATE_CASES = {**FEATURE_CASES,
                "sphere-light json": lambda: (scenes.json_scene("MIS_light_tests/sphere_light_small_mis.json", res=(64, 64)),
                                              dict(samples=16)),
                "quad-light json": lambda: (scenes.odyssey_without_monolith(res=(64, 48)), dict(samples=8))}


def _dev(s, **opts):
    from vimg_amd import hip
    return hip.DeviceScene(s, **opts)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _update(d, v=None, n=None, sp=None):
    """The update with device tensors (what a caller whose geometry lives on the GPU passes)."""
    d.update_geometry(vertices=None if v is None else _cuda(v), normals=None if n is None else _cuda(n),
                      spheres=None if sp is None or len(sp) == 0 else _cuda(sp))


def _same(a, b, what):
    (ia, sa), (ib, sb) = a, b
    assert np.array_equal(_bits(ia), _bits(ib)), what
    assert {k: getattr(sa, k) for k in STATS_FIELDS} == {k: getattr(sb, k) for k in STATS_FIELDS}, what


def _updated_and_fresh(make, seed, opts=None, scale=0.02):
    """(device scene uploaded from make() and updated with seeded positions, fresh upload of the same, host scene)."""
    opts = opts or {}
    s = make()
    d = _dev(s, **opts)
    v, n, sp = deformed(s, seed, scale)
    _update(d, v, n, sp)
    h = apply_host(make(), v, n, sp)
    return d, _dev(h, **opts), h


@pytest.mark.parametrize("case", list(UPDATE_CASES))
def test_updated_scene_is_the_fresh_upload_on_every_feature(case):
    """Triangle lights baked and with vertex normals, sphere lights, textures, normal maps, thin lens, env maps,
    deep trees, every integrator: image and all eight counters of the fresh upload, and the oracle's image."""
    make = lambda: UPDATE_CASES[case]()[0]              # noqa: E731
    kw = UPDATE_CASES[case]()[1]
    d, fresh, h = _updated_and_fresh(make, seed=5)
    p = h.default_params(**kw)
    got = d.render_to_host(p)
    _same(got, fresh.render_to_host(p), case)
    cpu, cst, _ = O.render(h, p)
    _compare_images(got[0], cpu, f"{case}, updated")
    assert got[1].paths == cst.paths


@pytest.mark.parametrize("scene_name", ["disney_spheres.json", "feature"])
def test_updated_scene_on_every_schedule_heatmap_and_trace_pixel(scene_name):
    s0, p = scheduler_scene(scene_name)
    make = lambda: scheduler_scene(scene_name)[0]       # noqa: E731
    v, n, sp = deformed(s0, seed=9)
    h = apply_host(make(), v, n, sp)
    for name in ("lane", "cu", "cu/nolds", "cu/stack1", "cu/early"):
        d, fresh = _dev(make(), **SCHEDULES[name]), _dev(h, **SCHEDULES[name])
        _update(d, v, n, sp)
        _same(d.render_to_host(p), fresh.render_to_host(p), (scene_name, name))
        assert np.array_equal(_bits(d.render_to_host(p, stats=False)), _bits(fresh.render_to_host(p, stats=False)))
        assert np.array_equal(_bits(d.trace_pixel(p, 17, 23)), _bits(fresh.trace_pixel(p, 17, 23))), (scene_name, name)
        assert np.array_equal(_bits(d.render_heatmap(p)), _bits(fresh.render_heatmap(p))), (scene_name, name)
        d.close()
        fresh.close()


def _root_chain_scene():
    """All ~420 primitives of big_mesh_scene in ONE leaf: the root is a chain of four records."""
    return with_python_tree(scenes.big_mesh_scene(res=(64, 48), n=14), 10 ** 9)


@pytest.mark.parametrize("name,make", [("chained leaves", chained_scene), ("root chain", _root_chain_scene),
                                       ("root leaf", single_prim_scene)])
def test_chains_and_a_root_that_is_a_leaf(name, make):
    for sched in ("lane", "cu"):
        d, fresh, h = _updated_and_fresh(make, seed=3, opts=dict(scheduler=sched))
        p = h.default_params(samples=4)
        _same(d.render_to_host(p), fresh.render_to_host(p), (name, sched))


def test_degenerate_triangle_and_two_updates_in_a_row():
    make = lambda: scenes.feature_scene(res=(72, 48))    # noqa: E731
    s = make()
    p = s.default_params(samples=6, depth=7)
    v0, n0, sp0 = s.geometry()
    d = _dev(s)
    before = d.render_to_host(p)
    # collapse 24 triangles of the textured mesh (mesh 3, behind the three quads) onto points, then restore them
    v = v0.copy()
    view = s.view.contents
    idx = np.ctypeslib.as_array(view.tri_indices, (view.num_tris, 3)).astype(np.int64)
    tri = [t for t in range(view.num_tris) if view.tri_mesh[t] == 3][:24]
    assert tri
    first = view.meshes[3].first_vertex
    for t in tri:
        v[first + idx[t]] = v[first + idx[t][0]]
    _update(d, v)
    collapsed = apply_host(make(), v)
    _same(d.render_to_host(p), _dev(collapsed).render_to_host(p), "collapsed")
    _update(d, v0)
    restored = d.render_to_host(p)
    _same(restored, _dev(apply_host(make(), v0)).render_to_host(p), "restored")
    # A then B: B's fresh upload
    va, na, spa = deformed(s, seed=21)
    vb, nb, spb = deformed(s, seed=22, scale=0.04)
    _update(d, va, na, spa)
    _update(d, vb, nb, spb)
    _same(d.render_to_host(p), _dev(apply_host(make(), vb, nb, spb)).render_to_host(p), "A then B")
    # spheres only, then vertices only (the other table stays as the last update left it)
    _update(d, sp=spa)
    _update(d, v=va)
    _same(d.render_to_host(p), _dev(apply_host(make(), va, nb, spa)).render_to_host(p), "split updates")


def test_numpy_inputs_are_copied_up():
    s = scenes.json_scene("cornell_box_spheres.json", res=(64, 64))
    p = s.default_params(samples=4)
    v, n, sp = deformed(s, seed=4)
    a, b = _dev(s), _dev(s)
    a.update_geometry(vertices=v, normals=n, spheres=sp)
    _update(b, v, n, sp)
    _same(a.render_to_host(p), b.render_to_host(p), "numpy vs tensors")


def test_set_camera_is_the_fresh_upload_with_that_camera():
    from vimg_amd import host, hip
    lib = hip._lib()
    make = lambda: scenes.feature_scene(res=(72, 48))    # noqa: E731
    s = make()
    p = s.default_params(samples=6, depth=7)
    d = _dev(s)
    cam = dict(look_from=(0.4, 1.6, 5.5), look_at=(0.1, 0.5, 0.0), up=(0, 1, 0), vfov_deg=35.0,
               aperture_radius=0.05, focal_dist=5.0)
    d.set_camera(**cam)
    h = make()
    h.set_camera(cam["look_from"], cam["look_at"], cam["up"], cam["vfov_deg"], (72, 48), cam["aperture_radius"],
                 cam["focal_dist"])
    want = _dev(h).render_to_host(p)
    _same(d.render_to_host(p), want, "set_camera")
    # another resolution is refused, and the scene renders what it rendered
    other = host.camera_lookat(cam["look_from"], cam["look_at"], cam["up"], 50.0, (80, 48))
    assert lib.vimg_hip_scene_set_camera(d._h, C.byref(other)) == -1
    assert b"resolution" in lib.vimg_hip_last_error()
    with pytest.raises(hip.HipError, match=r"\[-1\]"):
        d.set_camera(other)
    _same(d.render_to_host(p), want, "after a refused camera")
    # an abi.Camera is taken as it is
    d.set_camera(host.camera_lookat((0, 1, 6), (0, 0.5, 0), (0, 1, 0), 40.0, (72, 48)))
    h2 = make()
    h2.set_camera((0, 1, 6), (0, 0.5, 0), (0, 1, 0), 40.0, (72, 48))
    _same(d.render_to_host(p), _dev(h2).render_to_host(p), "abi.Camera")


def test_progressive_accumulators_refuse_a_changed_scene_until_reset():
    from vimg_amd import hip
    make = lambda: scenes.json_scene("disney_spheres.json", res=(96, 48))   # noqa: E731
    s = make()
    p = s.default_params(samples=1)
    d = _dev(s)
    v, n, sp = deformed(s, seed=8)
    fresh = _dev(apply_host(make(), v, n, sp))
    want = {}
    acc, idle = d.progressive(p), d.progressive(p)
    acc.render(2)
    _update(d, v, n, sp)
    for a in (acc, idle):                       # advanced before the change / created before it
        with pytest.raises(hip.HipError, match="scene changed"):
            a.render(1)
    assert acc.samples == 2
    acc.reset()
    idle.reset()
    for t, k in ((2, 2), (5, 3)):
        q = p.__class__.from_buffer_copy(p)
        q.samples = t
        want[t] = fresh.render(q, stats=False)
        assert np.array_equal(_bits(acc.render(k)), _bits(want[t])), t
    assert np.array_equal(_bits(idle.render(5)), _bits(want[5]))
    # a camera change refuses them too
    d.set_camera((0, 1, 6), (0, 0.5, 0), (0, 1, 0), 40.0)
    with pytest.raises(hip.HipError, match="scene changed"):
        acc.render(1)
    acc.reset()
    acc.render(1)
    # a refused change is no change
    lib = hip._lib()
    assert lib.vimg_hip_scene_set_camera(d._h, None) == -1
    acc.render(1)
    assert acc.samples == 2


def test_bad_arguments_leave_the_scene_as_it_was():
    import torch
    from vimg_amd import abi, hip
    lib = hip._lib()
    s = scenes.json_scene("cornell_box_spheres.json", res=(64, 64))
    p = s.default_params(samples=4)
    d = _dev(s)
    before = d.render_to_host(p)
    v, n, sp = deformed(s, seed=2)
    upd = abi.GeometryUpdate(vertices=_cuda(v).data_ptr())
    assert lib.vimg_hip_scene_update_geometry(None, C.byref(upd), None) == -1
    assert lib.vimg_hip_scene_update_geometry(d._h, None, None) == -1
    short = abi.GeometryUpdate(vertices=_cuda(v).data_ptr())
    short.struct_size = 8
    assert lib.vimg_hip_scene_update_geometry(d._h, C.byref(short), None) == -1
    assert b"struct_size" in lib.vimg_hip_last_error()
    assert lib.vimg_hip_scene_set_camera(None, None) == -1
    assert lib.vimg_hip_scene_set_camera(d._h, None) == -1
    # the Python layer checks shape, dtype, device and contiguity before anything is called
    for kw in (dict(vertices=_cuda(v[:-1])), dict(vertices=_cuda(v).double()), dict(vertices=torch.from_numpy(v)),
               dict(vertices=_cuda(np.ascontiguousarray(v.T)).T), dict(normals=_cuda(n[:, :2])),
               dict(spheres=_cuda(sp[:, :3])), dict(spheres=sp.astype(np.float64)), dict(vertices=v.tolist())):
        with pytest.raises(ValueError):
            d.update_geometry(**kw)
    _same(d.render_to_host(p), before, "after refused updates")
    acc = d.progressive(p)
    acc.render(1)
    with pytest.raises(ValueError):
        d.update_geometry(vertices=_cuda(v[:5]))
    acc.render(1)                               # nothing changed: the accumulator goes on
    assert acc.samples == 2
