"""The launch-constant shading tables of a small scene served from LDS (render_kernels.h: LdsTables,
render_cu_kernel.h: stage_tables, launch_policy.hip): the PLAIN builds of render_cu_kernel read the hit-record
tables from copies each workgroup makes when a launch starts.  The values are the same words read from
another address space, so every frame must be, bit for bit, the frame of the same scene uploaded under
VIMG_HIP_LDS_TABLES=0 (tables in global memory: the general build), under VIMG_HIP_PLAIN=0 (never a PLAIN build) and
the CPU oracle's; the copies are made anew by every launch, so an edited scene needs nothing more; a scene whose
tables do not fit runs the general build; and options that leave a launch no room are an error, not a failed launch."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import scenes
import vimg_amd
from vimg_amd import abi

pytestmark = pytest.mark.gpu

PLAIN_NAME, GENERAL_NAME = "render_cu_kernel<false>", "render_cu_kernel<false,general>"
RES, SPP = (64, 48), 8
SCENES = {"disney_spheres": "disney_spheres.json", "cornell_box_spheres": "cornell_box_spheres.json",
          "glass_in_box": "glass_in_box.json", "sphere_light": "MIS_light_tests/sphere_light_small_mis.json"}


def _dev(s, tables=True, general=False, **opts):
    """A resident scene.  Both overrides are read once, at upload: tables=False uploads under VIMG_HIP_LDS_TABLES=0,
    general=True under VIMG_HIP_PLAIN=0."""
    from vimg_amd import hip
    hip.init(0)
    want = {"VIMG_HIP_LDS_TABLES": None if tables else "0", "VIMG_HIP_PLAIN": "0" if general else None}
    old = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        return hip.DeviceScene(s, **opts)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _frame(d, p):
    """A frame without statistics: the timed build of the launch (PLAIN or general)."""
    import torch
    img = d.render(p, stats=False)
    torch.cuda.synchronize()
    d.check()
    return img.cpu().numpy()


def _three(s, **opts):
    """The scene with its tables staged, under VIMG_HIP_LDS_TABLES=0 and under VIMG_HIP_PLAIN=0."""
    return _dev(s, **opts), _dev(s, tables=False, **opts), _dev(s, general=True, **opts)


@pytest.fixture(scope="module")
def oracle_frames():
    """The oracle's frame and event counts per (scene, integrator), computed once."""
    cache = {}

    def get(name, integrator):
        if (name, integrator) not in cache:
            s = scenes.json_scene(SCENES[name], res=RES)
            img, st, _ = O.render(s, s.default_params(samples=SPP, integrator=integrator))
            cache[(name, integrator)] = (img, st)
        return cache[(name, integrator)]
    return get


@pytest.mark.parametrize("integrator", ["mis", "material"])
@pytest.mark.parametrize("name", list(SCENES))
def test_staged_tables_render_the_bits_of_global_tables_and_of_the_oracle(name, integrator, oracle_frames):
    """Frames without statistics (the PLAIN build with its tables in LDS against the general build twice over) and
    statistics launches (the statistics build on all three, which keeps its tables in global memory): one image, one
    set of event counts, and the image is the oracle's."""
    s = scenes.json_scene(SCENES[name], res=RES)
    p = s.default_params(samples=SPP, integrator=integrator)
    staged, off, general = _three(s)
    assert staged.kernel_for(p) == (PLAIN_NAME if integrator == "mis" else GENERAL_NAME)
    assert off.kernel_for(p) == GENERAL_NAME and general.kernel_for(p) == GENERAL_NAME
    a, b, c = _frame(staged, p), _frame(off, p), _frame(general, p)
    cpu, cst = oracle_frames(name, integrator)
    exact = (_bits(a) == _bits(cpu)).all(axis=-1).mean()
    print(f"{name} {integrator}: {exact * 100:.3f} % of the pixels are the oracle's bits, max |diff| {np.abs(a - cpu).max():.3e}")
    assert np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    assert np.array_equal(_bits(a), _bits(cpu))
    counts = []
    for d in (staged, off, general):
        img, st = d.render_to_host(p)
        assert np.array_equal(_bits(img), _bits(a))
        counts.append(st.as_dict())
    assert counts[0] == counts[1] == counts[2] and counts[0]["closest_rays"] > 0
    assert counts[0]["paths"] == cst.paths
    for d in (staged, off, general):
        d.close()


def test_the_late_ray_build_reads_its_tables_from_lds_too():
    """Which build a case of this file runs: at 64 x 48 every pixel of a launch owns a slot, so the policy queues rays
    early and every other case here runs k_cu_plain_early.hip (against k_cu_early.hip).  The build whole frames are
    timed on, k_cu_plain.hip, runs where a compute unit has more than three pools' worth of pixels: disney_spheres at
    its own 1800 x 800 (5 625 pixels per compute unit against 3 x 1 280 slots), here at 2 spp, against the general
    build k_cu.hip under either override.  Compared on the GPU."""
    import torch
    s = scenes.json_scene(SCENES["disney_spheres"])
    p = s.default_params(samples=2)
    staged, off, general = _three(s)
    assert staged.kernel_for(p) == PLAIN_NAME and off.kernel_for(p) == GENERAL_NAME and general.kernel_for(p) == GENERAL_NAME
    a, b, c = (d.render(p, stats=False) for d in (staged, off, general))
    torch.cuda.synchronize()
    for d in (staged, off, general):
        d.check()
    assert bool(torch.isfinite(a).all()) and float(a.max()) > 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    for d in (staged, off, general):
        d.close()


def test_a_shard_and_a_progressive_pair_of_increments(oracle_frames):
    """tile_world = 4 (a shard's pixels all own a slot: the early-ray builds) and 4 + 4 samples added in two launches."""
    import torch
    s = scenes.json_scene(SCENES["disney_spheres"], res=RES)
    staged, off, general = _three(s)
    p = s.default_params(samples=SPP, tile_world=4, tile_rank=1)
    assert staged.kernel_for(p) == PLAIN_NAME and off.kernel_for(p) == GENERAL_NAME
    a, b, c = _frame(staged, p), _frame(off, p), _frame(general, p)
    assert a.ndim == 2 and a.max() > 0
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    outs = []
    for d in (staged, off):
        acc = d.progressive(s.default_params(samples=1))
        acc.render(4)
        img = acc.render(4)
        torch.cuda.synchronize()
        d.check()
        outs.append(img.cpu().numpy())
        acc.close()
    cpu, _ = oracle_frames("disney_spheres", "mis")
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])) and np.array_equal(_bits(outs[0]), _bits(cpu))
    for d in (staged, off, general):
        d.close()


def test_an_edited_scene_is_the_fresh_upload_without_new_code():
    """Every launch copies the resident tables as they stand: after update_materials (types change too),
    update_geometry and set_camera the next frame is the frame of a fresh upload of the host scene edited the same
    way, with its tables staged and under VIMG_HIP_LDS_TABLES=0."""
    from test_scene_relight import TYPE_EDITS
    from test_scene_relight_host import edited_materials
    from test_scene_update_host import apply_host, deformed
    make = lambda: scenes.json_scene(SCENES["disney_spheres"], res=RES)     # noqa: E731
    s = make()
    p = s.default_params(samples=SPP)
    d = _dev(s)
    before = _frame(d, p)

    def same_as_fresh(h, what):
        assert d.kernel_for(p) == PLAIN_NAME, what
        got = _frame(d, p)
        fresh, fresh_off = _dev(h), _dev(h, tables=False)
        assert np.array_equal(_bits(got), _bits(_frame(fresh, p))), what
        assert np.array_equal(_bits(got), _bits(_frame(fresh_off, p))), what
        fresh.close(), fresh_off.close()
        return got

    h = make()
    h.set_materials(edited_materials(h, TYPE_EDITS))
    d.update_materials(materials=h.materials())
    edited = same_as_fresh(h, "update_materials")
    assert not np.array_equal(_bits(edited), _bits(before))
    v, n, sp = deformed(h, seed=11)
    d.update_geometry(vertices=v, normals=n, spheres=sp)
    apply_host(h, v, n, sp)
    moved = same_as_fresh(h, "update_geometry")
    assert not np.array_equal(_bits(moved), _bits(edited))
    cam = dict(look_from=(0.5, 2.5, 7.0), look_at=(0.0, 0.5, 0.0), up=(0, 1, 0), vfov_deg=35.0)
    d.set_camera(**cam)
    h.set_camera(cam["look_from"], cam["look_at"], cam["up"], cam["vfov_deg"], RES)
    turned = same_as_fresh(h, "set_camera")
    assert not np.array_equal(_bits(turned), _bits(moved))
    cpu, _, _ = O.render(h, p)
    assert np.array_equal(_bits(turned), _bits(cpu))
    d.close()


def _filled_scene(n_spheres, n_materials, res=RES):
    """n_spheres spheres over a floor sphere under a sphere light, and a material table of n_materials records (the
    spheres use them in turn; the others only take their place in the tables)."""
    s = vimg_amd.HostScene()
    s.set_camera((0.0, 3.0, 9.0), (0.0, 0.6, 0.0), (0, 1, 0), 40.0, res)
    s.set_render_defaults("mis", SPP, 8)
    t = [s.add_texture_const(c) for c in ((0.7, 0.6, 0.5), (0.3, 0.5, 0.8))]
    m_light = s.add_material("diffuse_light", emit=(14.0, 13.0, 11.0))
    mats = [s.add_material("principled", tex=t[i % 2], metallic=0.1 * (i % 7), roughness=0.2 + 0.1 * (i % 5), clearcoat=0.5)
            if i % 2 else s.add_material("lambertian", tex=t[i % 2]) for i in range(n_materials)]
    s.add_sphere((0.0, -1000.0, 0.0), 1000.0, mats[0])
    s.add_sphere((0.0, 6.0, 1.0), 1.0, m_light)
    for i in range(n_spheres):
        s.add_sphere(((i % 8 - 3.5) * 0.9, 0.35 + 0.75 * (i // 8 % 2), (i // 16) * 0.9 - 1.0), 0.35, mats[(1 + i) % n_materials])
    s.build_bvh(abi.BVH_SWEEP)
    return s


def test_one_primitive_more_than_fits_runs_the_general_build():
    """The policy stages the tables in the room the pool leaves and never shrinks the pool for them.  A scene's hit
    records are a few KB at most (the leaves of a PLAIN launch are in LDS: 85 primitives), so the room is made scarce
    instead: a tree as deep as it has primitives under sixteen walking waves (30 stack rows of 4 KB), a frame with more
    pixels per compute unit than slots fit, and pool_slots by name, which lifts the policy's cap of 1 280.  The
    boundary is found through kernel_for alone: the largest pool beside which the tables of 26 spheres still fit.
    Beside that pool the scene runs the PLAIN build and the scene with one sphere more the general build (64 slots
    fewer show that the primitives alone were not the reason), and both are the oracle's bits."""
    res, spp = (480, 320), 4
    cb = _caterpillar_builder()

    def scene(n_spheres):
        s = _filled_scene(n_spheres, 2, res)
        s.build_bvh_with(C.cast(cb, C.c_void_p))
        assert s.view.contents.bvh.max_depth + 2 <= 32       # (every stack row in LDS: not the DEEP build)
        return s

    def plain(s, slots):
        d = _dev(s, cu_walkers=16, pool_slots=slots)
        name = d.kernel_for(s.default_params(samples=spp))
        d.close()
        assert name in (PLAIN_NAME, GENERAL_NAME)
        return name == PLAIN_NAME

    fits, more = scene(26), scene(27)
    lo, hi = 1, 64             # pool slots in eights: 8 fit beside the tables, 512 do not fit the LDS at all
    assert plain(fits, 8 * lo) and not plain(fits, 8 * hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plain(fits, 8 * mid) else (lo, mid)
    slots = 8 * lo
    assert slots > 64 and plain(more, slots - 64), "the primitives alone must not be what sends the launch to the general build"
    for s, want in ((fits, PLAIN_NAME), (more, GENERAL_NAME)):
        p = s.default_params(samples=spp)
        d = _dev(s, cu_walkers=16, pool_slots=slots)
        assert d.kernel_for(p) == want
        gpu = _frame(d, p)
        cpu, _, _ = O.render(s, p)
        exact = (_bits(gpu) == _bits(cpu)).all(axis=-1).mean()
        print(f"{s.view.contents.num_prims} primitives beside {slots} slots, {want}: {exact * 100:.3f} % of the pixels are the oracle's bits")
        assert np.array_equal(_bits(gpu), _bits(cpu))
        d.close()


def _caterpillar_builder():
    """A caller's builder whose tree is as deep as the scene has primitives: every internal node has one leaf child."""
    BUILDER = C.CFUNCTYPE(C.c_int, C.c_uint32, abi.Pf32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                          C.c_void_p, abi.Pf32, C.POINTER(C.c_uint32))

    def build(n, bounds6, num_nodes, max_depth, nodes_p, bb_p, obj_p):
        b = np.ctypeslib.as_array(bounds6, (n, 6)).copy()
        nodes = np.ctypeslib.as_array(C.cast(nodes_p, C.POINTER(C.c_uint32)), (2 * n - 1, 2))
        bb = np.ctypeslib.as_array(bb_p, (2 * (2 * n - 1) + 3, 3))
        obj = np.ctypeslib.as_array(obj_p, (n,))
        order = np.argsort(b[:, 0] + b[:, 3], kind="stable")
        obj[:] = order
        bb[0], bb[2] = b[:, :3].min(0), b[:, 3:].max(0)
        node, nxt = 0, 1
        for i in range(n - 1):
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
    return BUILDER(build)


def test_options_beyond_the_compute_units_lds_are_an_error_not_a_failed_launch():
    """lds_budget_kb on a tree of thousands of nodes, lds_stack on a tree 80 levels deep: what the policy chooses
    itself gives way first (the stacks, the node cache), and a launch that still cannot fit is VIMG_E_INVALID naming
    the option, found before anything is enqueued - the scene's error word stays clean, kernel_for names no kernel,
    and the same scene with the option left to the policy renders."""
    from vimg_amd import hip
    big = scenes.big_mesh_scene(res=RES, n=64)
    assert big.view.contents.bvh.num_nodes > 2 * 3200      # internal nodes x 56 bytes: beyond 160 KB on their own
    deep = _filled_scene(78, 2)
    cb = _caterpillar_builder()
    deep.build_bvh_with(C.cast(cb, C.c_void_p))
    assert 64 < deep.view.contents.bvh.max_depth <= 92
    for s, opts, option in ((big, dict(lds_budget_kb=100000), "lds_budget_kb"), (deep, dict(lds_stack=92), "lds_stack")):
        p = s.default_params(samples=2)
        d = _dev(s, scheduler="cu", **opts)
        assert d.kernel_for(p) == ""
        with pytest.raises(hip.HipError, match=rf"^\[-1\] .*{option}"):
            d.render(p, stats=False)
        with pytest.raises(hip.HipError, match=rf"^\[-1\] .*{option}"):
            d.trace_pixel(p, 3, 3)
        d.check()
        d.close()
        ok = _dev(s, scheduler="cu")
        assert "deep" in ok.kernel_for(p)
        img = _frame(ok, p)
        assert np.isfinite(img).all() and img.max() > 0
        ok.close()
