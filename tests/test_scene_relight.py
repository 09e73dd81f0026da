"""Editing a resident scene's materials, lights and textures in place (the material fields of
vimg_hip_scene_update_geometry; DeviceScene.update_materials and .update_from): after the edit a launch reads exactly
what a fresh upload of the equally edited host scene reads - so image, all eight counters (with and without statistics),
heatmap, trace_pixel and scene_bytes are that upload's bits - and the image is the oracle's on that host scene.
"fresh" below is a new DeviceScene of the edited HostScene with the same options."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import scenes
from test_gpu_parity import FEATURE_CASES, SCHEDULES, _compare_images   # noqa: F401  (FEATURE_CASES: the shared sizes)
from test_progressive import STATS_FIELDS, _bits
from test_scene_relight_host import (ENV_SHAPE, F_MAT, F_TEX, IMG_SHAPE, LIGHT, TOGGLES, _new_image, between_scene,
                                     built_with, cornell_api, edited_materials)
from test_scene_update_host import apply_host, deformed

pytestmark = pytest.mark.gpu


def _dev(s, **opts):
    from vimg_amd import hip
    return hip.DeviceScene(s, **opts)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _same(a, b, what):
    (ia, sa), (ib, sb) = a, b
    assert np.array_equal(_bits(ia), _bits(ib)), what
    assert {k: getattr(sa, k) for k in STATS_FIELDS} == {k: getattr(sb, k) for k in STATS_FIELDS}, what


def _same_renders(d, fresh, p, what):
    """Image and counters with statistics, image without, and the bytes the scene counts."""
    got = d.render_to_host(p)
    _same(got, fresh.render_to_host(p), what)
    assert np.array_equal(_bits(d.render_to_host(p, stats=False)), _bits(fresh.render_to_host(p, stats=False))), what
    assert d.bytes == fresh.bytes, what
    return got


def _same_everything(d, fresh, p, what):
    got = _same_renders(d, fresh, p, what)
    assert np.array_equal(_bits(d.render_heatmap(p)), _bits(fresh.render_heatmap(p))), what
    assert np.array_equal(_bits(d.trace_pixel(p, 17, 23)), _bits(fresh.trace_pixel(p, 17, 23))), what
    return got


def _oracle(got, h, p, what):
    cpu, cst, _ = O.render(h, p)
    _compare_images(got[0], cpu, what)
    assert got[1].paths == cst.paths


# ---- 1. values ---------------------------------------------------------------------------------------------------
def _edit_cornell_values(h):
    h.set_texture_colors(0, (0.2, 0.6, 0.7))                 # white's, red's base colour
    h.set_texture_colors(1, (0.8, 0.7, 0.1))
    mats = h.materials()
    mats[3].emit[0], mats[3].emit[1], mats[3].emit[2] = 9.0, 14.0, 20.0
    h.set_materials(mats)
    return h


def _edit_feature_values(h):
    h.set_texture_colors(F_TEX["white"], (0.3, 0.7, 0.4))
    h.set_texture_colors(F_TEX["blue"], (0.9, 0.4, 0.1))
    h.set_texture_colors(F_TEX["checker"], (0.9, 0.2, 0.1), (0.1, 0.2, 0.9), 5, 3)
    mats = h.materials()
    for i, k in ((F_MAT["tex"], 1.0), (F_MAT["glass"], 0.6)):
        m = mats[i]
        m.metallic_factor, m.roughness_factor = 0.35 * k, 0.3 + 0.2 * k
        m.specular_transmission, m.subsurface, m.specular, m.specular_tint = 0.5 * k, 0.4, 0.7, 0.3
        m.anisotropic, m.sheen, m.sheen_tint, m.clearcoat, m.clearcoat_gloss, m.eta = 0.5, 0.6, 0.2, 0.8 * k, 0.7, 1.33
    mats[F_MAT["diel"]].ior = 1.8
    e = mats[F_MAT["light"]].emit
    e[0], e[1], e[2] = 4.0, 9.0, 15.0
    h.set_materials(mats)
    return h


VALUE_CASES = {"cornell": (lambda: scenes.json_scene("cornell_box_spheres.json", res=(64, 64)), _edit_cornell_values, dict(samples=8)),
               "feature": (lambda: scenes.feature_scene(res=(72, 48)), _edit_feature_values, dict(samples=6, depth=7))}


@pytest.mark.parametrize("case", list(VALUE_CASES))
def test_edited_values_are_the_fresh_upload(case):
    make, edit, kw = VALUE_CASES[case]
    d = _dev(make())
    h = edit(make())
    p = h.default_params(**kw)
    before = d.render_to_host(p, stats=False)
    d.update_from(h)
    fresh = _dev(h)
    got = _same_everything(d, fresh, p, case)
    assert not np.array_equal(_bits(got[0]), _bits(before)), case        # the edit is visible
    _oracle(got, h, p, f"{case}, edited values")


# ---- 2. types ----------------------------------------------------------------------------------------------------
TYPE_EDITS = {0: ("principled", dict(tex=0, roughness=0.4, metallic=0.6)),       # white walls
              4: ("lambertian", dict(tex=3)),                                    # d_1 (its own constant texture)
              5: ("dielectric", dict(ior=1.45)),                                 # d_2
              6: ("lambertian", dict(tex=5)),                                    # d_3
              1: ("dielectric", dict(ior=1.2))}                                  # the red wall
TYPE_SCHEDULES = ("lane", "cu", "cu/nolds", "cu/early", "cu/1class", "cu/2class")


@pytest.mark.parametrize("sched", TYPE_SCHEDULES)
def test_changed_material_types_on_the_schedules_and_after_a_rebuild(sched):
    """A stale class in a leaf slot would route hits into the wrong vertex queue; rebuild_bvh carries the classes over."""
    from vimg_amd import hip
    make = lambda: scenes.json_scene("disney_spheres.json", res=(96, 48))     # noqa: E731
    s = make()
    p = s.default_params(samples=8)
    d = _dev(s, **SCHEDULES[sched])
    h = make()
    h.set_materials(edited_materials(h, TYPE_EDITS))
    d.update_materials(materials=h.materials())
    fresh = _dev(h, **SCHEDULES[sched])
    _same_renders(d, fresh, p, sched)
    d.rebuild_bvh("ploc")
    h.build_bvh_with(hip.ploc_builder())
    rebuilt = _dev(h, **SCHEDULES[sched])
    _same_renders(d, rebuilt, p, (sched, "rebuilt"))


# ---- 3. lights ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TOGGLES))
def test_emissive_toggles_with_the_new_emitter_list(name):
    make, edits = TOGGLES[name]
    s = make()
    d = _dev(s)
    h = make()
    h.set_materials(edited_materials(h, edits))
    assert len(h.lights()) != len(s.lights()) or "moved" in name          # the list shrinks or grows
    d.update_materials(materials=h.materials(), lights=list(h.lights()))
    # (mis samples an emitter at every diffuse vertex: a scene left without one is rendered by the material integrator,
    # and what mis answers there is test_an_empty_emitter_list_then_a_mis_render's)
    p = h.default_params(samples=8, depth=7, integrator=None if len(h.lights()) else "material")
    got = _same_everything(d, _dev(h), p, name)
    _oracle(got, h, p, name)
    # the edited host scene is the scene built with those materials (test_scene_relight_host.py): so is the upload
    _same(got, _dev(built_with(make, edits)).render_to_host(p), name + ", built")


def test_an_empty_emitter_list_then_a_mis_render():
    """With no emitter the reference's GroupOfEmitters::sample indexes entry -1 of an empty list, so the library
    answers a mis launch on such a scene with VIMG_E_INVALID before any kernel runs, and the oracle has no image to
    give.  "Equals fresh" for the mis render is therefore the fresh upload's answer, message included, with the
    scene untouched by the refusal; the material integrator, which samples no emitter, gives the bits to compare."""
    from vimg_amd import hip
    make = lambda: cornell_api(res=(64, 64))        # noqa: E731
    edits = TOGGLES["cornell: quad light turned off"][1]
    d = _dev(make())
    h = make()
    h.set_materials(edited_materials(h, edits))
    assert len(h.lights()) == 0
    d.update_materials(materials=h.materials(), lights=[])
    fresh = _dev(h)
    p = h.default_params(samples=8, integrator="mis")
    answers = []
    for scene in (d, fresh):
        with pytest.raises(hip.HipError, match=r"\[-1\] mis integrator needs at least one light") as e:
            scene.render_to_host(p)
        answers.append(str(e.value))
    assert answers[0] == answers[1]
    pm = h.default_params(samples=8, integrator="material")
    got = _same_everything(d, fresh, pm, "no emitters")
    _oracle(got, h, pm, "no emitters")
    # and a list again: the original scene, under mis
    o = make()
    d.update_materials(materials=o.materials(), lights=list(o.lights()))
    _same_everything(d, _dev(o), p, "emitters again")


def test_a_light_made_lambertian_without_a_new_list_contributes_zero():
    """The emitter stays in the list (it is still sampled) with zero emission: the upload of the same TABLES - the new
    materials under the old emitter list - which no construction produces, so the fresh scene is made by hand."""
    from vimg_amd import abi, hip
    make = lambda: cornell_api(res=(64, 64))        # noqa: E731
    s = make()
    d = _dev(s)
    mats = edited_materials(s, TOGGLES["cornell: quad light turned off"][1])
    d.update_materials(materials=mats)
    h = make()
    old_lights = h.lights()
    h.set_materials(mats)
    view = abi.Scene.from_buffer_copy(h.view.contents)           # the edited tables, the emitter list as it was
    view.lights = C.cast(old_lights, C.POINTER(abi.Light))
    view.num_lights = len(old_lights)
    hd = C.c_void_p()
    lib = hip._lib()
    assert lib.vimg_hip_scene_upload_opts(C.byref(view), None, C.byref(hd)) == 0
    try:
        p = h.default_params(samples=8)
        w, ht = h.resolution
        want = np.empty((ht, w, 3), np.float32)
        wst = abi.RenderStats()
        assert lib.vimg_hip_render_to_host(hd, C.byref(p), want.ctypes.data_as(abi.Pf32), C.byref(wst)) == 0
        got = d.render_to_host(p)
        _same(got, (want, wst), "stale light")
        assert d.bytes == int(lib.vimg_hip_scene_bytes(hd))
        assert float(got[0].max()) == 0.0                         # nothing emits: the sampled light gives zero
        cpu = np.zeros_like(want)
        cst = abi.RenderStats()
        assert O.load().oracle_render(C.byref(view), C.byref(p), 0, cpu.ctypes.data_as(abi.Pf32), C.byref(cst)) >= 0
        _compare_images(got[0], cpu, "stale light, oracle")
    finally:
        lib.vimg_hip_scene_free(hd)


# ---- 4. images ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["tensor", "numpy"])
def test_swapped_images_and_back(source):
    make = lambda: scenes.feature_scene(res=(72, 48))        # noqa: E731
    s = make()
    p = s.default_params(samples=6, depth=7)
    d = _dev(s)
    original = d.render_to_host(p)
    env, img = _new_image(ENV_SHAPE, 31), _new_image(IMG_SHAPE, 32)
    up = _cuda if source == "tensor" else (lambda a: a)
    d.update_materials(images={F_TEX["env"]: up(env), F_TEX["img"]: up(img)})
    h = make()
    h.set_texture_image(F_TEX["env"], env)
    h.set_texture_image(F_TEX["img"], img)
    got = _same_everything(d, _dev(h), p, source)
    assert not np.array_equal(_bits(got[0]), _bits(original[0]))
    _oracle(got, h, p, f"swapped images ({source})")
    # the original images again (read back from the host scene's level 0): the original upload's render
    v = s.view.contents
    for t, shape in ((F_TEX["env"], ENV_SHAPE), (F_TEX["img"], IMG_SHAPE)):
        off = int(v.textures[t].level_offset[0]) * 3
        level0 = np.ctypeslib.as_array(v.texels, (int(v.num_texels) * 3,))[off:off + int(np.prod(shape))].reshape(shape).copy()
        d.update_materials(images={t: up(level0)})
    _same(d.render_to_host(p), original, "swapped back")


# ---- 5. family flip ----------------------------------------------------------------------------------------------
def _spare_image_scene(use_image=False, res=(64, 48)):
    """A box corner with a sphere under a quad light; texture 1 is an image no material uses unless `use_image`."""
    from vimg_amd import abi, host
    s = host.HostScene()
    s.set_camera((0.0, 1.2, 4.5), (0.0, 0.5, 0.0), (0, 1, 0), 40.0, res)
    s.set_render_defaults("mis", 8, 8)
    t_c = s.add_texture_const((0.7, 0.7, 0.6))
    t_i = s.add_texture_image(_new_image((8, 16, 3), 5), abi.WRAP_REPEAT, abi.WRAP_CLAMP)
    m_floor = s.add_material("lambertian", tex=t_i if use_image else t_c)
    m_ball = s.add_material("principled", tex=t_c, roughness=0.3)
    m_light = s.add_material("diffuse_light", emit=(10, 10, 10))
    v, idx, nrm, uv = scenes._grid_mesh(2, 2.0, lambda x, z: 0.0 * x)
    s.add_mesh(v, idx, m_floor, normals=None, uv_sets=[uv], color_uv=0)
    s.add_sphere((0.0, 0.6, 0.0), 0.6, m_ball)
    lv = np.array([[-0.5, 2.5, -0.5], [0.5, 2.5, -0.5], [0.5, 2.5, 0.5], [-0.5, 2.5, 0.5]], np.float32)
    s.add_mesh(lv, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), m_light)
    s.set_background_const((0, 0, 0), add_to_lights=False)
    s.build_bvh(abi.BVH_SWEEP)
    return s


def test_pointing_a_material_at_an_image_flips_the_kernel_family_and_back():
    plain, textured = _spare_image_scene(False), _spare_image_scene(True)
    p = plain.default_params(samples=8)
    d = _dev(_spare_image_scene(False))
    assert "<false" in d.kernel and "<false" in d.kernel_for(p)
    d.update_materials(materials=textured.materials())
    fresh = _dev(textured)
    assert "<true" in d.kernel and d.kernel == fresh.kernel and d.kernel_for(p) == fresh.kernel_for(p)
    got = _same_everything(d, fresh, p, "to TEX")
    _oracle(got, textured, p, "to TEX")
    d.update_materials(materials=plain.materials())
    fresh = _dev(plain)
    assert "<false" in d.kernel and d.kernel == fresh.kernel and d.kernel_for(p) == fresh.kernel_for(p)
    _same_everything(d, fresh, p, "back to non-TEX")


# ---- 6. background -----------------------------------------------------------------------------------------------
def test_background_rotation_scale_and_constant_colour():
    a = np.deg2rad(70.0)
    rot = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]], np.float32)
    make = lambda: scenes.feature_scene(res=(72, 48))        # noqa: E731
    h = make()
    h.set_background(world_to_env=rot.T.reshape(16), env_to_world=np.linalg.inv(rot).T.astype(np.float32).reshape(16),
                     radiance_scale=1.7)
    p = h.default_params(samples=6, depth=7)
    d = _dev(make())
    before = d.render_to_host(p, stats=False)
    d.update_materials(background=h.background())
    got = _same_everything(d, _dev(h), p, "env rotation")
    assert not np.array_equal(_bits(got[0]), _bits(before))
    _oracle(got, h, p, "env rotation")
    # a constant background that is a light: another colour; then black (no longer emissive, still in the list)
    make = lambda: scenes.feature_scene(res=(72, 48), envmap=False, lens=False)      # noqa: E731
    d = _dev(make())
    for col in ((0.9, 0.3, 0.1), (0.0, 0.0, 0.0)):
        h = make()
        h.set_background(col=col)
        d.update_materials(background=h.background())
        got = _same_everything(d, _dev(h), p, ("constant", col))
        _oracle(got, h, p, f"constant background {col}")


# ---- 7. one call -------------------------------------------------------------------------------------------------
def test_positions_materials_and_lights_in_one_call():
    make, edits = TOGGLES["feature: mesh with vertex normals made emissive"]
    make = lambda: scenes.feature_scene(res=(72, 48))        # noqa: E731
    s = make()
    d = _dev(s)
    v, n, sp = deformed(s, seed=6, scale=0.02)
    h = make()
    h.set_materials(edited_materials(h, edits))
    apply_host(h, v, n, sp)
    d.update_materials(materials=h.materials(), lights=list(h.lights()), vertices=_cuda(v), normals=_cuda(n), spheres=_cuda(sp))
    p = h.default_params(samples=6, depth=7)
    got = _same_everything(d, _dev(h), p, "one call")
    _oracle(got, h, p, "one call")


# ---- 8. progressive ----------------------------------------------------------------------------------------------
def test_an_accumulator_refuses_an_edited_scene_until_reset():
    from vimg_amd import hip
    make, edits = TOGGLES["cornell: a quad and a sphere turned into lights"]
    s = make()
    d = _dev(s)
    p = s.default_params(samples=8)
    acc = d.progressive(p)
    acc.render(2)
    h = make()
    h.set_materials(edited_materials(h, edits))
    d.update_from(h)
    with pytest.raises(hip.HipError, match=r"\[-1\]"):
        acc.render(1)
    assert acc.samples == 2
    acc.reset()
    acc.render(4)
    img = acc.render(4)
    assert np.array_equal(_bits(img), _bits(_dev(h).render(p, stats=False)))


# ---- 9. compatibility and errors ---------------------------------------------------------------------------------
def test_the_32_byte_struct_is_todays_update_and_40_bytes_are_refused():
    from vimg_amd import abi, hip
    lib = hip._lib()
    make = lambda: scenes.json_scene("cornell_box_spheres.json", res=(64, 64))       # noqa: E731
    s = make()
    p = s.default_params(samples=4)
    v, n, sp = deformed(s, seed=4)
    a, b = _dev(s), _dev(s)
    tv = _cuda(v)
    old = abi.GeometryUpdateV1(vertices=tv.data_ptr())
    assert old.struct_size == 32
    assert lib.vimg_hip_scene_update_geometry(a._h, C.cast(C.byref(old), C.POINTER(abi.GeometryUpdate)), None) == 0
    b.update_geometry(vertices=tv)
    _same(a.render_to_host(p), b.render_to_host(p), "v1 struct")
    _same(a.render_to_host(p), _dev(apply_host(make(), v)).render_to_host(p), "v1 struct, fresh")
    # a V1 caller's bytes behind its struct are never read: garbage there changes nothing
    buf = (C.c_uint8 * C.sizeof(abi.GeometryUpdate))(*([0xAB] * C.sizeof(abi.GeometryUpdate)))
    C.memmove(buf, C.byref(old), 32)
    assert lib.vimg_hip_scene_update_geometry(a._h, C.cast(buf, C.POINTER(abi.GeometryUpdate)), None) == 0
    _same(a.render_to_host(p), b.render_to_host(p), "v1 struct with bytes behind it")
    before = a.render_to_host(p)
    mid = abi.GeometryUpdate(vertices=tv.data_ptr())
    mid.struct_size = 40
    assert lib.vimg_hip_scene_update_geometry(a._h, C.byref(mid), None) == -1
    assert b"struct_size" in lib.vimg_hip_last_error()
    _same(a.render_to_host(p), before, "after struct_size 40")


def test_invalid_edits_leave_the_scene_and_its_generation_untouched():
    import torch
    from vimg_amd import abi, hip
    s = scenes.feature_scene(res=(72, 48))
    p = s.default_params(samples=4, depth=6)
    d = _dev(s)
    before = d.render_to_host(p)
    acc = d.progressive(p)
    acc.render(1)
    done = 1

    def mats(**fields):
        m = s.materials()
        for k, val in fields.items():
            setattr(m[F_MAT["wall"]], k, val)
        return m

    def texs(index, **fields):
        t = s.textures()
        for k, val in fields.items():
            setattr(t[index], k, val)
        return t

    level0 = torch.zeros(IMG_SHAPE, dtype=torch.float32, device="cuda")
    n_prims = s.view.contents.num_prims
    two_bg = [abi.Light(abi.LIGHT_BACKGROUND, 0), abi.Light(abi.LIGHT_BACKGROUND, 0)]
    bad_bg = s.background()
    bad_bg.env_tex = F_TEX["img"]
    cases = {"material index out of range": dict(materials=mats(tex=99)),
             "rg index out of range": dict(materials=mats(mr_tex=7)),
             "unknown type": dict(materials=mats(type=9)),
             "normal map that is no image": dict(materials=mats(normal_map=F_TEX["white"])),
             "texture record with another type": dict(textures=texs(F_TEX["white"], type=abi.TEX_CHECKER)),
             "image with another size": dict(textures=texs(F_TEX["img"], width=16)),
             "image wrap change": dict(textures=texs(F_TEX["img"], wrap_v=abi.WRAP_REPEAT)),
             "light prim out of range": dict(lights=[abi.Light(abi.LIGHT_PRIM, n_prims)]),
             "unknown light type": dict(lights=[abi.Light(7, 0)]),
             "two background entries": dict(lights=two_bg),
             "background with another env_tex": dict(background=bad_bg)}
    for what, kw in cases.items():
        with pytest.raises(hip.HipError, match=r"\[-1\] .+"):
            d.update_materials(**kw)
        _same(d.render_to_host(p), before, what)
        acc.render(1)                               # nothing changed: the accumulator goes on
        done += 1
        assert acc.samples == done, what
    # image entries: on a CONST texture, out of range, NULL and misaligned level0 (through the struct itself)
    lib = hip._lib()
    for what, tex, ptr in (("image entry on a CONST texture", F_TEX["white"], level0.data_ptr()), ("texture out of range", 99, level0.data_ptr()),
                           ("NULL level0", F_TEX["img"], None), ("misaligned level0", F_TEX["img"], level0.data_ptr() + 2)):
        im = (abi.TextureImage * 1)()
        im[0].texture, im[0].level0 = tex, ptr
        upd = abi.GeometryUpdate(images=C.cast(im, C.POINTER(abi.TextureImage)), num_images=1)
        assert lib.vimg_hip_scene_update_geometry(d._h, C.byref(upd), None) == -1, what
        assert lib.vimg_hip_last_error(), what
        _same(d.render_to_host(p), before, what)
        acc.render(1)
        done += 1
        assert acc.samples == done, what
    with pytest.raises(ValueError):
        d.update_materials(images={F_TEX["white"]: level0})
    with pytest.raises(ValueError):
        d.update_materials(images={F_TEX["img"]: level0[:4]})
    with pytest.raises(ValueError):
        d.update_materials(materials=list(s.materials())[:-1])
    # a valid edit after all that still works, and bumps the generation once
    h = scenes.feature_scene(res=(72, 48))
    h.set_texture_colors(F_TEX["white"], (0.2, 0.5, 0.9))
    d.update_from(h)
    with pytest.raises(hip.HipError, match=r"\[-1\]"):
        acc.render(1)
    _same(d.render_to_host(p), _dev(h).render_to_host(p), "a valid edit after the refused ones")
