#!/usr/bin/env python3
"""Cost of editing a resident scene's materials, lights and textures, on the config 3 and config 5
stand-ins at their default sizes.  Reports per scene, best of `reps` after a warm-up, host wall clock around the
blocking call (device tensors in):
  materials_ms  DeviceScene.update_materials(materials=...): the table, material_flags, every leaf slot's class, every
                emitter's emission
  lights_ms     ... (lights=...): the emitter list swapped for one of another length and back (new buffers, the bake)
  image_ms      ... (images={...}): the env map (config 3) or a mip-mapped colour texture (config 5) at the stand-in's
                size - level 0 device to device, the mip chain, and for the env map the sampling CDFs
  upload_ms     a full vimg_hip_scene_upload of the same host scene
and checks that one sample per pixel after the last edits is bit for bit the fresh upload of the host scene edited the
same way.  One JSON line per scene."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import scenes
from vimg_amd import abi, hip

hip.init(0)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5


def best(fn, n):
    out = []
    for k in range(n + 1):                  # the first one warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(k)
        out.append(time.perf_counter() - t0)
    return round(min(out[1:]) * 1e3, 3), round(float(np.median(out[1:])) * 1e3, 3)


for name, make in (("config3", scenes.config3_scene), ("config5", scenes.config5_scene)):
    s = make()
    view = s.view.contents
    upload = best(lambda k: hip.DeviceScene(s).close(), reps)
    d = hip.DeviceScene(s)
    # materials: two tables that differ in every Principled scalar (the last applied: `mats[1]`, as k ends odd or even below)
    mats = [s.materials(), s.materials()]
    for m in mats[1]:
        if m.type == abi.MAT_PRINCIPLED:
            m.roughness_factor, m.metallic_factor, m.clearcoat = 0.5 * m.roughness_factor + 0.1, 1.0 - m.metallic_factor, 0.25
    materials = best(lambda k: d.update_materials(materials=mats[k % 2]), 2 * reps + 1)      # (ends on mats[1])
    # lights: the list without its last entry, and whole again
    full = list(s.lights())
    lists = [full, full[:-1]]
    lights = best(lambda k: d.update_materials(lights=lists[k % 2]), 2 * reps + 1)           # (ends on the shorter list)
    d.update_materials(lights=full)
    # image: the env map, or the first image texture
    tex = view.background.env_tex if view.background.type == abi.BG_ENVMAP else \
        next(i for i in range(view.num_textures) if view.textures[i].type == abi.TEX_IMAGE)
    t = view.textures[tex]
    off = int(t.level_offset[0]) * 3
    level0 = np.ctypeslib.as_array(view.texels, (int(view.num_texels) * 3,))[off:off + t.width * t.height * 3].reshape(t.height, t.width, 3)
    imgs = [torch.from_numpy(level0.copy()).cuda(), torch.from_numpy(np.ascontiguousarray(level0[:, ::-1] * 0.8 + 0.05)).cuda()]
    image = best(lambda k: d.update_materials(images={tex: imgs[k % 2]}), 2 * reps + 1)      # (ends on imgs[1])
    # the fresh upload of the host scene with the same edits renders the same bits
    s.set_materials(mats[1])
    s.set_texture_image(tex, imgs[1].cpu().numpy())
    p = s.default_params(samples=1, depth=4)
    img, st = d.render_to_host(p)
    ref, rst = hip.DeviceScene(s).render_to_host(p)
    same = bool(np.array_equal(img.view(np.uint32), ref.view(np.uint32))) and st.as_dict() == rst.as_dict()
    print(json.dumps({"scene": name, "triangles": int(view.num_tris), "prims": int(view.num_prims), "materials": int(view.num_materials),
                      "lights": len(full), "image": [int(t.width), int(t.height)], "env_map": bool(view.background.type == abi.BG_ENVMAP),
                      "materials_ms": materials[0], "materials_ms_median": materials[1], "lights_ms": lights[0],
                      "lights_ms_median": lights[1], "image_ms": image[0], "image_ms_median": image[1],
                      "upload_ms": upload[0], "upload_ms_median": upload[1], "bit_identical_to_fresh": same}), flush=True)
    assert same
    d.close()
