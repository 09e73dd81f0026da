"""The baked material records (DMaterial, v-img_amd/csrc/material_record.h): the terms of a Principled or Lambertian
vertex that depend on the material alone are evaluated once per material by a kernel, at upload and after every edit,
and the stages load them for materials whose validity bits are set.  The statements that bake are the statements the
stages run for the other materials (material_terms.h), so every frame must stay the CPU oracle's bit for bit: no
comparison below has a tolerance.

The textured build: tests/scenes.py's feature_scene has a Principled material with a metallic-roughness map (scalar
bit clear, colour bit clear: an image) beside one with a constant colour and no map (both bits set), Lambertians on a
constant, a checkerboard and an image; it is rendered against the oracle below."""
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import scenes
from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "v-img_amd", "csrc")
RES = (90, 40)
SPHERE = 4          # d_1 of disney_spheres.json: a Principled sphere on its own constant texture (index 3)
WALL = 0            # the white walls: Lambertian on texture 0

# ---------------------------------------------------------------------------------------------- CPU
PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "material_record.h"
int main(int argc, char** argv) {
  using namespace vimg;
  std::printf("%zu %zu\n", sizeof(DMaterial), alignof(DMaterial));
  VimgTexture tex[3] = {};
  tex[0].type = VIMG_TEX_CONST, tex[1].type = VIMG_TEX_CHECKER, tex[2].type = VIMG_TEX_IMAGE;
  // rows of three integers: material type, mr_tex, type of its colour texture (-1: none)
  for (int i = 1; i + 2 < argc; i += 3) {
    VimgMaterial m = {};
    m.type = uint32_t(atol(argv[i]));
    m.mr_tex = int32_t(atol(argv[i + 1]));
    m.tex = int32_t(atol(argv[i + 2]));
    std::printf("%u\n", dmaterial_bits(m, tex));
  }
  return 0;
}
"""


def _golden_scenes():
    out = {}
    for path in sorted(glob.glob(os.path.join(scenes.SCENES, "**", "*.json"), recursive=True)):
        name = os.path.relpath(path, scenes.SCENES)
        out[name] = scenes.odyssey_without_monolith() if name.endswith("odyssey_mis.json") else scenes.json_scene(name)
    return out


def _bits_in_python(m, textures):
    """dmaterial_bits restated: the scalar group holds for a Principled material without a metallic-roughness map,
    the colour group for a Lambertian or Principled material on a constant colour."""
    scalars = m.type == abi.MAT_PRINCIPLED and m.mr_tex < 0
    colour = m.type in (abi.MAT_PRINCIPLED, abi.MAT_LAMBERTIAN) and m.tex >= 0 and textures[m.tex].type == abi.TEX_CONST
    return (1 if scalars else 0) | (2 if colour else 0)


def test_the_record_is_304_aligned_bytes_and_the_validity_bits_follow_the_material(tmp_path):
    """material_record.h compiles as plain C++; DMaterial is 304 bytes on a 16-byte boundary; dmaterial_bits agrees
    with its Python restatement for every material of every scene under tests/golden/scenes, and for the
    combinations those scenes do not hold (a map, a checkerboard, an image, every material type)."""
    src, exe = tmp_path / "bits.cpp", tmp_path / "bits"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++20", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    rows, want = [], []
    for name, s in _golden_scenes().items():
        mats, texs = s.materials(), s.textures()
        assert len(mats) > 0, name
        for m in mats:
            rows.append((m.type, m.mr_tex, texs[m.tex].type if m.tex >= 0 else -1))
            want.append(_bits_in_python(m, texs))
    assert 3 in want and 2 in want                      # Principled and Lambertian on constants: the flagship's kinds

    class M:                                            # the combinations beyond the golden scenes
        def __init__(self, type, mr_tex, tex):
            self.type, self.mr_tex, self.tex = type, mr_tex, tex

    class T:
        def __init__(self, type):
            self.type = type
    texs3 = [T(abi.TEX_CONST), T(abi.TEX_CHECKER), T(abi.TEX_IMAGE)]
    for mt in (abi.MAT_LAMBERTIAN, abi.MAT_DIELECTRIC, abi.MAT_DIFFUSE_LIGHT, abi.MAT_PRINCIPLED):
        for mr in (-1, 0):
            for tt in (-1, 0, 1, 2):
                rows.append((mt, mr, tt))
                want.append(_bits_in_python(M(mt, mr, tt), texs3))
    argv = [str(v) for row in rows for v in row]
    out = subprocess.run([str(exe)] + argv, check=True, capture_output=True, text=True).stdout.split()
    assert (int(out[0]), int(out[1])) == (304, 16)
    assert [int(v) for v in out[2:]] == want


# ---------------------------------------------------------------------------------------------- GPU
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _disney(checker=False):
    """disney_spheres at test size; `checker`: with one more texture record, a checkerboard nothing points at yet
    (a resident scene's texture table keeps its length and its records' types)."""
    s = scenes.json_scene("disney_spheres.json", res=RES)
    if checker:
        s.add_texture_checker(6, 4, (0.9, 0.2, 0.1), (0.1, 0.3, 0.9))
        s.build_bvh(abi.BVH_SWEEP)      # (the scene's view takes its tables when the tree is built: the same tree again)
    return s


def _checker_index(s):
    texs = s.textures()
    (i,) = [k for k in range(len(texs)) if texs[k].type == abi.TEX_CHECKER]
    return i


def _dev(s, general=False, **opts):
    """A resident scene; `general`: uploaded under VIMG_HIP_PLAIN=0 (read once at upload): never a PLAIN build."""
    from vimg_amd import hip
    hip.init(0)
    old = os.environ.get("VIMG_HIP_PLAIN")
    try:
        if general:
            os.environ["VIMG_HIP_PLAIN"] = "0"
        else:
            os.environ.pop("VIMG_HIP_PLAIN", None)
        return hip.DeviceScene(s, **opts)
    finally:
        if old is None:
            os.environ.pop("VIMG_HIP_PLAIN", None)
        else:
            os.environ["VIMG_HIP_PLAIN"] = old


_oracle_cache = {}


def _oracle(key, s, p):
    if key not in _oracle_cache:
        img, st, _ = O.render(s, p)
        img.setflags(write=False)
        _oracle_cache[key] = (img, st)
    return _oracle_cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("integrator", ["mis", "material"])
def test_every_baked_path_renders_the_oracles_bits(integrator):
    """disney_spheres, 90 x 40, 8 spp: all six Principled spheres are hit, primary hits evaluate without
    regularisation, hits after a diffuse bounce with it, d_4 (spec_trans 1) is entered and left.  The PLAIN build,
    the general build and the lane-bound kernel give one frame, and it is the oracle's."""
    s = _disney()
    p = s.default_params(samples=8, integrator=integrator)
    cpu, cst = _oracle(("disney", integrator), s, p)
    assert cst.closest_rays > 2 * cst.paths, "no path longer than two vertices: the regularised variant never ran"
    plain, general, lane = _dev(s), _dev(s, general=True), _dev(s, scheduler="lane")
    if integrator == "mis":
        assert plain.kernel_for(p) == "render_cu_kernel<false>" and general.kernel_for(p) == "render_cu_kernel<false,general>"
    frames = {}
    for name, d in (("plain", plain), ("general", general), ("lane", lane)):
        frames[name], st = d.render_to_host(p)
        assert st.paths == cst.paths and st.rays == cst.rays, name
        frames[name + "/timed"] = d.render_to_host(p, stats=False)
        d.close()
    for name, img in frames.items():
        differ = int((_bits(img) != _bits(cpu)).any(axis=-1).sum())
        print(f"{integrator} {name}: {differ} of {cpu.shape[0] * cpu.shape[1]} pixels differ from the oracle")
    for name, img in frames.items():
        assert np.array_equal(_bits(img), _bits(cpu)), name


def _with_checkers(s):
    """One Principled sphere and the Lambertian walls on the checkerboard: their bits clear, the others' set."""
    mats = s.materials()
    mats[SPHERE].tex = mats[WALL].tex = _checker_index(s)
    s.set_materials(mats)
    return s


@pytest.mark.gpu
def test_computed_and_baked_lanes_share_batches():
    """A checkerboard under one Principled sphere and under the Lambertian walls: those materials run
    material_terms.h's statements in the stages, beside lanes that load their records."""
    s = _with_checkers(_disney(checker=True))
    p = s.default_params(samples=8)
    cpu, cst = _oracle("checkers", s, p)
    plain_cpu, _ = _oracle(("disney", "mis"), _disney(), _disney().default_params(samples=8))
    assert not np.array_equal(_bits(cpu), _bits(plain_cpu))        # the checkerboards are seen
    for opts in ({}, dict(scheduler="lane")):
        d = _dev(s, **opts)
        img, st = d.render_to_host(p)
        d.close()
        differ = int((_bits(img) != _bits(cpu)).any(axis=-1).sum())
        print(f"checkers {opts}: {differ} pixels differ from the oracle")
        assert st.paths == cst.paths and np.array_equal(_bits(img), _bits(cpu)), opts


@pytest.mark.gpu
def test_a_textured_build_with_a_metallic_roughness_map():
    """feature_scene (the TEX builds): scalar bit clear on the mapped Principled material, set on the glass one."""
    s = scenes.feature_scene(res=(72, 48))
    mats, texs = s.materials(), s.textures()
    assert sorted(_bits_in_python(m, texs) for m in mats if m.type == abi.MAT_PRINCIPLED) == [0, 3]
    p = s.default_params(samples=6, depth=7)
    cpu, cst = _oracle("feature", s, p)
    for opts in ({}, dict(scheduler="lane")):
        d = _dev(s, **opts)
        img, st = d.render_to_host(p)
        d.close()
        differ = int((_bits(img) != _bits(cpu)).any(axis=-1).sum())
        print(f"feature {opts}: {differ} pixels differ from the oracle")
        assert st.paths == cst.paths and np.array_equal(_bits(img), _bits(cpu)), opts


# ---- re-bake on edit: each edit is a function of a host scene (with the spare checkerboard) that edits it in place
def _set(index, **fields):
    def edit(s):
        mats = s.materials()
        for k, v in fields.items():
            setattr(mats[index], k, v)
        s.set_materials(mats)
    return edit


def _colour(s):
    s.set_texture_colors(s.materials()[SPHERE].tex, (0.15, 0.7, 0.35))


def _to_lambertian(s):
    from vimg_amd import host
    mats = s.materials()
    mats[SPHERE] = host.make_material("lambertian", tex=mats[SPHERE].tex)
    s.set_materials(mats)


EDITS = {
    "roughness": [_set(SPHERE, roughness_factor=0.03)],
    "anisotropic": [_set(SPHERE, anisotropic=0.85)],
    "clearcoat_gloss": [_set(SPHERE, clearcoat=0.9, clearcoat_gloss=0.05)],
    # (sample_mat's glass lobe is the stage that loads the baked eta: the edit gives the sphere one)
    "eta": [_set(SPHERE, eta=1.9, specular_transmission=0.7)],
    "spec_trans": [_set(SPHERE, specular_transmission=0.8)],
    "metallic": [_set(SPHERE, metallic_factor=0.15)],
    "lambertian and back": [_to_lambertian, "back"],
    "colour": [_colour],
    "checkerboard and back": [lambda s: _with_checkers(s), "back"],
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDITS))
def test_an_edit_bakes_the_records_of_a_fresh_upload(name):
    """update_materials on a resident disney_spheres: image and scene_bytes of a fresh upload of the equally edited
    host scene, 4 spp; "back" returns to the first tables, whose records must come back with them."""
    base = _disney(checker=True)
    p = base.default_params(samples=4)
    d = _dev(base)
    first = d.render_to_host(p, stats=False)
    h = _disney(checker=True)
    for step in EDITS[name]:
        if step == "back":
            h = _disney(checker=True)
        else:
            step(h)
        d.update_materials(materials=h.materials(), textures=h.textures())
        fresh = _dev(h)
        got, want = d.render_to_host(p, stats=False), fresh.render_to_host(p, stats=False)
        assert np.array_equal(_bits(got), _bits(want)), (name, step)
        assert d.bytes == fresh.bytes, (name, step)
        assert np.array_equal(_bits(got), _bits(first)) == (step == "back"), (name, step)
        fresh.close()
    d.close()


@pytest.mark.gpu
def test_an_invalid_edit_leaves_the_records_as_they_were():
    from vimg_amd import hip
    base = _disney(checker=True)
    p = base.default_params(samples=4)
    d = _dev(base)
    first = d.render_to_host(p, stats=False)
    mats = base.materials()
    mats[SPHERE].roughness_factor = 0.9
    mats[WALL].tex = len(base.textures())            # out of range
    with pytest.raises(hip.HipError):
        d.update_materials(materials=mats)
    assert np.array_equal(_bits(d.render_to_host(p, stats=False)), _bits(first))
    d.close()
