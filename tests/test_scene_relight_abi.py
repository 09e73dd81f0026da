"""The material update at the boundary, without a GPU: VimgGeometryUpdate grew behind its struct_size, so the layout of
the header must equal the ctypes mirror, its first 32 bytes must be the earlier struct, and argument errors must be
answered before anything touches the scene or a device.  The feature adds no export to the HIP library."""
import ctypes as C
import os
import subprocess
import tempfile

from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # VIMG_E_INVALID

FIELDS = ("struct_size", "vertices", "normals", "spheres", "materials", "textures", "lights", "num_lights", "set_lights",
          "background", "images", "num_images", "reserved")


def test_update_struct_of_the_header_is_the_ctypes_mirror():
    offs = ",".join(f"offsetof(VimgGeometryUpdate,{f})" for f in FIELDS)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vimg_hip.h"\nint main(void){size_t v[]={sizeof(VimgGeometryUpdate),'
           f'sizeof(VimgTextureImage),offsetof(VimgTextureImage,level0),VIMG_GEOMETRY_UPDATE_V1_SIZE,{offs}}};'
           'for(size_t i=0;i<sizeof v/sizeof v[0];++i)printf("%zu ",v[i]);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o",
                        os.path.join(d, "p")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(abi.GeometryUpdate), C.sizeof(abi.TextureImage), abi.TextureImage.level0.offset, C.sizeof(abi.GeometryUpdateV1)]
    want += [getattr(abi.GeometryUpdate, f).offset for f in FIELDS]
    assert got == want
    # the earlier layout: 32 bytes, its four fields where they were
    assert C.sizeof(abi.GeometryUpdateV1) == 32 and got[3] == 32
    assert [getattr(abi.GeometryUpdate, f).offset for f in FIELDS[:4]] == [0, 8, 16, 24]
    assert [getattr(abi.GeometryUpdateV1, f).offset for f in FIELDS[:4]] == [0, 8, 16, 24]
    assert abi.GeometryUpdate.materials.offset == 32
    assert abi.GeometryUpdate().struct_size == C.sizeof(abi.GeometryUpdate) and abi.GeometryUpdateV1().struct_size == 32
    assert C.sizeof(abi.TextureImage) == 16


def test_null_scene_or_update_is_invalid_without_a_gpu():
    lib = abi.hip_lib()                       # loads on a machine without a GPU
    upd = abi.GeometryUpdate()
    mats = (abi.Material * 1)()
    upd.materials = C.cast(mats, C.POINTER(abi.Material))
    assert lib.vimg_hip_scene_update_geometry(None, C.byref(upd), None) == INVALID
    assert b"null" in lib.vimg_hip_last_error()
    v1 = abi.GeometryUpdateV1()
    assert lib.vimg_hip_scene_update_geometry(None, C.cast(C.byref(v1), C.POINTER(abi.GeometryUpdate)), None) == INVALID


def test_the_feature_is_declared_without_a_new_hip_export():
    header = open(os.path.join(ROOT, "include", "vimg_hip.h")).read()
    assert "VimgTextureImage" in header and "set_lights" in header
    want = open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read().split()
    assert set(abi.HIP_SYMBOLS) <= set(want)          # nothing bound that the library did not export before
    host_header = open(os.path.join(ROOT, "include", "vimg_host.h")).read()
    lib = abi.host_lib()
    for name in ("vimg_host_set_materials", "vimg_host_set_texture_colors", "vimg_host_set_texture_image", "vimg_host_set_background"):
        assert name + "(" in host_header and name in abi.HOST_SYMBOLS and hasattr(lib, name), name
