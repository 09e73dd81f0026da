"""vimg_hip_scene_rebuild_bvh and vimg_hip_scene_bvh_cost at the boundary, without a GPU: both libraries export
them and the header declares them, VimgRebuildOptions has the C compiler's size, argument errors are answered
before the scene or the device is touched, and the new kernels keep everything in registers."""
import ctypes as C
import os
import subprocess
import tempfile

from vimg_amd import abi
from test_host_and_abi import _declared, _kernel_notes
from test_ray_query_abi import _Fake, _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vimg_hip_scene_rebuild_bvh", "vimg_hip_scene_bvh_cost")
INVALID = -1   # VIMG_E_INVALID
KERNELS = ("scene_rebuild_bounds", "scene_rebuild_classify", "scene_rebuild_nodes", "scene_rebuild_cls", "scene_rebuild_slots",
           "scene_bvh_cost_partial", "scene_bvh_cost_final")


def test_entry_points_are_declared_and_exported():
    declared = _declared("vimg_hip.h")
    lib = abi.hip_lib()   # loads on a machine without a GPU
    for name in ENTRY_POINTS:
        assert name in declared, name
        assert name in abi.HIP_SYMBOLS, name
        assert hasattr(lib, name), name


def test_rebuild_options_have_the_c_compilers_size():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "vimg_hip.h"\nint main(void){printf("%zu %zu %d %d\\n",'
           'sizeof(VimgRebuildOptions),offsetof(VimgRebuildOptions,builder),VIMG_BUILDER_PLOC,VIMG_BUILDER_LBVH);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(abi.RebuildOptions), abi.RebuildOptions.builder.offset, abi.BUILDER_PLOC, abi.BUILDER_LBVH]
    assert abi.RebuildOptions().struct_size == C.sizeof(abi.RebuildOptions) == 8
    assert abi.BUILDERS == {"ploc": abi.BUILDER_PLOC, "lbvh": abi.BUILDER_LBVH}


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    """The scene handle is a buffer that is never dereferenced: the checks must not read it."""
    lib, f = abi.hip_lib(), _Fake()
    good = abi.RebuildOptions(builder=abi.BUILDER_LBVH)
    assert lib.vimg_hip_scene_rebuild_bvh(None, C.byref(good), None) == INVALID and "null scene" in _err()
    assert lib.vimg_hip_scene_rebuild_bvh(None, None, None) == INVALID and "null scene" in _err()
    short = abi.RebuildOptions(builder=abi.BUILDER_PLOC)
    short.struct_size = 4
    assert lib.vimg_hip_scene_rebuild_bvh(f.scene, C.byref(short), None) == INVALID and "struct_size" in _err()
    for b in (2, 0xFFFFFFFF):
        assert lib.vimg_hip_scene_rebuild_bvh(f.scene, C.byref(abi.RebuildOptions(builder=b)), None) == INVALID
        assert "unknown builder" in _err()
    cost = C.c_double(-1.0)
    assert lib.vimg_hip_scene_bvh_cost(None, None, C.byref(cost)) == INVALID and "null" in _err()
    assert lib.vimg_hip_scene_bvh_cost(f.scene, None, None) == INVALID and "null" in _err()
    assert cost.value == -1.0


def test_python_layer_refuses_an_unknown_builder_name():
    import pytest
    from vimg_amd import hip
    d = hip.DeviceScene.__new__(hip.DeviceScene)     # (no upload: the name is checked before the handle is used)
    d._h = C.c_void_p()
    with pytest.raises(ValueError, match="builder"):
        d.rebuild_bvh(builder="sweep")


def test_rebuild_and_cost_kernels_use_no_scratch_and_spill_nothing():
    """The five kernels that make the device layout from a new tree and the two of the cost, read from the code
    object of build/hip/scene_rebuild.o as the ray-query pin reads its own."""
    import pytest
    notes = _kernel_notes(os.path.join(ROOT, "build", "hip", "scene_rebuild.o"))
    if notes is None:
        pytest.skip("no build/hip objects or no binutils / llvm tools here")
    for kernel in KERNELS:
        mine = {k: v for k, v in notes.items() if kernel in k}
        assert len(mine) == 1, (kernel, sorted(notes))
        for name, n in mine.items():
            assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0, (name, n)
