"""Progressive rendering at the boundary, without a GPU: the entry points are exported and declared, the
ctypes declarations agree with the C prototypes, and the Python layer fails loudly."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vimg_hip_progressive_create", "vimg_hip_progressive_render", "vimg_hip_progressive_samples",
                "vimg_hip_progressive_reset", "vimg_hip_progressive_free")


def test_progressive_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vimg_hip.h")).read()
    assert "typedef struct VimgProgressive VimgProgressive;" in header
    lib = abi.hip_lib()                       # loads on a machine without a GPU
    for name in ENTRY_POINTS:
        assert name + "(" in header, name
        assert name in abi.HIP_SYMBOLS, name
        assert hasattr(lib, name), name


def test_ctypes_declarations_match_the_c_prototypes():
    """A C probe assigns every entry point to a pointer of the function type the ctypes table describes;
    the compiler refuses any mismatch (-Werror)."""
    ctype_of = {C.c_int: "int", C.c_uint64: "uint64_t", abi.u32: "uint32_t", C.c_void_p: "void*",
                abi.PParams: "const VimgRenderParams*", abi.PStats: "VimgRenderStats*",
                C.POINTER(C.c_void_p): "VimgProgressive**"}
    # the opaque handles travel as void* in ctypes: the probe names their C types per position
    handles = {"vimg_hip_progressive_create": {0: "VimgDeviceScene*"},
               "vimg_hip_progressive_render": {0: "VimgDeviceScene*", 1: "VimgProgressive*", 3: "void*", 4: "void*"},
               "vimg_hip_progressive_samples": {0: "const VimgProgressive*"},
               "vimg_hip_progressive_reset": {0: "VimgProgressive*"},
               "vimg_hip_progressive_free": {0: "VimgProgressive*"}}
    lines = ['#include <stdint.h>', '#include "vimg_hip.h"', "int main(void) {"]
    for name in ENTRY_POINTS:
        res, args = abi.HIP_SYMBOLS[name]
        cargs = [handles[name].get(i, ctype_of[a]) for i, a in enumerate(args)]
        lines.append(f"  {ctype_of[res]} (*p_{name})({', '.join(cargs)}) = {name}; (void)p_{name};")
    lines.append("  return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.c")
        open(src, "w").write("\n".join(lines) + "\n")
        r = subprocess.run(["gcc", "-std=c11", "-Werror", "-Wall", "-c", "-I", os.path.join(ROOT, "include"), src,
                            "-o", os.path.join(d, "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_progressive_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("this check is for the GPU-less container")
    import scenes
    from vimg_amd import hip
    s = scenes.json_scene("disney_spheres.json", res=(32, 16))
    with pytest.raises(hip.HipError):
        hip.DeviceScene(s).progressive(s.default_params())
    # a scene that never reached the device: the accumulator is refused, no silent fallback
    dead = hip.DeviceScene.__new__(hip.DeviceScene)
    dead._lib, dead._h, dead.resolution = abi.hip_lib(), C.c_void_p(), (32, 16)
    with pytest.raises(hip.HipError, match=r"\[-1\]"):
        dead.progressive(s.default_params())
    lib = abi.hip_lib()
    assert lib.vimg_hip_progressive_samples(None) == 0
    assert lib.vimg_hip_progressive_reset(None) == -1
    assert lib.vimg_hip_progressive_free(None) == 0
    assert lib.vimg_hip_progressive_render(None, None, 1, None, None, None) == -1
