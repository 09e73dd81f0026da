"""Ray queries at the boundary, without a GPU (vimg_hip_trace_rays, _occluded, _camera_rays): the record layouts
of the header equal the ctypes mirror, argument errors are answered before anything touches the scene or the
device, and the query kernels keep everything in registers."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from vimg_amd import abi
from test_host_and_abi import _kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vimg_hip_trace_rays", "vimg_hip_occluded", "vimg_hip_camera_rays")
INVALID = -1   # VIMG_E_INVALID


def test_record_sizes_of_the_header_are_the_ctypes_mirror():
    src = ('#include <stdio.h>\n#include "vimg_hip.h"\nint main(void){printf("%zu %zu %zu %u\\n",'
           'sizeof(VimgRay),sizeof(VimgRayHit),sizeof(VimgHitInfo),VIMG_NO_HIT);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o",
                        os.path.join(d, "p")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(d, "p")], capture_output=True,
                                              text=True, check=True).stdout.split()]
    assert got == [C.sizeof(abi.Ray), C.sizeof(abi.RayHit), C.sizeof(abi.HitInfo), abi.NO_HIT]
    assert got[:3] == [32, 16, 48]
    # field offsets the kernels store by
    assert abi.Ray.t_min.offset == 12 and abi.Ray.dir.offset == 16 and abi.Ray.t_max.offset == 28
    assert abi.RayHit.prim.offset == 4 and abi.HitInfo.uv.offset == 36 and abi.HitInfo.mat.offset == 44


def test_query_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vimg_hip.h")).read()
    lib = abi.hip_lib()                       # loads on a machine without a GPU
    for name in ENTRY_POINTS:
        assert name + "(" in header, name
        assert name in abi.HIP_SYMBOLS, name
        assert hasattr(lib, name), name


class _Fake:
    """A scene handle and device-like buffers that are never dereferenced: the checks must not read them."""

    def __init__(self):
        self.buf = (C.c_uint8 * 256)()
        base = C.addressof(self.buf)
        self.aligned = base + (-base) % 16
        self.scene = C.c_void_p(self.aligned)

    def at(self, off):
        return C.c_void_p(self.aligned + 16 + off)


def _err():
    return abi.hip_lib().vimg_hip_last_error().decode()


@pytest.mark.parametrize("call", ENTRY_POINTS)
def test_bad_arguments_are_refused_before_any_launch(call):
    lib, f = abi.hip_lib(), _Fake()
    fn = getattr(lib, call)

    def run(scene, inp, n, out, info=None):
        if call == "vimg_hip_trace_rays":
            return fn(scene, inp, n, out, info, None)
        return fn(scene, inp, n, out, None)

    good_in, good_out = f.at(0), f.at(32)
    # NULL scene
    assert run(None, good_in, 4, good_out) == INVALID and "null scene" in _err()
    # NULL buffers with n > 0
    assert run(f.scene, None, 4, good_out) == INVALID and "null" in _err()
    assert run(f.scene, good_in, 4, None) == INVALID and "null" in _err()
    # misaligned input
    assert run(f.scene, f.at(4), 4, good_out) == INVALID and "aligned" in _err()
    # misaligned output: refused for the 16-byte records, any alignment for the occlusion flags
    if call != "vimg_hip_occluded":
        assert run(f.scene, good_in, 4, f.at(36)) == INVALID and "aligned" in _err()
    if call == "vimg_hip_trace_rays":
        assert run(f.scene, good_in, 4, good_out, f.at(72)) == INVALID and "info" in _err()
    # n >= 2^32
    assert run(f.scene, good_in, 1 << 32, good_out) == INVALID and "2^32" in _err()
    # n == 0: nothing to do, even with NULL buffers
    assert run(f.scene, None, 0, None) == 0


def test_query_kernels_use_no_scratch_and_spill_nothing():
    """The three query builds (closest, closest + record, occlusion) of build/hip/ray_query.o: traversal only, so
    everything stays in registers."""
    notes = _kernel_notes(os.path.join(ROOT, "build", "hip", "ray_query.o"))
    if notes is None:
        pytest.skip("no build/hip objects or no binutils / llvm tools here")
    queries = {k: v for k, v in notes.items() if "ray_query_kernel" in k}
    assert len(queries) == 3, sorted(notes)
    for name, n in queries.items():
        assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0, (name, n)
    assert any("camera_rays_kernel" in k for k in notes), sorted(notes)
