"""The first-hit feature integrators at the boundary, without a GPU: six new values of VimgRenderParams.integrator
(include/vimg_scene.h) under the names of abi.INTEGRATORS, in a struct that did not change, through a library that
exports what it exported before."""
import ctypes as C
import os
import subprocess
import tempfile

from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEATURES = {"albedo": "VIMG_INTEGRATOR_ALBEDO", "normal": "VIMG_INTEGRATOR_NORMAL", "depth": "VIMG_INTEGRATOR_DEPTH",
            "position": "VIMG_INTEGRATOR_POSITION", "uv": "VIMG_INTEGRATOR_UV", "coverage": "VIMG_INTEGRATOR_COVERAGE"}
OLD = {"s_normal": "VIMG_INTEGRATOR_S_NORMAL", "g_normal": "VIMG_INTEGRATOR_G_NORMAL",
       "material": "VIMG_INTEGRATOR_MATERIAL", "mis": "VIMG_INTEGRATOR_MIS"}
INVALID = -1   # VIMG_E_INVALID


def _header_values(names):
    """The values the C compiler gives the enumerators `names` of vimg_hip.h, then sizeof(VimgRenderParams)."""
    src = ('#include <stdio.h>\n#include "vimg_hip.h"\nint main(void){'
           + "".join(f'printf("%d\\n",(int){n});' for n in names)
           + 'printf("%zu\\n",sizeof(VimgRenderParams));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")],
                       check=True)
        out = subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()
    return [int(v) for v in out]


def test_the_six_feature_integrators_of_the_header_are_the_names_of_the_binding():
    names = {**OLD, **FEATURES}
    got = _header_values(list(names.values()))
    assert dict(zip(names, got[:-1])) == abi.INTEGRATORS
    assert [abi.INTEGRATORS[k] for k in FEATURES] == [4, 5, 6, 7, 8, 9]
    assert tuple(FEATURES) == abi.FEATURES
    assert (abi.INTEGRATOR_ALBEDO, abi.INTEGRATOR_NORMAL, abi.INTEGRATOR_DEPTH, abi.INTEGRATOR_POSITION,
            abi.INTEGRATOR_UV, abi.INTEGRATOR_COVERAGE) == (4, 5, 6, 7, 8, 9)


def test_the_render_parameters_did_not_change():
    assert _header_values(list(FEATURES.values()))[-1] == C.sizeof(abi.RenderParams) == 20
    assert [f for f, _ in abi.RenderParams._fields_] == ["integrator", "samples", "depth", "tile_rank", "tile_world"]


def test_the_features_enter_through_the_entry_points_the_library_had():
    want = open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read().split()
    assert set(abi.HIP_SYMBOLS) <= set(want)
    abi.hip_lib()                       # loads on a machine without a GPU
    lib = os.path.join(ROOT, "v-img_amd", "lib", "libvimg_hip.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    have = sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("vimg_"))
    assert have == want
    # ... and the kernel of their own is in it
    assert any("feature_kernel" in l for l in nm.splitlines())


def test_make_params_takes_the_features_by_name():
    from vimg_amd.host import make_params
    for name in FEATURES:
        p = make_params(integrator=name, samples=3)
        assert (p.integrator, p.samples) == (abi.INTEGRATORS[name], 3)


def test_values_behind_the_last_feature_are_unknown_integrators():
    """check_params answers before it reads the scene: a handle that is never dereferenced will do."""
    lib = abi.hip_lib()
    buf = (C.c_uint8 * 64)()
    for bad in (10, 11, 0xFFFFFFFF):
        p = abi.RenderParams(bad, 1, 1, 0, 1)
        assert lib.vimg_hip_shard_pixels(C.c_void_p(C.addressof(buf)), C.byref(p)) == INVALID
        assert b"unknown integrator" in lib.vimg_hip_last_error()


def test_the_command_line_refuses_feature_buffers_without_an_image():
    """-a prefix writes the feature buffers beside a rendered image: with the heatmap (-m) or the single-pixel trace
    (-d) there is none, and the flag is refused with the usage text before anything is loaded."""
    exe = os.path.join(abi.PKG_DIR, "bin", "vimg-amd")
    for extra in (["-m", "20"], ["-d", "3 4"]):
        r = subprocess.run([exe, "-f", "no_such_scene.json", "-a", "aux"] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "-a prefix" in r.stderr and "usage" in r.stderr, r.stderr
