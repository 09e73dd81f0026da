"""The filter library at its boundary, without a GPU: include/vimg_filter.h against its ctypes mirror, the exports
of libvimg_filter.so, every argument error of vimg_filter_atrous, and the numpy restatement of the filter's contract
(tests/atrous_ref.py) pinned on its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import atrous_ref as R
from abi_layout import c_layout, ctypes_layout
from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # VIMG_E_INVALID
F = np.float32


# ---- 1. header and ctypes ------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_structs(tmp_path):
    structs = {"VimgFilterFrames": abi.FilterFrames, "VimgAtrousParams": abi.AtrousParams}
    got = c_layout(tmp_path, ["vimg_filter.h"], structs, 'printf("codes %d %d\\n", VIMG_OK, VIMG_E_INVALID);')
    assert got.pop("codes 0") == str(INVALID)
    assert got == ctypes_layout(structs)
    assert C.sizeof(abi.FilterFrames) == 56 and C.sizeof(abi.AtrousParams) == 24
    assert abi.FilterFrames().struct_size == 56


def test_the_workspace_is_64_bytes_per_pixel_and_the_defaults_are_valid():
    lib = abi.filter_lib()
    for w, h in ((1, 1), (3, 5), (1800, 800), (32768, 32768), (0, 7)):
        assert lib.vimg_filter_atrous_workspace(w, h) == 64 * w * h
    p = abi.AtrousParams()
    lib.vimg_filter_atrous_defaults(C.byref(p))
    assert p.struct_size == C.sizeof(abi.AtrousParams) and 1 <= p.iterations <= 12
    assert p.sigma_color > 0 and 0 < p.sigma_normal < np.inf and 0 < p.sigma_plane < np.inf
    assert 0 < p.albedo_floor < 1 and np.frexp(p.albedo_floor)[0] == 0.5       # a power of two: x / f * f is exact


def test_the_library_exports_the_four_declared_names_and_leaves_the_render_library_alone():
    assert sorted(abi.FILTER_SYMBOLS) == ["vimg_filter_atrous", "vimg_filter_atrous_defaults", "vimg_filter_atrous_workspace",
                                          "vimg_filter_last_error"]
    abi.filter_lib()                    # loads on a machine without a GPU
    lib = os.path.join(ROOT, "v-img_amd", "lib", "libvimg_filter.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    have = sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("vimg_"))
    assert have == sorted(abi.FILTER_SYMBOLS)
    assert any("atrous_iteration_kernel" in l for l in nm.splitlines())       # ... and its kernels are in it
    # the shared host skeleton (frames/frame_lib.h) is internal: no error slot and no helper of it is a dynamic symbol,
    # so the dynamic linker cannot merge this library's error slot with the other frame library's
    assert not [l for l in nm.splitlines() if any(w in l for w in ("g_error", "vimg_frames", "4fail", "last_errorEv", "check_"))]
    header = open(os.path.join(ROOT, "include", "vimg_filter.h")).read()
    for name in abi.FILTER_SYMBOLS:
        assert name + "(" in header
    assert not set(abi.FILTER_SYMBOLS) & set(abi.HIP_SYMBOLS)
    assert "filter" not in open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read()


# ---- 2. argument errors, found before anything is enqueued -------------------------------------------------------
def _good_call():
    """Arguments vimg_filter_atrous accepts up to the launch (the pointers are never read on the host)."""
    frames = abi.FilterFrames(width=8, height=4, color=0x1000, normal=0x2000, position=0x3000, depth=0x4000, albedo=0x5000)
    params = abi.AtrousParams()
    abi.filter_lib().vimg_filter_atrous_defaults(C.byref(params))
    return dict(frames=frames, params=params, out=0x6000, workspace=0x10000, nbytes=64 * 8 * 4)


def _call(frames, params, out, workspace, nbytes):
    lib = abi.filter_lib()
    rc = lib.vimg_filter_atrous(None if frames is None else C.byref(frames), None if params is None else C.byref(params),
                                C.c_void_p(out), C.c_void_p(workspace), nbytes, None)
    return rc, lib.vimg_filter_last_error().decode()


def _edit(**kw):
    a = _good_call()
    for k, v in kw.items():
        if k in a:
            a[k] = v
        elif k in dict(abi.FilterFrames._fields_):
            setattr(a["frames"], k, v)
        else:
            setattr(a["params"], k, v)
    return a


ERRORS = [
    (dict(frames=None), "null frames"), (dict(params=None), "null params"),
    (dict(color=None), "null color frame"), (dict(normal=None), "null normal frame"),
    (dict(position=None), "null position frame"), (dict(depth=None), "null depth frame"),
    (dict(out=None), "null output"), (dict(workspace=None), "null workspace"),
    (dict(struct_size=55), "frames.struct_size 55 is below"),
    (dict(width=0), "width and height must be 1..32768"), (dict(height=0), "width and height must be 1..32768"),
    (dict(width=32769, nbytes=2 ** 40), "width and height must be 1..32768"),
    (dict(height=32769, nbytes=2 ** 40), "width and height must be 1..32768"),
    (dict(iterations=0), "iterations must be 1..12"), (dict(iterations=13), "iterations must be 1..12"),
    (dict(sigma_color=0.0), "sigma_color must be > 0"), (dict(sigma_color=-1.0), "sigma_color must be > 0"),
    (dict(sigma_color=float("nan")), "sigma_color must be > 0"),
    (dict(sigma_normal=0.0), "sigma_normal must be > 0"), (dict(sigma_normal=float("nan")), "sigma_normal must be > 0"),
    (dict(sigma_plane=-0.5), "sigma_plane must be > 0"), (dict(sigma_plane=float("nan")), "sigma_plane must be > 0"),
    (dict(sigma_normal=float("inf")), "sigma_normal must be > 0 and finite"),
    (dict(sigma_plane=0.0), "sigma_plane must be > 0"), (dict(sigma_plane=float("inf")), "sigma_plane must be > 0 and finite"),
    (dict(albedo_floor=0.0), "albedo_floor must be > 0"), (dict(albedo_floor=-0.25), "albedo_floor must be > 0"),
    (dict(albedo_floor=float("nan")), "albedo_floor must be > 0"),
    (dict(albedo_floor=float("inf")), "albedo_floor must be > 0 and finite"),
    (dict(nbytes=64 * 8 * 4 - 1), "the workspace has 2047 bytes, 8 x 4 needs 2048"),
    (dict(workspace=0x10008), "the workspace must be 16-byte aligned"),
]


@pytest.mark.parametrize("edit,sentence", ERRORS, ids=[f"{'-'.join(e)}-{i}" for i, (e, _) in enumerate(ERRORS)])
def test_argument_errors_are_invalid_with_their_sentence_and_need_no_device(edit, sentence):
    rc, msg = _call(**_edit(**edit))
    assert rc == INVALID and sentence in msg, (rc, msg)


def test_params_struct_size_and_the_message_of_the_last_failure():
    a = _good_call()
    a["params"].struct_size = 23
    rc, msg = _call(**a)
    assert rc == INVALID and "params.struct_size 23 is below" in msg
    rc, msg2 = _call(**_edit(iterations=99))
    assert rc == INVALID and msg2 != msg and "99" in msg2
    # sigma_color may be +inf: the call passes every argument check (and only then needs a device)
    import torch
    if not torch.cuda.is_available():
        rc, msg = _call(**_edit(sigma_color=float("inf")))
        assert rc == -2 and "launch failed" in msg, (rc, msg)          # VIMG_E_DEVICE, no silent success


# ---- 3. the restatement, pinned on its own -----------------------------------------------------------------------
PARAMS = dict(iterations=5, sigma_color=np.inf, sigma_normal=0.25, sigma_plane=0.02, albedo_floor=1 / 64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_guides_of_all_zero_normals_give_the_input_back_bit_for_bit():
    """n = 0 makes dn = 1, so s_n = 1 / sigma_normal >= 1 for sigma_normal <= 1: every off-centre weight is 0 and a
    live pixel is (k C) / k with k = 9/64.  That is C itself whenever 9 C is a float32 - colours of at most 20
    significant bits here, which every iteration returns bit for bit; for an arbitrary float32 the product rounds,
    about one value in ten comes back one ulp off, and the restatement must say exactly that: (k C) / k per
    iteration, never more than an ulp per iteration from C.  Where the guides are all zero (depth too: a frame of
    misses) nothing is live and any colour comes back bit for bit."""
    rng = np.random.default_rng(5)
    h, w = 13, 21
    zero = np.zeros((h, w, 3), F)
    position = rng.normal(size=(h, w, 3)).astype(F)
    depth = np.repeat(rng.uniform(1, 5, (h, w, 1)), 3, axis=-1).astype(F)
    exact = (rng.integers(0, 2 ** 20, (h, w, 3)) * 2.0 ** -18).astype(F)         # 9 C is exact
    anyf = rng.gamma(2.0, 0.5, (h, w, 3)).astype(F)
    k = F(9 / 64)
    for sn in (0.25, 1.0):
        p = dict(PARAMS, sigma_normal=sn, iterations=3)
        assert np.array_equal(_bits(R.atrous(exact, zero, position, depth, **p)), _bits(exact))
        out, want = R.atrous(anyf, zero, position, depth, **p), anyf
        for _ in range(3):
            want = (k * want) / k
        assert np.array_equal(_bits(out), _bits(want))
        assert np.abs(_bits(out).astype(np.int64) - _bits(anyf).astype(np.int64)).max() <= 3
        assert np.array_equal(_bits(R.atrous(anyf, zero, zero, zero, None, **p)), _bits(anyf))


def test_a_nan_colour_stays_where_it_is():
    """A NaN colour makes every S it enters NaN, so the pixel is no one's tap; it stays NaN itself (its centre tap)."""
    h, w = 24, 24
    color = np.full((h, w, 3), 0.5, F)
    color[11, 13, 1] = np.nan
    normal = np.zeros((h, w, 3), F)
    normal[..., 2] = 1
    yy, xx = np.mgrid[0:h, 0:w]
    position = np.stack([xx, yy, np.zeros_like(xx)], -1).astype(F)
    depth = np.full((h, w, 3), 10, F)
    for sc in (np.inf, 2.0):
        out = R.atrous(color, normal, position, depth, **dict(PARAMS, sigma_color=sc))
        assert np.isnan(out[11, 13, 1]) and np.isnan(out).sum() == 1
        rest = np.ones((h, w), bool)
        rest[11, 13] = False
        assert np.allclose(out[rest], 0.5, rtol=1e-6)


def test_the_synthetic_frame_loses_nine_tenths_of_its_error_and_its_sky_keeps_its_bits():
    s = R.synthetic_frame(64, 96)
    out = R.atrous(s["noisy"], s["normal"], s["position"], s["depth"], s["albedo"], **PARAMS)
    mse = lambda a: float(((a.astype(np.float64) - s["clean"]) ** 2).mean())
    before, after = mse(s["noisy"]), mse(out)
    print(f"mse noisy {before:.5f} filtered {after:.5f} ratio {before / after:.0f}")
    assert np.isfinite(out).all() and after < before / 10
    sky = ~s["hit"]
    assert sky.sum() > 500 and np.array_equal(_bits(out[sky]), _bits(s["noisy"][sky]))
    # the shaded pixels did change, with or without demodulation
    plain = R.atrous(s["noisy"], s["normal"], s["position"], s["depth"], None, **PARAMS)
    assert np.array_equal(_bits(plain[sky]), _bits(s["noisy"][sky])) and mse(plain) < before


# ---- 4. the command line ---------------------------------------------------------------------------------------------
def test_the_command_line_refuses_the_filter_without_an_image():
    """-n iterations filters a rendered image: with the heatmap (-m) or the single-pixel trace (-d) there is none, and
    the flag is refused with the usage text before anything is loaded, as -a is."""
    exe = os.path.join(abi.PKG_DIR, "bin", "vimg-amd")
    for extra in (["-m", "20"], ["-d", "3 4"]):
        r = subprocess.run([exe, "-f", "no_such_scene.json", "-n", "5"] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "-n iterations" in r.stderr and "usage" in r.stderr, r.stderr
    r = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert r.returncode == 2 and "[-n iterations]" in r.stderr
    # 0, a negative count, more than the library takes and no number at all are refused, not rendered unfiltered
    for bad in ("0", "-3", "13", "abc", "5x", ""):
        r = subprocess.run([exe, "-f", "no_such_scene.json", "-n", bad], capture_output=True, text=True)
        assert r.returncode == 2 and "-n iterations must be 1..12" in r.stderr, (bad, r.stderr)


def test_the_module_and_the_source_directory_of_the_same_name_do_not_collide():
    """v-img_amd/filter.py beside v-img_amd/filter/ (HIP sources, no Python): the import is the module."""
    import vimg_amd.filter as flt
    assert flt.__file__.endswith("filter.py") and callable(flt.atrous)
    assert not [f for f in os.listdir(os.path.join(abi.PKG_DIR, "filter")) if f.endswith(".py")]
