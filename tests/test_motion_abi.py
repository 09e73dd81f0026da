"""The motion library at its boundary, without a GPU: include/vimg_motion.h against its ctypes mirror, the exports of
libvimg_motion.so and of the other libraries, every argument error of vimg_motion_previous_position with its whole
sentence, and the numpy restatement of its contract (tests/motion_ref.py) pinned on its own against cases worked out by
hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import motion_ref as R
from abi_layout import c_layout, ctypes_layout
from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # VIMG_E_INVALID
F = np.float32
EXPORTS = ["vimg_motion_last_error", "vimg_motion_previous_position"]
OTHERS = {"filter": (abi.FILTER_SYMBOLS,), "temporal": (abi.TEMPORAL_SYMBOLS,), "varfilter": (abi.VARFILTER_SYMBOLS,),
          "moments": (abi.MOMENTS_SYMBOLS,), "infill": (abi.INFILL_SYMBOLS,), "wtemporal": (abi.WTEMPORAL_SYMBOLS,),
          "antilag": (abi.ANTILAG_SYMBOLS,), "host": (abi.HOST_SYMBOLS,)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _exports(name):
    lib = os.path.join(ROOT, "v-img_amd", "lib", f"libvimg_{name}.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    return nm, sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("vimg_"))


# ---- 1. header and ctypes ------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree_on_the_structs(tmp_path):
    structs = {"VimgMotionFrames": abi.MotionFrames, "VimgMotionGeometry": abi.MotionGeometry}
    got = c_layout(tmp_path, ["vimg_motion.h"], structs,
                   'printf("extent %u\\n", VIMG_MOTION_MAX_EXTENT);'
                   'printf("codes %d%d%d%d\\n", VIMG_MOTION_STATIC, VIMG_MOTION_TRIANGLE, VIMG_MOTION_SPHERE, VIMG_MOTION_OUT_OF_RANGE);'
                   'printf("records %zu\\n", sizeof(VimgRayHit) * 10000 + sizeof(VimgRay) * 100 + sizeof(VimgPrim));')
    assert got.pop("extent") == "32768" and got.pop("records") == "163208"          # 16, 32 and 8 bytes
    assert got.pop("codes") == "0123"
    assert (abi.MOTION_STATIC, abi.MOTION_TRIANGLE, abi.MOTION_SPHERE, abi.MOTION_OUT_OF_RANGE) == (0, 1, 2, 3)
    assert (R.STATIC, R.MOVED_TRIANGLE, R.MOVED_SPHERE, R.OUT_OF_RANGE, R.NO_HIT) == (0, 1, 2, 3, abi.NO_HIT)
    assert got == ctypes_layout(structs)
    assert C.sizeof(abi.MotionFrames) == 40 and C.sizeof(abi.MotionGeometry) == 72
    assert abi.MotionFrames().struct_size == 40 and abi.MotionGeometry().struct_size == 72
    assert C.sizeof(abi.RayHit) == 16 and C.sizeof(abi.Ray) == 32 and C.sizeof(abi.Prim) == 8


def test_the_library_exports_the_two_declared_names_and_leaves_the_other_libraries_alone():
    assert sorted(abi.MOTION_SYMBOLS) == EXPORTS
    # an eighth frame library, registered beside the closed list of the first nine, and loadable without a GPU
    assert "motion" not in abi._LIBRARIES and "motion" in abi._LATER_LIBRARIES
    assert not set(abi._LIBRARIES) & set(abi._LATER_LIBRARIES)
    lib = abi.motion_lib()
    assert lib is abi.motion_lib() and callable(lib.vimg_motion_previous_position)
    nm, have = _exports("motion")
    assert have == EXPORTS
    assert any("motion_previous_kernel" in l for l in nm.splitlines())
    # the shared host skeleton (frames/frame_lib.h) is internal: no error slot and no helper of it is a dynamic symbol
    assert not [l for l in nm.splitlines() if any(w in l for w in ("g_error", "vimg_frames", "4fail", "last_errorEv", "check_", "overlaps"))]
    header = open(os.path.join(ROOT, "include", "vimg_motion.h")).read()
    for name in abi.MOTION_SYMBOLS:
        assert name + "(" in header
    # the other libraries export what they exported - their symbol tables, and libvimg_hip.so its golden list - and
    # share no name with this one
    for name, tables in OTHERS.items():
        want = sorted(s for t in tables for s in t)
        assert _exports(name)[1] == want, name
        assert not set(abi.MOTION_SYMBOLS) & set(want)
    hip = open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read().split()
    assert _exports("hip")[1] == sorted(hip) and "motion" not in " ".join(hip)
    assert not set(abi.MOTION_SYMBOLS) & (set(abi.HIP_SYMBOLS) | set(abi.HIP_TEST_SYMBOLS))
    # it links the HIP runtime and none of the project's libraries
    path = os.path.join(ROOT, "v-img_amd", "lib", "libvimg_motion.so")
    needed = subprocess.run(["readelf", "-d", path], check=True, capture_output=True, text=True).stdout
    assert "libamdhip64" in needed and "libvimg" not in needed.replace("libvimg_motion", "")


def test_the_module_and_the_source_directory_of_the_same_name_do_not_collide():
    import vimg_amd.motion as mo
    assert mo.__file__.endswith("motion.py") and callable(mo.previous_position) and callable(mo.SceneTables.from_host)
    assert not [f for f in os.listdir(os.path.join(abi.PKG_DIR, "motion")) if f.endswith(".py")]


def test_centre_samples_are_the_pixel_centres_in_frame_array_order():
    import vimg_amd.motion as mo
    s = mo.centre_samples(3, 5)
    assert s.shape == (15, 4) and s.dtype == F
    s = s.reshape(3, 5, 4)
    assert np.array_equal(s[..., 0], np.tile(np.arange(5) + 0.5, (3, 1)))
    assert np.array_equal(s[..., 1], np.tile(np.array([2.5, 1.5, 0.5])[:, None], (1, 5)))          # array row r is sample y = H - 1 - r + 0.5
    assert not s[..., 2:].any()                                                                     # sample_disk(0, .) is the lens centre


def test_the_tables_of_a_host_scene():
    """tri_vertex_rows adds each mesh's first_vertex: a scene of two quads and a mesh has rows beyond the first mesh's."""
    import scenes
    import vimg_amd.motion as mo
    s = scenes.feature_scene(res=(24, 16), lens=False)
    v = s.view.contents
    rows, prims = mo.tri_vertex_rows(s), mo.prim_records(s)
    assert rows.shape == (v.num_tris, 3) and rows.dtype == np.uint32 and rows.max() == v.num_vertices - 1
    for t in (0, v.num_tris // 2, v.num_tris - 1):
        first = v.meshes[v.tri_mesh[t]].first_vertex
        assert list(rows[t]) == [first + v.tri_indices[3 * t + k] for k in range(3)]
    assert prims.shape == (v.num_prims, 2) and (prims[:, 0] == R.TRIANGLE).sum() == v.num_tris and (prims[:, 0] == R.SPHERE).sum() == 3


# ---- 2. argument errors, found before anything is enqueued -------------------------------------------------------
W, H = 8, 4
N = W * H
FRAME, HITS, RAYS, CODE = 12 * N, 16 * N, 32 * N, N
NP, NT, NV, NS = 5, 3, 7, 2


def _good_call():
    """Arguments vimg_motion_previous_position accepts up to the launch (the device pointers are never read on the host)."""
    frames = abi.MotionFrames(width=W, height=H, position=0x1000, hits=0x2000, rays=0x3000)
    geometry = abi.MotionGeometry(num_prims=NP, num_tris=NT, num_vertices=NV, num_spheres=NS, prims=0x5000, tri_vertices=0x5100,
                                  old_vertices=0x5200, new_vertices=0x5300, old_spheres=0x5400, new_spheres=0x5500)
    return dict(frames=frames, geometry=geometry, previous=0x10000, code=0x11000)


def _call(frames, geometry, previous, code):
    lib = abi.motion_lib()
    rc = lib.vimg_motion_previous_position(None if frames is None else C.byref(frames), None if geometry is None else C.byref(geometry),
                                           C.c_void_p(previous), C.c_void_p(code), None)
    return rc, lib.vimg_motion_last_error().decode()


def _edit(**kw):
    a = _good_call()
    for k, v in kw.items():
        if k in a:
            a[k] = v
        elif k in ("frames_size", "geometry_size"):
            a[k[:-5]].struct_size = v
        elif k in dict(abi.MotionFrames._fields_):
            setattr(a["frames"], k, v)
        else:
            assert k in dict(abi.MotionGeometry._fields_), k
            setattr(a["geometry"], k, v)
    return a


PREV, CODE_OUT = "motion: the previous-position output overlaps the ", "motion: the code output overlaps the "
ERRORS = [
    (dict(frames=None), "motion: null frames"), (dict(geometry=None), "motion: null geometry"),
    (dict(frames_size=39), "motion: frames.struct_size 39 is below the struct's 40"),
    (dict(geometry_size=71), "motion: geometry.struct_size 71 is below the struct's 72"),
    (dict(frames_size=0), "motion: frames.struct_size 0 is below the struct's 40"),
    (dict(width=0), "motion: width and height must be 1..32768, not 0 x 4"),
    (dict(height=0), "motion: width and height must be 1..32768, not 8 x 0"),
    (dict(width=32769), "motion: width and height must be 1..32768, not 32769 x 4"),
    (dict(height=32769), "motion: width and height must be 1..32768, not 8 x 32769"),
    (dict(position=None), "motion: null position frame"), (dict(hits=None), "motion: null hits frame"),
    (dict(position=0x1002), "motion: the position frame must be 4-byte aligned"),
    (dict(hits=0x2008), "motion: the hits must be 16-byte aligned"),
    (dict(rays=0x3004), "motion: the rays must be 16-byte aligned"),
    (dict(rays=None), "motion: null rays with 2 spheres: a sphere hit reads its ray"),
    (dict(prims=None), "motion: null prims table with num_prims 5"),
    (dict(tri_vertices=None), "motion: null tri_vertices table with num_tris 3"),
    (dict(prims=0x5004), "motion: the prims table must be 8-byte aligned"),
    (dict(tri_vertices=0x5102), "motion: the tri_vertices table must be 4-byte aligned"),
    (dict(old_vertices=None), "motion: old_vertices and new_vertices go together: old_vertices is null"),
    (dict(new_vertices=None), "motion: old_vertices and new_vertices go together: new_vertices is null"),
    (dict(old_spheres=None), "motion: old_spheres and new_spheres go together: old_spheres is null"),
    (dict(new_spheres=None), "motion: old_spheres and new_spheres go together: new_spheres is null"),
    (dict(old_vertices=0x5201), "motion: the vertex tables must be 4-byte aligned"),
    (dict(new_vertices=0x5302), "motion: the vertex tables must be 4-byte aligned"),
    (dict(old_spheres=0x5404), "motion: the sphere tables must be 16-byte aligned"),
    (dict(new_spheres=0x5508), "motion: the sphere tables must be 16-byte aligned"),
    (dict(previous=None), "motion: null previous-position output"),
    (dict(previous=0x10002), "motion: the previous-position output must be 4-byte aligned"),
    # each forbidden overlap: the last bytes of one buffer on the first of the other, and the other way round
    (dict(previous=0x1000 + FRAME - 4), PREV + "position frame"), (dict(previous=0x1000 - FRAME + 4), PREV + "position frame"),
    (dict(previous=0x2000 + HITS - 4), PREV + "hits"), (dict(previous=0x2000 - FRAME + 4, position=0x20000), PREV + "hits"),
    (dict(previous=0x3000 + RAYS - 4), PREV + "rays"), (dict(previous=0x3000 - FRAME + 4, hits=0x20000), PREV + "rays"),
    (dict(previous=0x5000 + 8 * NP - 4), PREV + "prims table"),
    (dict(previous=0x5100 + 12 * NT - 4), PREV + "tri_vertices table"),
    (dict(previous=0x5200 + 12 * NV - 4), PREV + "old_vertices table"),
    (dict(previous=0x5300 + 12 * NV - 4), PREV + "new_vertices table"),
    (dict(previous=0x5400 + 16 * NS - 4), PREV + "old_spheres table"),
    (dict(previous=0x5500 + 16 * NS - 4), PREV + "new_spheres table"),
    (dict(code=0x1000 + FRAME - 1), CODE_OUT + "position frame"), (dict(code=0x1000 - CODE + 1), CODE_OUT + "position frame"),
    (dict(code=0x2000), CODE_OUT + "hits"), (dict(code=0x3000 + RAYS - 1), CODE_OUT + "rays"),
    (dict(code=0x5000 + 8 * NP - 1), CODE_OUT + "prims table"), (dict(code=0x5100 + 1), CODE_OUT + "tri_vertices table"),
    (dict(code=0x5200), CODE_OUT + "old_vertices table"), (dict(code=0x5300 + 12 * NV - 1), CODE_OUT + "new_vertices table"),
    (dict(code=0x5400 + 16 * NS - 1), CODE_OUT + "old_spheres table"), (dict(code=0x5500), CODE_OUT + "new_spheres table"),
    (dict(code=0x10000 + FRAME - 1), "motion: the code output overlaps the previous-position output"),
    (dict(code=0x10000 - CODE + 1), "motion: the code output overlaps the previous-position output"),
]


@pytest.mark.parametrize("edit,sentence", ERRORS, ids=[f"{'-'.join(e)}-{i}" for i, (e, _) in enumerate(ERRORS)])
def test_argument_errors_are_invalid_with_their_whole_sentence_and_need_no_device(edit, sentence):
    rc, msg = _call(**_edit(**edit))
    assert rc == INVALID and msg == sentence, (rc, msg)


def test_the_checks_come_in_a_fixed_order():
    order = [dict(frames_size=1), dict(geometry_size=1), dict(width=0), dict(hits=None), dict(position=0x1001), dict(rays=0x3001),
             dict(prims=None), dict(tri_vertices=0x5101), dict(old_vertices=None), dict(new_spheres=None), dict(previous=None)]
    sentences = ["frames.struct_size", "geometry.struct_size", "width and height", "null hits frame", "the position frame must be",
                 "the rays must be", "null prims table", "the tri_vertices table must be", "old_vertices and new_vertices",
                 "old_spheres and new_spheres", "null previous-position output"]
    for i in range(len(order) - 1):
        for j in range(i + 1, len(order)):
            rc, msg = _call(**_edit(**order[i], **order[j]))
            assert rc == INVALID and sentences[i] in msg, (i, j, msg)
    # the previous-position output's overlaps come before the code output's
    rc, msg = _call(**_edit(previous=0x2000, code=0x1000))
    assert rc == INVALID and msg == PREV + "hits"


def test_the_error_slot_is_the_librarys_own_and_what_is_not_an_error():
    import test_temporal_abi as TA
    tmp, lib = abi.temporal_lib(), abi.motion_lib()
    fail_m = lambda: _call(**_edit(hits=None))
    fail_t = lambda: TA._call(**TA._edit(sigma_plane=-3.0))
    for first, second in ((fail_m, fail_t), (fail_t, fail_m)):
        assert first()[0] == INVALID and second()[0] == INVALID
        assert lib.vimg_motion_last_error().decode() == "motion: null hits frame"
        assert tmp.vimg_temporal_last_error().decode() == "temporal: sigma_plane must be > 0 and finite, not -3"
    # a good call, no code output, no moved tables, no rays without spheres, empty tables with NULL pointers, buffers that
    # touch end to start, an output inside a table that is not read: all pass every argument check and only then need
    # a device.  The pointers are made up, so the calls are only made where no device could follow them
    import torch
    if not torch.cuda.is_available():
        for ok in (dict(), dict(code=None), dict(old_vertices=None, new_vertices=None), dict(old_spheres=None, new_spheres=None),
                   dict(rays=None, num_spheres=0), dict(prims=None, num_prims=0), dict(tri_vertices=None, num_tris=0),
                   dict(previous=0x1000 + FRAME), dict(previous=0x2000 - FRAME), dict(code=0x10000 + FRAME),
                   dict(previous=0x5400, num_spheres=0), dict(width=32768, height=1, previous=0x4000000, code=0x5000000)):
            rc, msg = _call(**_edit(**ok))
            assert rc == -2 and "launch failed" in msg, (ok, rc, msg)          # VIMG_E_DEVICE, no silent success


# ---- 3. the restatement, pinned on its own against cases worked by hand ---------------------------------------------
PRIMS = np.array([[0, 0], [0, 1], [1, 0], [1, 1], [7, 0]], np.uint32)          # two triangles, two spheres, an unknown type
TRIS = np.array([[0, 1, 2], [2, 3, 9]], np.uint32)                             # the second names vertex row 9 of 4
OLD_V = np.array([[0, 0, 0], [64, 0, 0], [0, 64, 0], [64, 64, 8]], F)
RAY = np.array([[0, 0, -10, 1e-4, 0, 0, 1, np.inf]], F)                        # along +z from (0, 0, -10)


def _one(P, hit, old_v=None, new_v=None, old_s=None, new_s=None, rays=RAY, prims=PRIMS, tris=TRIS, nv=4, ns=2):
    Q, code = R.previous_position(np.array(P, F).reshape(1, 1, 3), R.hit_records(*[[v] for v in hit]), rays, prims, tris, nv, ns, old_v,
                                  new_v, old_s, new_s)
    return Q[0, 0], int(code[0, 0])


def test_a_static_triangle_hit_returns_the_positions_bits_minus_zero_included():
    P = np.array([-0.0, 3.25, -7.5], F)
    for new in (OLD_V, OLD_V.copy()):
        Q, code = _one(P, (2.0, 0, 0.25, 0.5), OLD_V, new)
        assert code == 0 and np.array_equal(_bits(Q), _bits(P)) and np.signbit(Q[0])
    # ... and with the vertex tables NULL: D = 0
    Q, code = _one(P, (2.0, 0, 0.25, 0.5))
    assert code == 0 and np.array_equal(_bits(Q), _bits(P))
    # the add would have lost the sign: -0 + 0 = +0
    assert not np.signbit(P[0] + F(0))


def test_integer_vertices_moved_by_an_integer_vector_give_that_vector_exactly():
    """new = old + (8, 0, -24), b1 = b2 = 0.25: e_k = (-8, 0, 24) each, w0 = 0.5, D = (0.5 e + 0.25 e) + 0.25 e = e exactly."""
    new = OLD_V + np.array([8, 0, -24], F)
    P = np.array([16.0, 16.0, 0.0], F)
    Q, code = _one(P, (5.0, 0, 0.25, 0.25), OLD_V, new)
    assert code == 1 and np.array_equal(Q - P, np.array([-8, 0, 24], F)) and np.array_equal(Q, np.array([8, 16, 24], F))
    # one vertex alone moved: D = b2 e2
    new = OLD_V.copy()
    new[2] += F(4)
    Q, code = _one(P, (5.0, 0, 0.25, 0.5), OLD_V, new)
    assert code == 1 and np.array_equal(Q - P, np.array([-2, -2, -2], F))


def test_a_sphere_that_only_translates_and_one_that_only_scales():
    old_s = np.array([[0, 0, 0, 2], [5, 5, 5, 1]], F)
    # translation by (1, 2, -4): s = 1, u s - u = 0, D = c_old - c_new, whatever the ray
    new_s = old_s + np.array([1, 2, -4, 0], F)
    P = np.array([1.0, 2.0, -6.0], F)
    Q, code = _one(P, (4.0, 2, 0.0, 0.0), old_s=old_s, new_s=new_s)
    assert code == 2 and np.array_equal(Q, np.array([0, 0, -2], F))
    # scaling 2 -> 4 about the origin: the ray from (0, 0, -10) along +z hits the new sphere at t = 6, (0, 0, -4):
    # u = (0, 0, -4), s = 0.5, u s - u = (0, 0, -2) - (0, 0, -4) = (0, 0, 2), D = 0 + that: Q = (0, 0, -2), on the old sphere
    new_s = old_s.copy()
    new_s[0, 3] = 4
    P = np.array([0.0, 0.0, -4.0], F)
    Q, code = _one(P, (6.0, 2, 0.0, 0.0), old_s=old_s, new_s=new_s)
    assert code == 2 and np.array_equal(Q, np.array([0, 0, -2], F))
    # shrinking 3 -> 1, worked in float32 operation for operation: the hit at (0, 0, -1), t = 9, was at (0, 0, -3)
    new_s[0, 3], old = 1, old_s.copy()
    old[0, 3] = 3
    Q, code = _one(np.array([0.0, 0.0, -1.0], F), (9.0, 2, 0.0, 0.0), old_s=old, new_s=new_s)
    u = (F(-10) + F(9) * F(1)) - F(0)
    want = F(-1) + (F(0) + (u * (F(3) / F(1)) - u))
    assert code == 2 and Q[2] == want == F(-3)
    # the other sphere did not move: P's bits
    Q, code = _one(P, (6.0, 3, 0.0, 0.0), old_s=old_s, new_s=new_s)
    assert code == 0 and np.array_equal(_bits(Q), _bits(P))
    # with the sphere tables NULL: D = 0, and no ray is needed
    Q, code = _one(P, (6.0, 2, 0.0, 0.0), rays=None)
    assert code == 0 and np.array_equal(_bits(Q), _bits(P))


def test_a_new_radius_of_zero_translates_only():
    old_s = np.array([[0, 0, 0, 2], [5, 5, 5, 1]], F)
    for r_new in (0.0, -1.0, np.nan):
        new_s = np.array([[1, 0, 0, r_new], [5, 5, 5, 1]], F)
        Q, code = _one(np.array([3.0, 0.0, 0.0], F), (6.0, 2, 0.0, 0.0), old_s=old_s, new_s=new_s)
        assert code == 2 and np.array_equal(Q, np.array([2, 0, 0], F)), r_new


def test_a_miss_and_the_five_indices_out_of_range():
    new = OLD_V + F(1)
    old_s = np.array([[0, 0, 0, 2], [5, 5, 5, 1]], F)
    new_s = old_s + F(1)
    P = np.array([1.5, -0.0, 2.5], F)
    kw = dict(old_v=OLD_V, new_v=new, old_s=old_s, new_s=new_s)
    Q, code = _one(P, (np.inf, R.NO_HIT, 0.0, 0.0), **kw)
    assert code == 0 and np.array_equal(_bits(Q), _bits(P))
    cases = {"prim >= num_prims": dict(hit=(1.0, 5, 0.1, 0.1)),
             "triangle index >= num_tris": dict(hit=(1.0, 1, 0.1, 0.1), tris=TRIS[:1]),
             "vertex row >= num_vertices": dict(hit=(1.0, 1, 0.1, 0.1)),
             "sphere index >= num_spheres": dict(hit=(1.0, 3, 0.0, 0.0), ns=1),
             "unknown type": dict(hit=(1.0, 4, 0.1, 0.1))}
    for name, c in cases.items():
        Q, code = _one(P, **c, **kw)
        assert code == 3 and np.array_equal(_bits(Q), _bits(P)), name
    # the same hits in range: they move
    assert _one(P, (1.0, 0, 0.1, 0.1), **kw)[1] == 1 and _one(P, (1.0, 3, 0.0, 0.0), **kw)[1] == 2
    # a huge prim index just below VIMG_NO_HIT is out of range, not a miss
    assert _one(P, (1.0, 0xFFFFFFFE, 0.0, 0.0), **kw)[1] == 3
