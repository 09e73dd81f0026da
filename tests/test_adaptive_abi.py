"""Adaptive sampling at the boundary, without a GPU: the entry points are exported, declared and mirrored, the
ctypes declarations agree with the C prototypes, argument errors are answered before anything touches a device,
and the error statistic of include/vimg_hip.h restated in numpy float32 (used by tests/test_adaptive.py)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from vimg_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vimg_hip_progressive_render_masked", "vimg_hip_progressive_launches", "vimg_hip_progressive_state",
                "vimg_hip_progressive_error", "vimg_hip_progressive_select")

F = np.float32


# ---- the statistic (include/vimg_hip.h, "Adaptive sampling"): float32, one rounding per operation, in order -------
def lum(v):
    v = np.asarray(v, dtype=F)
    return v[..., 0] * F(0.212671) + v[..., 1] * F(0.715160) + v[..., 2] * F(0.072169)


def stat_update(n_old, k_old, m2_old, s_old, s_new, n, selected):
    """(N', K', M2') after an increment of `n` samples that reached the pixels of `selected` and took their sums
    from s_old to s_new; the other pixels keep theirs."""
    n_old, k_old = np.asarray(n_old, dtype=np.uint32), np.asarray(k_old, dtype=np.uint32)
    m2_old, s_old, s_new = np.asarray(m2_old, dtype=F), np.asarray(s_old, dtype=F), np.asarray(s_new, dtype=F)
    sel = np.asarray(selected).astype(bool)
    with np.errstate(all="ignore"):
        b = lum(s_new - s_old) / F(n)
        m_old = np.where(n_old > 0, lum(s_old) / np.maximum(n_old, 1).astype(F), F(0))
        m_new = lum(s_new) / (n_old + np.uint32(n)).astype(F)
        m2 = m2_old + F(n) * (b - m_old) * (b - m_new)
    return (np.where(sel, n_old + np.uint32(n), n_old).astype(np.uint32), np.where(sel, k_old + 1, k_old).astype(np.uint32),
            np.where(sel, m2, m2_old).astype(F))


def stat_error(n, k, m2, s):
    n, k, m2 = np.asarray(n, dtype=np.uint32), np.asarray(k, dtype=np.uint32), np.asarray(m2, dtype=F)
    with np.errstate(all="ignore"):
        nf = np.maximum(n, 1).astype(F)
        m = lum(s) / nf
        var = np.where(m2 < 0, F(0), m2) / np.maximum(k.astype(np.int64) - 1, 1).astype(F) / nf
        e = np.sqrt(var) / (np.abs(m) + F(1e-3))
    return np.where(k < 2, F(np.inf), e).astype(F)


def same_floats(a, b):
    """Bitwise equality that lets NaN equal NaN (and tells +0 from -0)."""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def test_the_restatement_on_values_worked_by_hand():
    # two increments of 2 samples on one grey pixel: sums 2 -> 6 (batch means 1 and 2; Y of grey = sum of weights)
    w = F(0.212671) + F(0.715160) + F(0.072169)
    s0, s1, s2 = np.zeros((1, 3), F), np.full((1, 3), 2, F), np.full((1, 3), 6, F)
    n, k, m2 = stat_update([0], [0], [0], s0, s1, 2, [1])
    assert (n[0], k[0]) == (2, 1) and m2[0] == 0          # b == m_new: the first increment adds nothing
    assert np.isinf(stat_error(n, k, m2, s1)[0])
    n, k, m2 = stat_update(n, k, m2, s1, s2, 2, [1])
    assert (n[0], k[0]) == (4, 2)
    assert np.isclose(m2[0], 2.0 * (2 * w - w) * (2 * w - 1.5 * w), rtol=1e-6)
    e = stat_error(n, k, m2, s2)[0]
    assert np.isclose(e, np.sqrt(m2[0] / 1 / 4) / (1.5 * w + 1e-3), rtol=1e-6)
    # an unselected pixel keeps its record; a constant pixel has error 0 after two increments
    n2, k2, m22 = stat_update(n, k, m2, s2, s2, 3, [0])
    assert (n2[0], k2[0], m22[0]) == (4, 2, m2[0])
    c1, c2 = np.full((1, 3), 0.5 * 3, F), np.full((1, 3), 0.5 * 6, F)
    n, k, m2 = stat_update([0], [0], [0], s0, c1, 3, [1])
    n, k, m2 = stat_update(n, k, m2, c1, c2, 3, [1])
    assert stat_error(n, k, m2, c2)[0] == 0
    assert same_floats([np.nan, np.inf, 0.0], [np.nan, np.inf, 0.0]) and not same_floats([0.0], [-0.0])


def test_adaptive_entry_points_are_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "vimg_hip.h")).read()
    lib = abi.hip_lib()                       # loads on a machine without a GPU
    for name in ENTRY_POINTS:
        assert name + "(" in header, name
        assert name in abi.HIP_SYMBOLS, name
        assert hasattr(lib, name), name
    # the header states the statistic the restatement above follows
    for piece in ("0.212671f", "0.715160f", "0.072169f", "1e-3f", "float(K - 1)", "(b - m_old) * (b - m_new)"):
        assert piece in header, piece
    from vimg_amd import hip
    for method in ("render", "counts", "error", "state", "select", "render_adaptive", "launches"):
        assert hasattr(hip.Progressive, method), method


def test_ctypes_declarations_match_the_c_prototypes():
    """A C probe assigns every entry point to a pointer of the function type the ctypes table describes;
    the compiler refuses any mismatch (-Werror)."""
    ctype_of = {C.c_int: "int", C.c_uint64: "uint64_t", abi.u32: "uint32_t", abi.f32: "float", C.c_void_p: "void*",
                abi.PStats: "VimgRenderStats*", C.POINTER(abi.u32): "uint32_t*"}
    # the opaque handles (and the typed device pointers) travel as void* in ctypes: the probe names their C types
    handles = {"vimg_hip_progressive_render_masked": {0: "VimgDeviceScene*", 1: "VimgProgressive*", 3: "const uint8_t*"},
               "vimg_hip_progressive_launches": {0: "const VimgProgressive*"},
               "vimg_hip_progressive_state": {0: "VimgProgressive*"},
               "vimg_hip_progressive_error": {0: "VimgProgressive*"},
               "vimg_hip_progressive_select": {0: "VimgProgressive*", 3: "uint8_t*"}}
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


def test_argument_errors_are_answered_before_anything_is_enqueued():
    """No scene can reach a device here, so these are the checks that need neither: NULL handles and pointers
    answer VIMG_E_INVALID (-1) and say why.  (samples == 0, another scene's accumulator and a stale generation
    need a resident scene: tests/test_adaptive.py.)"""
    lib = abi.hip_lib()
    n = abi.u32(7)
    assert lib.vimg_hip_progressive_render_masked(None, None, 1, None, None, None, None) == -1
    assert b"null scene or accumulator" in lib.vimg_hip_last_error()
    st = abi.RenderStats()
    assert lib.vimg_hip_progressive_render_masked(None, None, 0, None, None, None, C.byref(st)) == -1
    assert lib.vimg_hip_progressive_state(None, None, None, None, None, None) == -1
    assert lib.vimg_hip_progressive_error(None, None, None) == -1
    assert b"null accumulator" in lib.vimg_hip_last_error()
    assert lib.vimg_hip_progressive_select(None, 0.05, 64, None, None, C.byref(n)) == -1
    assert n.value == 7                       # nothing was written
    assert lib.vimg_hip_progressive_launches(None) == 0
