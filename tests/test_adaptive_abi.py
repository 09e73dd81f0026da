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


# ---- the statistic from its definition, float64: what the float32 expressions above are supposed to estimate ------
U = 2.0 ** -24                                 # unit roundoff of float32
# (the kernel's weights ARE these float32 numbers: the model takes them as exact inputs, like the sums)
LUM64 = np.array([F(0.212671), F(0.715160), F(0.072169)], dtype=np.float64)
# the increment lengths of the long runs (tests/test_adaptive.py runs the same four on a device)
SEQUENCES = {"128x4": (4,) * 128, "256x1": (1,) * 256, "32x16": (16,) * 32, "unequal": (1, 7, 64, 3, 128, 5, 2, 90)}


def model_stat(sums, ns):
    """The statistic of a pixel whose float32 running sums were sums[0] = 0, sums[1], ..., sums[K] ([K + 1, ..., 3])
    after increments of ns[0], ..., ns[K - 1] samples, in float64 and from the definition - not from adapt_m2:
    b_i = Y(S_i - S_{i-1}) / n_i, N = sum n_i, m = Y(S_K) / N, M2 = sum n_i (b_i - m)^2 in closed form (the
    incremental form equals it exactly in real arithmetic), err = sqrt(M2 / (K - 1) / N) / (|m| + 1e-3).
    Returns (N, m, M2, err, bound), `bound` the derived limit of |M2_float32 - M2| (m2_bound)."""
    s = np.asarray(sums, dtype=np.float64)
    ns = np.asarray(ns, dtype=np.float64)
    k, n_all = len(ns), ns.sum()
    assert s.shape[0] == k + 1 and k >= 2 and not s[0].any()
    shape = (k,) + (1,) * (s.ndim - 2)
    b = ((s[1:] - s[:-1]) @ LUM64) / ns.reshape(shape)
    m = (s[-1] @ LUM64) / n_all
    m2 = (ns.reshape(shape) * (b - m) ** 2).sum(axis=0)
    err = np.sqrt(m2 / (k - 1) / n_all) / (np.abs(m) + 1e-3)
    return n_all, m, m2, err, m2_bound(s, ns)


def m2_bound(s, ns):
    """How far the float32 M2 of include/vimg_hip.h may lie from model_stat's, derived (u = 2^-24), not fitted.
    b = ((x1 - x0) w0 + (y1 - y0) w1 + (z1 - z0) w2) / float(n) is a subtraction, a product, two additions and a
    division on exact inputs - five roundings on a sum of terms of one sign (sums of radiance only grow) - and m_old,
    m_new are four (float(N) is exact below 2^24): each is off by at most 6 u of itself, so a difference b - m_x is
    off by at most 12 u L, L = max(|b|, |m_old|, |m_new|), before its own rounding.  The term n (b - m_old)(b - m_new)
    is then off by n 12 u L (|b - m_old| + |b - m_new| + 12 u L) from the two perturbed factors, and by 4 u |term|
    from its own four roundings (two subtractions, two products).  Adding it to M2 rounds once more: u |M2|.  The
    bound is the sum of the three over the increments.  It is absolute: on a pixel whose samples nearly agree M2 is
    some 1e-8 m^2 and the first part dominates it."""
    s, ns = np.asarray(s, dtype=np.float64), np.asarray(ns, dtype=np.float64)
    bound, m2, n_old = 0.0, 0.0, 0.0
    for i, n in enumerate(ns):
        b = ((s[i + 1] - s[i]) @ LUM64) / n
        m_old = (s[i] @ LUM64) / n_old if n_old else 0.0 * b
        m_new = (s[i + 1] @ LUM64) / (n_old + n)
        big = np.maximum(np.abs(b), np.maximum(np.abs(m_old), np.abs(m_new)))
        term = n * (b - m_old) * (b - m_new)
        m2 = m2 + term
        bound = bound + n * 12 * U * big * (np.abs(b - m_old) + np.abs(b - m_new) + 12 * U * big) + 4 * U * np.abs(term) \
            + U * np.abs(m2)
        n_old += n
    return bound


def check_against_model(what, sums, ns, m2_f32, err_f32):
    """|M2_float32 - M2| <= bound and the matching limit of err, no extra factor; prints the worst ratios.  Returns
    (worst |dM2| / bound, worst |dM2| / M2)."""
    n_all, m, m2, err, bound = model_stat(sums, ns)
    k = len(ns)
    d = np.abs(np.asarray(m2_f32, dtype=np.float64) - m2)
    ratio = float(np.max(np.where(bound > 0, d / np.where(bound > 0, bound, 1), np.where(d > 0, np.inf, 0.0))))
    pos = m2 > 0
    rel = float(np.max(d[pos] / m2[pos])) if pos.any() else 0.0
    e = np.asarray(err_f32, dtype=np.float64)
    e_lim = np.where(pos, err * (8 * U + 0.5 * bound / np.where(pos, m2, 1)), np.sqrt(bound / (k - 1) / n_all) / (np.abs(m) + 1e-3))
    e_off = np.where(pos, np.abs(e - err), e)
    e_ratio = float(np.max(np.where(e_lim > 0, e_off / np.where(e_lim > 0, e_lim, 1), np.where(e_off > 0, np.inf, 0.0))))
    print(f"{what}: worst |M2_f32 - M2_f64| / bound {ratio:.3f}, worst relative error of M2 {rel:.3e}, "
          f"worst |err_f32 - err_f64| / its limit {e_ratio:.3f}")
    assert (d <= bound).all(), (what, "M2", ratio)
    assert (e_off <= e_lim).all(), (what, "err", e_ratio)
    return ratio, rel


def restatement_over(sums, ns):
    """stat_update over the whole sequence (every pixel selected every time), then stat_error: (N, K, M2, err)."""
    shape = np.asarray(sums[0]).shape[:-1]
    n, k, m2 = np.zeros(shape, np.uint32), np.zeros(shape, np.uint32), np.zeros(shape, F)
    for i, inc in enumerate(ns):
        n, k, m2 = stat_update(n, k, m2, sums[i], sums[i + 1], inc, np.ones(shape, bool))
    return n, k, m2, stat_error(n, k, m2, sums[-1])


def synthetic_sums(kind, ns, pixels, seed):
    """Float32 running sums [K + 1, pixels, 3] of per-sample radiances added one by one in float32, as the render
    kernels add them: gamma-distributed noise; near-constant (relative spread 1e-4); 1 % fireflies of x 1e4."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.05, 2.0, (pixels, 3)).astype(F)
    run = np.zeros((pixels, 3), F)
    sums = [run.copy()]
    for n in ns:
        if kind == "near-constant":
            y = base * (F(1) + F(1e-4) * (F(2) * rng.random((n, pixels, 3), dtype=F) - F(1)))
        else:
            y = base * (F(0.5) * rng.standard_gamma(2.0, (n, pixels, 3), dtype=F))
            if kind == "firefly":
                y = y * np.where(rng.random((n, pixels, 1), dtype=F) < F(0.01), F(1e4), F(1))
        for sample in y:
            run = run + sample
        sums.append(run.copy())
    return np.stack(sums)


def test_the_model_is_the_textbook_standard_error():
    """With every increment one sample long, err (|m| + 1e-3) is the standard error of the mean of the samples'
    luminances: np.std(y, ddof=1) / sqrt(N)."""
    ns = (1,) * 200
    sums = synthetic_sums("noisy", ns, 50, 7)
    n_all, m, m2, err, _ = model_stat(sums, ns)
    y = (sums[1:].astype(np.float64) - sums[:-1].astype(np.float64)) @ LUM64
    assert n_all == 200
    assert np.allclose(m, y.mean(axis=0), rtol=1e-12, atol=0)
    assert np.allclose(err * (np.abs(m) + 1e-3), np.std(y, axis=0, ddof=1) / np.sqrt(200), rtol=1e-12, atol=0)


def test_the_float32_statistic_stays_within_its_derived_bound_of_the_float64_model():
    """The incremental float32 M2 and err, after the 8 to 256 increments of SEQUENCES, against model_stat on 20 000
    synthetic pixels of each kind; the bound is m2_bound's, derived there.  Figures of this test (the worst over
    all twelve cases): DESIGN.md 4.14."""
    worst, rel_noisy, rel_const = 0.0, 0.0, 0.0
    for kind in ("noisy", "near-constant", "firefly"):
        for j, (name, ns) in enumerate(SEQUENCES.items()):
            sums = synthetic_sums(kind, ns, 20000, 100 + j)
            n, k, m2, err = restatement_over(sums, ns)
            assert (n == sum(ns)).all() and (k == len(ns)).all()
            ratio, rel = check_against_model((kind, name), sums, ns, m2, err)
            worst = max(worst, ratio)
            if kind == "noisy":
                rel_noisy = max(rel_noisy, rel)
            if kind == "near-constant":
                rel_const = max(rel_const, rel)
    print(f"all cases: worst |dM2| / bound {worst:.3f}; worst relative error of M2: noisy {rel_noisy:.2e}, "
          f"near-constant {rel_const:.2e}")


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
