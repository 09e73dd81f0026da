"""The walk's box pass as one wave-uniform loop with one exec region (render_cu_kernel.h, cu_mask /
cu_lanes and the selects at the end of a step; render_kernels.h, the triangle test's predicate from lane masks).  The
arithmetic, the visiting order and the event counts are what they were, so every frame is, bit for bit, the general
build's, the lane-bound kernel's and the oracle's pixel - on the flagship, on the flagship with a dielectric sphere
(the fourth vertex ring in use), after a material's type was edited on the resident scene, on the exact-slab
instantiation of the loop and on a ray that pops an empty stack at the root - and the statistics build counts the
oracle's visits with a pool of eight slots, where partial refills and pops of an empty stack are the rule.

The hand-over without the fourth vertex ring (plain_build.h: PF_NO_OTHER) is the PLAIN build of a scene that holds no
material of class 3: the flagship runs it, the flagship with a dielectric sphere runs the PLAIN build that keeps the
ring, and a material edit that brings the first such material moves the resident scene from the one to the other
(DeviceScene.plain_fold_for: the fold of the build a launch runs)."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import scenes
import vimg_amd
from test_lds_tables import GENERAL_NAME, PLAIN_NAME, _bits, _dev, _frame
from test_scene_relight_host import edited_materials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "v-img_amd", "csrc")
PF_NO_OTHER = 512          # plain_build.h (the CPU test below holds the header to it)

RES, SPP = (64, 32), 8
# which PLAIN build: left to the policy, a frame this small queues its rays early (k_cu_plain_early.hip); cu_flex = 1 by
# name is the late build whole frames are timed on (k_cu_plain.hip)
VARIANTS = {"auto": {}, "late": dict(cu_flex=1)}


def _flagship(res=RES):
    return scenes.json_scene("disney_spheres.json", res=res)


def _flagship_with_glass(res=RES):
    """disney_spheres.json and one dielectric sphere in front of the row of spheres: material class 3 occurs."""
    with open(os.path.join(scenes.SCENES, "disney_spheres.json")) as f:
        d = json.load(f)
    d["camera"]["resolution"] = [int(res[0]), int(res[1])]
    d["materials"].append({"type": "dielectric", "name": "glass", "ior": 1.5})
    d["surfaces"].append({"type": "sphere", "center": [0, -120, 180], "radius": 90, "mat_name": "glass"})
    return vimg_amd.HostScene.from_json_text(json.dumps(d))


PROGRAM = r"""
#include <cstdio>
#include "plain_build.h"
int main() {
  using namespace vimg;
  int bad = 0;
  auto expect = [&](const char* what, bool got, bool want) { if (got != want) { std::printf("wrong: %s\n", what); ++bad; } };
  static_assert(PF_NO_OTHER == 512u, "the bit the tests name");
  static_assert((PF_NO_OTHER & (PF_INTEGRATOR | PF_CLASSES | PF_LEAF_LDS | PF_SINGLE | PF_ITEMS | PF_FLEX | PF_TABLES | PF_LEAF_PERM)) == 0u, "a bit of its own");
  static_assert(PLAIN_FOLD_OTHER == (PLAIN_FOLD & ~PF_NO_OTHER), "the other fold differs in the bit alone");
  struct Args {
    unsigned integrator = 3, pool_classes = 3, lds_leaf = 11, cu_flex = 1, full_stats = 0;
    int single_x = -1;
    const unsigned* item_list = nullptr;
  } a;
  const PlainLaunch none = plain_launch_of(true, false, false, 16, false, false, a);
  const PlainLaunch some = plain_launch_of(true, false, false, 16, false, false, a, true);
  expect("no class 3: the folded build serves", plain_build_serves(none, 1023u), true);
  expect("class 3: the folded build does not serve", plain_build_serves(some, 1023u), false);
  expect("class 3: the build without the bit serves", plain_build_serves(some, 1023u & ~PF_NO_OTHER), true);
  expect("no class 3: the build without the bit would serve too", plain_build_serves(none, 1023u & ~PF_NO_OTHER), true);
  expect("the fold that serves, no class 3", plain_fold_serving(none) == PLAIN_FOLD, true);
  expect("the fold that serves, class 3", plain_fold_serving(some) == PLAIN_FOLD_OTHER, true);
  Args m = a; m.integrator = 2;
  expect("another integrator: neither", plain_fold_serving(plain_launch_of(true, false, false, 16, false, false, m, true)) == 0u,
         (PLAIN_FOLD & PF_INTEGRATOR) != 0u);
  expect("the override: neither", plain_fold_serving(plain_launch_of(true, false, false, 16, false, true, a)) == 0u, true);
  expect("the tables and the leaf copies do not read the bit", plain_tables_serve(0u, PF_NO_OTHER) && plain_leaf_perm_serves(0u, PF_NO_OTHER), true);
  std::printf("bad %d\n", bad);
  return bad;
}
"""


def test_the_predicate_of_the_build_without_the_fourth_ring(tmp_path):
    """plain_build_serves / plain_fold_serving (plain_build.h, compiled on its own): a scene with a material of class 3
    is served by the fold without PF_NO_OTHER and by no build that folds the bit."""
    import subprocess
    src, exe = tmp_path / "other.cpp", tmp_path / "other"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++20", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "bad 0", r.stdout


def _three_way(s, p, no_other, **opts):
    """The frame of the PLAIN build, of the general build and of the lane-bound kernel; `no_other`: whether the PLAIN
    build of this scene is the one without the fourth vertex ring."""
    plain, general, lane = _dev(s, **opts), _dev(s, general=True, **opts), _dev(s, scheduler="lane")
    assert plain.kernel_for(p) == PLAIN_NAME and general.kernel_for(p) == GENERAL_NAME
    assert lane.kernel_for(p).startswith("render_kernel<")
    fold = plain.plain_fold_for(p)
    assert fold != 0 and bool(fold & PF_NO_OTHER) == no_other, hex(fold)
    assert general.plain_fold_for(p) == 0 and lane.plain_fold_for(p) == 0
    a, b, c = _frame(plain, p), _frame(general, p), _frame(lane, p)
    for d in (plain, general, lane):
        d.close()
    return a, b, c


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_flagship_on_three_builds(variant):
    s = _flagship()
    a, b, c = _three_way(s, s.default_params(samples=SPP), True, **VARIANTS[variant])
    assert np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(a), _bits(c))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_flagship_with_a_dielectric_sphere_on_three_builds(variant):
    s = _flagship_with_glass()
    assert any(m.type == vimg_amd.abi.MAT_DIELECTRIC for m in s.materials())
    p = s.default_params(samples=SPP)
    a, b, c = _three_way(s, p, False, **VARIANTS[variant])
    assert np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(a), _bits(c))
    without = _dev(_flagship())
    assert not np.array_equal(_bits(a), _bits(_frame(without, p)))      # the sphere is in the picture
    without.close()


@pytest.mark.gpu
def test_a_principled_sphere_made_dielectric_on_the_resident_scene():
    """The material fields of update_geometry: the next launch leaves the build without the fourth ring, and its frame
    is a fresh upload's, on both builds; the edit taken back, the scene runs the folded build again."""
    s = _flagship()
    p = s.default_params(samples=SPP)
    d = _dev(s)
    assert d.plain_fold_for(p) & PF_NO_OTHER
    before = _frame(d, p)
    h = _flagship()
    assert h.materials()[5].type == vimg_amd.abi.MAT_PRINCIPLED
    h.set_materials(edited_materials(h, {5: ("dielectric", dict(ior=1.45))}))
    d.update_materials(materials=h.materials())
    fresh, general = _dev(h), _dev(h, general=True)
    assert d.kernel_for(p) == PLAIN_NAME and fresh.kernel_for(p) == PLAIN_NAME and general.kernel_for(p) == GENERAL_NAME
    for x in (d, fresh):
        fold = x.plain_fold_for(p)
        assert fold != 0 and not (fold & PF_NO_OTHER), hex(fold)
    after = _frame(d, p)
    assert not np.array_equal(_bits(after), _bits(before))
    assert np.array_equal(_bits(after), _bits(_frame(fresh, p)))
    assert np.array_equal(_bits(after), _bits(_frame(general, p)))
    d.update_materials(materials=s.materials())
    assert d.plain_fold_for(p) & PF_NO_OTHER
    assert np.array_equal(_bits(_frame(d, p)), _bits(before))
    for x in (d, fresh, general):
        x.close()


EXACT_RES, EXACT_VFOV = (64, 16), 28.072484970092773


def _exact_slab_scene():
    """The flagship seen from outside the box's open side by a camera turned 45 degrees about y whose horizontal
    half-width is 1 (aspect 4, vfov = 2 atan 1/4 as the float next to it that makes the product exact): the ray through
    the frame's corner (0, 0) runs in the plane x = const - its x component is w.x - 1 * u.x of two equal floats."""
    s = _flagship(EXACT_RES)
    s.set_camera((100.0, 250.0, 1500.0), (101.0, 250.0, 1499.0), (0, 1, 0), EXACT_VFOV, EXACT_RES)
    return s


@pytest.mark.gpu
def test_single_pixels_on_the_exact_slab_loop_and_on_an_empty_stack():
    """trace_pixel, 16 spp, against the oracle's pixel bit for bit.

    The exact-slab instantiation of the box loop runs for a whole wave when one of its lanes holds a ray with a
    direction component of exactly 0 (cu_walk: w_exact).  Sample 0 of pixel (0, 0) sits at the frame's corner (the R2
    offset of index px + py + sample = 0 is (0, 0): asserted), and the camera of _exact_slab_scene sends the ray through
    that corner with x component exactly 0: asserted on the GPU's own camera ray (probe CAMERA_RAY, the function the
    kernels generate their rays with) and on the oracle's.  Pixel (0, 0) therefore walks its first camera ray, and
    every lane that shares its passes, through box_loop(std::true_type).

    The camera inside the box looking out of its open side: the centre pixel's rays start inside the root's box and
    meet nothing - the first step pops an empty stack."""
    exact = _exact_slab_scene()
    p = exact.default_params(samples=16)
    assert O.r2(0) == (0.0, 0.0)
    corner = np.array([[0.0, 0.0, 0.25, 0.75]], dtype=np.float32)
    res = (65, 33)
    outward = _flagship(res)
    outward.set_camera((0.0, 0.0, 100.0), (0.0, 0.0, 1600.0), (0, 1, 0), 25.0, res)
    for what, s, pixels, lit in (("exact slab", exact, ((0, 0), (1, 0), (0, 1)), True),
                                 ("out of the box", outward, ((32, 16), (31, 17)), False)):
        d = _dev(s)
        if s is exact:
            for ray in (d.probe(O.PROBE_CAMERA_RAY, corner)[0], O.probe(s, O.PROBE_CAMERA_RAY, corner)[0]):
                print(f"camera ray through the corner: origin {ray[:3]}, direction {ray[3:6]}")
                assert ray[3] == 0.0 and ray[4] != 0.0 and ray[5] != 0.0, ray[3:6]
        for x, y in pixels:
            got, ref = d.trace_pixel(p, x, y), O.trace_pixel(s, p, x, y)
            print(f"{what} ({x}, {y}): GPU {got}, oracle {ref}")
            assert np.array_equal(_bits(got), _bits(ref)), (what, x, y, got, ref)
        centre = d.trace_pixel(p, *pixels[0])
        assert (centre.max() > 0) == lit, (what, centre)
        d.close()


@pytest.mark.gpu
def test_the_statistics_build_counts_the_oracles_visits_with_eight_slots():
    """P = 8 (pool_slots by name): refills of a few rays, box passes of a few lanes, pops of an empty stack."""
    s = _flagship()
    p = s.default_params(samples=SPP)
    cpu, cst, _ = O.render(s, p)
    d = _dev(s, scheduler="cu", pool_slots=8)
    gpu, gst = d.render_to_host(p)
    d.close()
    for k in ("internal_visits", "leaf_visits", "prim_tests", "sphere_tests"):
        print(f"{k}: GPU {getattr(gst, k)}, oracle {getattr(cst, k)}")
    assert gst.paths == cst.paths
    for k in ("internal_visits", "leaf_visits", "prim_tests", "sphere_tests"):
        assert getattr(gst, k) == getattr(cst, k) and getattr(gst, k) > 0, (k, getattr(gst, k), getattr(cst, k))
    assert np.array_equal(_bits(gpu), _bits(cpu))
