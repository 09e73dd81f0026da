"""The PLAIN builds of render_cu_kernel (v-img_amd/csrc/plain_build.h): the launch-constant options of the
persistent loop compiled in.  They are the same source as the general build with constants substituted, so
every frame must be the general build's bit for bit, and the host must pick them for exactly the launches
their constants describe."""
import os
import subprocess

import numpy as np
import pytest

import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "v-img_amd", "csrc")

PLAIN_NAME, GENERAL_NAME = "render_cu_kernel<false>", "render_cu_kernel<false,general>"

# ---------------------------------------------------------------------------------------------- CPU
# The predicate is plain C++ (no HIP): a small program prints its answer for a table of launches.
# fields: cu_sched textured deep cu_waves stats force_general integrator pool_classes lds_leaf cu_flex single_x has_item_list
FLAGSHIP = dict(cu_sched=1, textured=0, deep=0, cu_waves=16, stats=0, force_general=0, integrator=3, pool_classes=3,
                lds_leaf=11, cu_flex=1, single_x=-1, has_item_list=0)
FIELDS = list(FLAGSHIP)
LAUNCHES = {
    "flagship": {},
    "flagship, thin shard (early rays)": dict(cu_flex=1 | 32),
    "material integrator": dict(integrator=2),
    "shading-normal integrator": dict(integrator=0),
    "geometric-normal integrator": dict(integrator=1),
    "two material classes": dict(pool_classes=2),
    "one material class": dict(pool_classes=1),
    "leaves in global memory": dict(lds_leaf=0),
    "trace_pixel": dict(single_x=5),
    "trace_pixel at x = 0": dict(single_x=0),
    "item list (masked progressive increment)": dict(has_item_list=1),
    "statistics launch": dict(stats=1),
    "cu_flex: walking waves never shade": dict(cu_flex=0),
    "cu_flex: shading at priority": dict(cu_flex=1 | 2),
    "cu_flex: walking at priority": dict(cu_flex=1 | 4),
    "cu_flex: no split batches": dict(cu_flex=1 | 16),
    "cu_flex: no split batches, early": dict(cu_flex=1 | 16 | 32),
    "lane scheduler": dict(cu_sched=0),
    "textured scene": dict(textured=1),
    "deep tree": dict(deep=1),
    "eight-wave workgroups": dict(cu_waves=8),
    "override: general build forced": dict(force_general=1),
    "override on a thin shard": dict(force_general=1, cu_flex=1 | 32),
}
PLAIN_EXPECTED = {"flagship", "flagship, thin shard (early rays)"}

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "plain_build.h"
int main(int argc, char** argv) {
  // rows of twelve integers, in the order of PlainLaunch's members
  for (int i = 1; i + 11 < argc; i += 12) {
    long v[12];
    for (int k = 0; k < 12; ++k) v[k] = atol(argv[i + k]);
    const vimg::PlainLaunch l{v[0] != 0, v[1] != 0, v[2] != 0, int(v[3]), v[4] != 0, v[5] != 0, uint32_t(v[6]), uint32_t(v[7]),
                              uint32_t(v[8]), uint32_t(v[9]), int(v[10]), v[11] != 0};
    std::printf("%d %d\n", vimg::plain_build_serves(l) ? 1 : 0, vimg::plain_build_serves(l, 0u) ? 1 : 0);
  }
  std::printf("fold %u\n", vimg::PLAIN_FOLD);
  return 0;
}
"""


def test_the_host_predicate_picks_plain_for_the_flagship_description_only(tmp_path):
    """plain_build_serves (the one predicate launch_policy.hip asks): each folded option off by one, the lane
    scheduler, a textured scene, a deep tree, trace_pixel, an item list, a statistics launch and the
    override all get the general build; the flagship description, late or early rays, gets PLAIN."""
    src, exe = tmp_path / "pred.cpp", tmp_path / "pred"
    src.write_text(PROGRAM)
    subprocess.run(["g++", "-std=c++20", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    names = list(LAUNCHES)
    argv = []
    for n in names:
        row = dict(FLAGSHIP, **LAUNCHES[n])
        argv += [str(row[f]) for f in FIELDS]
    out = subprocess.run([str(exe)] + argv, check=True, capture_output=True, text=True).stdout.split("\n")
    assert len(out) >= len(names) + 1
    fold = int(out[len(names)].split()[1])
    assert fold != 0, "the PLAIN builds fold nothing"
    got = {n for n, line in zip(names, out) if line.split()[0] == "1"}
    # a launch one folded option away from the flagship may keep PLAIN only if that option's bit is NOT folded
    bit_of = {"integrator": 1, "pool_classes": 2, "lds_leaf": 4, "single_x": 8, "has_item_list": 16, "cu_flex": 32}
    expected = set(PLAIN_EXPECTED)
    for n in names:
        changed = set(LAUNCHES[n])
        if changed and changed <= set(bit_of) and all(not (fold & bit_of[k]) for k in changed):
            expected.add(n)
    assert got == expected, (sorted(got - expected), sorted(expected - got))
    if fold == 63:
        assert got == PLAIN_EXPECTED
    # a build that folds nothing is served by every launch of the untextured CU build for trees in LDS
    nothing_folded = {n for n, line in zip(names, out) if line.split()[1] == "1"}
    assert nothing_folded == {n for n in names if not (set(LAUNCHES[n]) & {"cu_sched", "textured", "deep", "cu_waves", "stats", "force_general"})}


GLUE_PROGRAM = r"""
#include <cstdio>
#include "plain_build.h"
// the members plain_launch_of reads, under RenderArgs' names, with distinct values in the others
struct Args {
  unsigned integrator = 3, samples = 77, pool_classes = 3, pool_slots = 1280, lds_leaf = 11, lds_nodes = 82, cu_flex = 1, full_stats = 0;
  int single_x = -1, single_y = 5;
  const unsigned* item_list = nullptr;
  unsigned item_count = 9;
};
int main() {
  using namespace vimg;
  const unsigned list[1] = {0};
  int bad = 0;
  auto expect = [&](const char* what, const PlainLaunch& l, bool want) {
    if (plain_build_serves(l, 63u) != want) { std::printf("wrong: %s\n", what); ++bad; }
  };
  Args a;
  expect("flagship", plain_launch_of(true, false, false, 16, false, false, a), true);
  expect("lane", plain_launch_of(false, false, false, 16, false, false, a), false);
  expect("textured", plain_launch_of(true, true, false, 16, false, false, a), false);
  expect("deep", plain_launch_of(true, false, true, 16, false, false, a), false);
  expect("waves", plain_launch_of(true, false, false, 8, false, false, a), false);
  expect("stats flag", plain_launch_of(true, false, false, 16, true, false, a), false);
  expect("override", plain_launch_of(true, false, false, 16, false, true, a), false);
  { Args b = a; b.full_stats = 1; expect("full_stats argument", plain_launch_of(true, false, false, 16, false, false, b), false); }
  { Args b = a; b.integrator = 2; expect("integrator", plain_launch_of(true, false, false, 16, false, false, b), false); }
  { Args b = a; b.pool_classes = 2; expect("classes", plain_launch_of(true, false, false, 16, false, false, b), false); }
  { Args b = a; b.lds_leaf = 0; expect("leaf", plain_launch_of(true, false, false, 16, false, false, b), false); }
  { Args b = a; b.cu_flex = 1 | 16; expect("flex", plain_launch_of(true, false, false, 16, false, false, b), false); }
  { Args b = a; b.cu_flex = 1 | 32; expect("early", plain_launch_of(true, false, false, 16, false, false, b), true); }
  { Args b = a; b.single_x = 0; expect("single", plain_launch_of(true, false, false, 16, false, false, b), false); }
  { Args b = a; b.item_list = list; expect("items", plain_launch_of(true, false, false, 16, false, false, b), false); }
  // the members it must NOT read decide nothing
  { Args b = a; b.samples = 1; b.pool_slots = 8; b.lds_nodes = 0; b.single_y = -1; b.item_count = 0;
    expect("other members", plain_launch_of(true, false, false, 16, false, false, b), true); }
  std::printf("bad %d\n", bad);
  return bad;
}
"""


def test_the_launch_description_is_filled_from_the_arguments_it_names(tmp_path):
    """plain_launch_of (plain_build.h): what launch_policy.hip fills the predicate's PlainLaunch with, from the
    scene's and the launch's flags and the members of RenderArgs - each of them alone turns PLAIN off, the
    early bit and the members it has no business with do not."""
    src, exe = tmp_path / "glue.cpp", tmp_path / "glue"
    src.write_text(GLUE_PROGRAM)
    subprocess.run(["g++", "-std=c++20", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "bad 0", r.stdout


def test_the_library_exports_the_symbols_it_exported_before():
    """tests/golden/hip_exports.txt: the vimg_* symbols of the library before the PLAIN builds."""
    from vimg_amd import abi
    abi.hip_lib()
    lib = os.path.join(ROOT, "v-img_amd", "lib", "libvimg_hip.so")
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    have = sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("vimg_"))
    want = open(os.path.join(ROOT, "tests", "golden", "hip_exports.txt")).read().split()
    assert have == want


def test_the_plain_units_hold_one_untextured_kernel_each_without_scratch():
    """k_cu_plain.o / k_cu_plain_early.o as `make` left them: one kernel each, 0 bytes of scratch, no spilled
    vector register, within the 128 registers of four waves per SIMD."""
    from test_host_and_abi import _kernel_notes
    for unit, early in (("k_cu_plain.o", 0), ("k_cu_plain_early.o", 1)):
        notes = _kernel_notes(os.path.join(ROOT, "build", "hip", unit))
        if notes is None:
            pytest.skip("no build/hip objects or no binutils / llvm tools here")
        assert len(notes) == 1, sorted(notes)
        (name, n), = notes.items()
        assert f"render_cu_kernelILb0ELb0ELi16ELi4ELb0ELi{early}ELj" in name and not name.split("ELj")[1].startswith("0E"), name
        assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0 and n["vgpr_count"] <= 128, (name, n)


# ---------------------------------------------------------------------------------------------- GPU
def _dev(s, general=False, **opts):
    """A resident scene; `general`: uploaded under the override VIMG_HIP_PLAIN=0 (read once at upload)."""
    from vimg_amd import hip
    hip.init(0)
    old = os.environ.get("VIMG_HIP_PLAIN")
    try:
        if general:
            os.environ["VIMG_HIP_PLAIN"] = "0"
        else:
            os.environ.pop("VIMG_HIP_PLAIN", None)
        return hip.DeviceScene(s, **opts)
    finally:
        if old is None:
            os.environ.pop("VIMG_HIP_PLAIN", None)
        else:
            os.environ["VIMG_HIP_PLAIN"] = old


def _frame(d, p):
    import torch
    img = d.render(p, stats=False)      # (no statistics: the timed build, PLAIN or general)
    torch.cuda.synchronize()
    d.check()
    return img.cpu().numpy()


CASES = [("disney_spheres.json", (72, 40)), ("cornell_box_spheres.json", (64, 64))]
# Which build a launch runs.  At these sizes every pixel owns a slot, so the policy sets cu_flex bit 32 itself
# ("auto": the EARLY builds, k_cu_plain_early.hip against k_cu_early.hip, for the whole frame and the shard
# alike).  An explicit cu_flex = 1 keeps the policy from adding the bit and is the PLAIN builds' constant: "late"
# runs k_cu_plain.hip against k_cu.hip, the builds whole frames of config 2 are timed on.
VARIANTS = {"late": dict(cu_flex=1), "auto": {}}


@pytest.fixture(scope="module", params=[(c, v) for c in CASES for v in VARIANTS],
                ids=[f"{c[0].split('.')[0]}-{v}" for c in CASES for v in VARIANTS])
def pair(request):
    (name, res), variant = request.param
    s = scenes.json_scene(name, res=res)
    return name, s, _dev(s, **VARIANTS[variant]), _dev(s, general=True, **VARIANTS[variant])


@pytest.fixture(scope="module")
def reference_frames():
    """8 spp frames of the lane-bound kernel (no PLAIN build, no pool), one per scene: what every build must give."""
    out = {}
    for name, res in CASES:
        s = scenes.json_scene(name, res=res)
        d = _dev(s, scheduler="lane")
        out[name] = _frame(d, s.default_params(samples=8))
        d.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shard", [(1, 0), (8, 3)], ids=["whole", "eighth"])
def test_plain_and_general_builds_render_the_same_bits(pair, shard, reference_frames):
    """8 spp, the whole frame and the thin shard tile_world = 8, tile_rank = 3, on the late-ray builds (fixture
    "late": k_cu_plain.hip against k_cu.hip) and on the early-ray builds (fixture "auto": k_cu_plain_early.hip
    against k_cu_early.hip).  Frames without statistics run the two builds under test; the ray counts come
    from statistics launches, which run the statistics build on both scenes (the public API counts rays
    nowhere else) and must agree too.  The whole frame is also the lane-bound kernel's, bit for bit."""
    name, s, plain, general = pair
    p = s.default_params(samples=8, tile_world=shard[0], tile_rank=shard[1])
    assert plain.kernel_for(p) == PLAIN_NAME and general.kernel_for(p) == GENERAL_NAME
    a, b = _frame(plain, p), _frame(general, p)
    assert a.shape == b.shape and np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    if shard[0] == 1:
        assert np.array_equal(a.view(np.uint32), reference_frames[name].view(np.uint32))
    (ia, sa), (ib, sb) = plain.render(p), general.render(p)
    assert sa.closest_rays == sb.closest_rays and sa.shadow_rays == sb.shadow_rays and sa.rays == sb.rays and sa.rays > 0
    assert np.array_equal(ia.cpu().numpy().view(np.uint32), a.view(np.uint32))
    assert np.array_equal(ib.cpu().numpy().view(np.uint32), a.view(np.uint32))


@pytest.mark.gpu
def test_the_flagship_launch_itself_renders_the_general_builds_bits():
    """disney_spheres at its own 1800 x 800, 2 spp, options left to the policy: 5 625 pixels per compute unit
    are more than three pools' worth, so the policy queues rays late and this is the launch the benchmark
    times - k_cu_plain.hip, chosen by the policy itself, against k_cu.hip by override.  Compared on the GPU."""
    import torch
    s = scenes.json_scene("disney_spheres.json")
    p = s.default_params(samples=2)
    plain, general = _dev(s), _dev(s, general=True)
    assert plain.kernel_for(p) == PLAIN_NAME and general.kernel_for(p) == GENERAL_NAME
    a, b = plain.render(p, stats=False), general.render(p, stats=False)
    torch.cuda.synchronize()
    plain.check(), general.check()
    assert bool(torch.isfinite(a).all()) and float(a.max()) > 0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    plain.close(), general.close()


@pytest.mark.gpu
def test_launches_the_constants_do_not_describe_fall_through_to_the_general_build(pair):
    """The material integrator, a masked progressive increment (item list), trace_pixel and a statistics launch
    on a scene whose whole frames run PLAIN, with rays queued late and early (the fixture's two variants: the
    general builds of k_cu.hip and of k_cu_early.hip).  kernel_for sees a launch's parameters only: it names the
    general kernel for the material integrator; for the other three (which it cannot tell from a frame) the
    results must be those of a second call and of the scene uploaded under the override, where no PLAIN build
    ever runs - a PLAIN build given a list or a single pixel would ignore both."""
    import torch
    name, s, plain, general = pair
    # material integrator
    pm = s.default_params(samples=8, integrator="material")
    assert plain.kernel_for(pm) == GENERAL_NAME and general.kernel_for(pm) == GENERAL_NAME
    m1, m2, m3 = _frame(plain, pm), _frame(plain, pm), _frame(general, pm)
    assert np.array_equal(m1.view(np.uint32), m2.view(np.uint32)) and np.array_equal(m1.view(np.uint32), m3.view(np.uint32))
    assert not np.array_equal(m1, _frame(plain, s.default_params(samples=8)))
    # statistics launch: the event counts only the statistics build keeps
    p = s.default_params(samples=8)
    _, st1 = plain.render(p)
    _, st2 = plain.render(p)
    _, st3 = general.render(p)
    for st in (st2, st3):
        assert (st.rays, st.internal_visits, st.prim_tests) == (st1.rays, st1.internal_visits, st1.prim_tests)
    assert st1.internal_visits > 0 and st1.prim_tests > 0
    # trace_pixel: the pixel of the frame at the same sample count
    w, h = s.resolution
    frame = _frame(plain, p)
    for x, y in ((0, 0), (w // 2, h // 2), (w - 1, h - 1)):
        t1, t2, t3 = plain.trace_pixel(p, x, y), plain.trace_pixel(p, x, y), general.trace_pixel(p, x, y)
        assert np.array_equal(t1.view(np.uint32), t2.view(np.uint32)) and np.array_equal(t1.view(np.uint32), t3.view(np.uint32))
        assert np.array_equal(t1.view(np.uint32), frame[h - 1 - y, x].view(np.uint32))
    # a masked increment: 4 spp everywhere, 4 more where the mask is set
    mask = np.zeros((h, w), dtype=np.uint8)
    mask[::3, ::2] = 1
    outs = []
    for d in (plain, plain, general):
        acc = d.progressive(s.default_params(samples=1))
        acc.render(4)
        img = acc.render(4, mask=mask)
        torch.cuda.synchronize()
        d.check()
        outs.append(img.cpu().numpy())
        acc.close()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)) and np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))
    eight, four = _frame(plain, p), _frame(plain, s.default_params(samples=4))
    sel = mask.astype(bool)
    assert np.array_equal(outs[0][sel].view(np.uint32), eight[sel].view(np.uint32))
    assert np.array_equal(outs[0][~sel].view(np.uint32), four[~sel].view(np.uint32))
