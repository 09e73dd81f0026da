"""The launch planner (v-img_amd/csrc/launch_plan.hip, cu_layout.h) on the CPU: it asks the GPU nothing, so a small host
program around it answers for any scene facts, parameters and options.

tests/golden/cu_launch_plans.json holds, for every case of CASES below, the inputs and the complete plan the commit
before the planner was split from the device scene made of them (tests/golden/make_cu_launch_plans.py; recorded there
around launch_policy.hip compiled for the host alone, with stub kernel getters).  The planner must make the same plans;
a test of the record itself says what it covers, and a seeded sweep asserts the layout's invariants."""
import json
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "v-img_amd", "csrc")
RECORD = os.path.join(ROOT, "tests", "golden", "cu_launch_plans.json")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

FACTS = ["res_x", "res_y", "num_nodes", "max_depth", "num_cus", "num_leaf_prims", "num_tris", "num_spheres", "num_meshes",
         "num_materials", "textured", "too_wide", "force_general", "no_lds_tables", "has_other", "waves_per_simd"]
PARAMS = ["integrator", "samples", "depth", "tile_rank", "tile_world"]
CALL = ["sx", "sy", "lane_per_cu"]
# (VimgHipOptions behind struct_size, in its order, under "o_" so that no name is taken twice)
OPTIONS = ["scheduler", "waves_per_simd", "lds_budget_kb", "pool_slots", "pool_segments", "pool_refill", "pool_vbatch",
           "pool_classes", "pool_starve", "pool_boxmin", "lds_leaf", "stage_slots", "stage_seg_len", "stage_wchunk",
           "stage_walk_quota", "pool4_rays", "lds_stack", "pool_gbreak", "cu_waves", "cu_walkers", "cu_flex", "cu_lowwater",
           "cu_patience", "cu_join", "cu_sleep"]
FIELDS = FACTS + PARAMS + CALL + ["o_" + o for o in OPTIONS]
TABS = ["prims", "tri_shade", "spheres", "material_flags", "meshes", "materials", "dmaterials"]
ARGS = ["integrator", "samples", "depth", "tile_rank", "tile_world", "tiles_x", "tiles_y", "num_local_tiles", "full_stats",
        "stack_entries", "lds_nodes", "stack_lds", "lds_leaf", "pool_segments", "pool_seg_len", "pool_epoch", "pool_slots",
        "pool_refill", "pool_vbatch", "pool_boxmin", "pool_starve", "pool_gbreak", "pool_classes", "cu_walkers", "cu_flex",
        "cu_lowwater", "cu_patience", "cu_join", "cu_sleep", "cu_watchdog", "cu_magic_v", "cu_shift_v", "cu_magic_w",
        "cu_shift_w", "single_x", "single_y", "sample_base", "spp_div", "item_count", "lds_tables"]
PLAN = (["error", "grid", "lds_bytes", "table_bytes", "sched", "wps", "deep", "feature", "cold_bytes", "ovf_bytes"]
        + ["a_" + a for a in ARGS] + ["tab_off_" + t for t in TABS] + ["tab_rows_" + t for t in TABS]
        + ["a_leaf_perm", "a_leaf_perm_off", "a_leaf_perm_stride", "plain_fold", "plain_fold_stats", "kernel"])
# behind the plan with --layout: where cu_layout puts the regions of the plan's workgroup
REGIONS = ["stacks", "recs", "hitx", "ring_v", "ring_w", "tq", "ctl", "wave_recs", "leaf", "end"]

SCHED_LANE, SCHED_CU = 1, 6
MIS, MATERIAL, ALBEDO, COVERAGE = 3, 2, 4, 9
LDS_LIMIT = 160 * 1024
ERRORS = {
    "both": "options: lds_budget_kb and lds_stack together are beyond the compute unit's 160 KB of LDS",
    "nodes": "options: lds_budget_kb is beyond the compute unit's 160 KB of LDS",
    "stack": "options: lds_stack is beyond the compute unit's 160 KB of LDS",
}

# A small untextured scene whose tree, leaves and tables all fit the LDS, a whole 1800 x 800 frame on 256 compute units
BASE = dict(res_x=1800, res_y=800, num_nodes=82, max_depth=10, num_cus=256, num_leaf_prims=40, num_tris=24, num_spheres=16,
            num_meshes=2, num_materials=5, textured=0, too_wide=0, force_general=0, no_lds_tables=0, has_other=0,
            waves_per_simd=2, integrator=MIS, samples=64, depth=8, tile_rank=0, tile_world=1, sx=-1, sy=-1, lane_per_cu=1,
            **{"o_" + o: -1 for o in OPTIONS})
BIG_TREE = dict(num_nodes=200000, max_depth=40, num_leaf_prims=400000, num_tris=400000, num_spheres=0, num_meshes=30,
                num_materials=40)


def _named_cases():
    c = {"base": {}}
    for w, h in ((1, 1), (8, 8), (136, 72)):
        c[f"frame {w}x{h}"] = dict(res_x=w, res_y=h)
    for tw in (2, 3, 4, 8):
        c[f"tile_world {tw}"] = dict(tile_world=tw)
        c[f"tile_world {tw}, last rank"] = dict(tile_world=tw, tile_rank=tw - 1)
    c["nodes 83: one beyond the budget"] = dict(num_nodes=83)
    c["max_depth 30"] = dict(max_depth=30)
    c["max_depth 31: one beyond the LDS stack"] = dict(max_depth=31)
    c["leaves 85"] = dict(num_leaf_prims=85, num_tris=30, num_spheres=55)
    c["leaves 86"] = dict(num_leaf_prims=86, num_tris=30, num_spheres=56)
    c["big tree"] = dict(BIG_TREE)
    c["big tree, textured"] = dict(BIG_TREE, textured=1)
    for tw in (2, 4, 8):
        c[f"big tree, tile_world {tw}"] = dict(BIG_TREE, tile_world=tw)
    c["big tree, 304 CUs, tile_world 8"] = dict(BIG_TREE, num_cus=304, tile_world=8)
    c["big tree, pool_boxmin 4, tile_world 8"] = dict(BIG_TREE, tile_world=8, o_pool_boxmin=4)
    c["all the LDS for slots: no room for tables"] = dict(o_pool_slots=4096)
    c["material integrator: no PLAIN build"] = dict(integrator=MATERIAL)
    c["shading normals"] = dict(integrator=0)
    c["geometric normals"] = dict(integrator=1)
    c["no triangles"] = dict(num_tris=0, num_spheres=40, num_meshes=0)
    c["no spheres"] = dict(num_tris=40, num_spheres=0)
    c["node budget shrunk to 1 KB"] = dict(max_depth=73, o_lds_stack=75, o_cu_walkers=8, num_leaf_prims=4000, num_tris=4000,
                                           num_spheres=0)
    # the stacks shrink in rounds: beside the case itself, what the first attempt needs (lds_stack as the policy starts)
    # and the layout one round arrives at, which is still too large
    budget = dict(num_nodes=1800, max_depth=30, o_lds_budget_kb=100)
    c["stack shrink"] = dict(budget)
    c["stack shrink: the first attempt"] = dict(budget, o_lds_stack=32)
    c["stack shrink: one round"] = dict(budget, o_lds_stack=25)
    c["stack shrink, 120 KB of nodes"] = dict(BIG_TREE, o_lds_budget_kb=120)
    c["error: both"] = dict(BIG_TREE, o_lds_budget_kb=200, o_lds_stack=32)
    c["error: lds_budget_kb"] = dict(BIG_TREE, o_lds_budget_kb=200)
    c["error: lds_stack"] = dict(max_depth=98, o_lds_stack=100)
    c["error: lds_budget_kb, largest"] = dict(BIG_TREE, num_nodes=1 << 26, o_lds_budget_kb=1 << 30)
    c["pool_segments 3"] = dict(o_pool_segments=3)
    c["pool_segments 3, tile_world 4"] = dict(o_pool_segments=3, tile_world=4)
    c["pool_segments 10000"] = dict(o_pool_segments=10000, samples=100000)
    c["no local tiles"] = dict(res_x=8, res_y=8, tile_world=2, tile_rank=1)
    c["no local tiles, lane"] = dict(res_x=8, res_y=8, tile_world=2, tile_rank=1, o_scheduler=SCHED_LANE)
    c["trace_pixel"] = dict(sx=5, sy=7)
    c["trace_pixel at 0 0"] = dict(sx=0, sy=0)
    c["trace_pixel, big tree"] = dict(BIG_TREE, sx=900, sy=400)
    c["trace_pixel, lane"] = dict(sx=5, sy=7, o_scheduler=SCHED_LANE)
    for s in (1, 3, 4, 512, 4096):
        c[f"samples {s}"] = dict(samples=s)
        c[f"samples {s}, tile_world 3"] = dict(samples=s, tile_world=3)
    off = dict(scheduler=SCHED_CU, waves_per_simd=3, lds_budget_kb=2, pool_slots=256, pool_segments=2, pool_refill=4,
               pool_vbatch=32, pool_classes=2, pool_starve=8, pool_boxmin=4, lds_leaf=0, stage_slots=5, stage_seg_len=5,
               stage_wchunk=5, stage_walk_quota=5, pool4_rays=5, lds_stack=4, pool_gbreak=5, cu_waves=8, cu_walkers=12,
               cu_flex=17, cu_lowwater=32, cu_patience=2, cu_join=4, cu_sleep=8)
    assert list(off) == OPTIONS
    for o, v in off.items():
        c[f"option {o} {v}"] = {"o_" + o: v}
    more = dict(lds_budget_kb=(0, 1, 40), pool_slots=(0, 8, 9, 1000), pool_refill=(0,), pool_vbatch=(0, 200), pool_classes=(0, 1, 7),
                pool_starve=(0, 200), pool_boxmin=(0, 200), lds_leaf=(1,), lds_stack=(0, 1, 11, 12, 64), cu_walkers=(0, 1, 16, 40),
                cu_flex=(0, 1, 3, 32, 33), cu_lowwater=(0,), cu_patience=(0,), cu_join=(0,), cu_sleep=(0, 500))
    for o, vs in more.items():
        for v in vs:
            c[f"option {o} {v}"] = {"o_" + o: v}
            if o in ("lds_budget_kb", "lds_stack", "cu_walkers", "pool_slots"):
                c[f"option {o} {v}, big tree"] = dict(BIG_TREE, **{"o_" + o: v})
    c["lane by name"] = dict(o_scheduler=SCHED_LANE)
    c["lane by name, 3 waves per SIMD by the scene"] = dict(o_scheduler=SCHED_LANE, waves_per_simd=3)
    c["lane by name, waves_per_simd 3"] = dict(o_scheduler=SCHED_LANE, o_waves_per_simd=3)
    c["lane by name, waves_per_simd 2"] = dict(o_scheduler=SCHED_LANE, waves_per_simd=3, o_waves_per_simd=2)
    c["lane by name, big tree"] = dict(BIG_TREE, o_scheduler=SCHED_LANE, waves_per_simd=3)
    c["lane by name, big tree, textured"] = dict(BIG_TREE, o_scheduler=SCHED_LANE, textured=1)
    for kb in (1, 8, 64, 160):
        c[f"lane by name, big tree, lds_budget_kb {kb}"] = dict(BIG_TREE, o_scheduler=SCHED_LANE, o_lds_budget_kb=kb)
    c["lane by name, max_depth 60"] = dict(o_scheduler=SCHED_LANE, max_depth=60)
    c["lane by name, 136x72"] = dict(o_scheduler=SCHED_LANE, res_x=136, res_y=72)
    c["too wide"] = dict(res_x=70000, res_y=16, too_wide=1)
    c["too wide, textured"] = dict(res_x=70000, res_y=16, too_wide=1, textured=1)
    for flag in ("textured", "force_general", "no_lds_tables", "has_other"):
        c[flag] = {flag: 1}
        c[flag + ", tile_world 4"] = {flag: 1, "tile_world": 4}
    c["has_other, no tables"] = dict(has_other=1, no_lds_tables=1)
    c["textured, 86 leaves"] = dict(textured=1, num_leaf_prims=86, num_tris=86, num_spheres=0)
    for i in range(ALBEDO, COVERAGE + 1):
        c[f"feature integrator {i}"] = dict(integrator=i)
    c["feature integrator, textured"] = dict(integrator=ALBEDO, textured=1)
    c["feature integrator, big tree, CU by name"] = dict(BIG_TREE, integrator=COVERAGE, o_scheduler=SCHED_CU)
    c["feature integrator, trace_pixel"] = dict(integrator=ALBEDO, sx=3, sy=4)
    for cus in (1, 8, 64, 304):
        c[f"{cus} CUs"] = dict(num_cus=cus)
        c[f"{cus} CUs, 136x72"] = dict(num_cus=cus, res_x=136, res_y=72)
    return c


def _pick(rng, values):
    return values[rng.randrange(len(values))]


def random_case(rng):
    """One input of the sweeps: every field from a short list around the policy's thresholds, each option off its
    default one time in five."""
    c = {}
    c["res_x"], c["res_y"] = _pick(rng, ((1, 1), (8, 8), (20, 12), (136, 72), (640, 360), (1800, 800), (4096, 2160)))
    if rng.randrange(4) == 0:
        c["res_x"], c["res_y"] = 1 + rng.randrange(3000), 1 + rng.randrange(1500)
    c["num_nodes"] = _pick(rng, (1, 2, 18, 19, 36, 82, 83, 731, 5000, 3000000))
    c["max_depth"] = _pick(rng, (1, 2, 3, 10, 29, 30, 31, 32, 45, 62))
    c["num_cus"] = _pick(rng, (1, 8, 64, 256, 304))
    leaves = _pick(rng, (1, 2, 11, 40, 85, 86, 1000, 4000000))
    tris = _pick(rng, (0, leaves // 2, leaves))
    c.update(num_leaf_prims=leaves, num_tris=tris, num_spheres=leaves - tris, num_meshes=0 if tris == 0 else 1 + rng.randrange(4),
             num_materials=1 + rng.randrange(12))
    for flag in ("textured", "force_general", "no_lds_tables", "has_other"):
        c[flag] = int(rng.randrange(5) == 0)
    c["waves_per_simd"] = 2 + rng.randrange(2)
    c["integrator"] = MIS if rng.randrange(3) else rng.randrange(COVERAGE + 1)
    c["samples"] = _pick(rng, (1, 2, 4, 16, 64, 512, 10000))
    c["tile_world"] = _pick(rng, (1, 1, 2, 3, 4, 8, 64))
    c["tile_rank"] = rng.randrange(c["tile_world"])
    if rng.randrange(8) == 0:
        c["sx"], c["sy"] = rng.randrange(c["res_x"]), rng.randrange(c["res_y"])
    values = dict(scheduler=(SCHED_LANE, SCHED_CU), waves_per_simd=(2, 3), lds_budget_kb=(0, 1, 2, 4, 16, 40, 100, 150, 400),
                  pool_slots=(0, 1, 8, 15, 100, 1000, 1280, 4096, 100000), pool_segments=(0, 1, 2, 7, 64, 5000), pool_refill=(0, 1, 2, 64),
                  pool_vbatch=(0, 1, 32, 100), pool_classes=(0, 1, 2, 3, 4), pool_starve=(0, 1, 64, 100), pool_boxmin=(0, 4, 8, 100),
                  lds_leaf=(0, 1), lds_stack=(0, 1, 2, 4, 16, 31, 32, 33, 64, 200), cu_walkers=(0, 1, 4, 8, 10, 15, 16, 17),
                  cu_flex=(0, 1, 3, 5, 16, 17, 32, 33), cu_lowwater=(0, 1, 1000), cu_patience=(0, 9), cu_join=(0, 9), cu_sleep=(0, 9, 1000))
    for o in OPTIONS:
        if rng.randrange(5) == 0:
            c["o_" + o] = _pick(rng, values.get(o, (0, 5)))
    return c


def _cases():
    c = _named_cases()
    rng = random.Random(20250)
    for i in range(160):
        c[f"random {i}"] = random_case(rng)
    return {name: [dict(BASE, **over)[f] for f in FIELDS] for name, over in c.items()}


CASES = _cases()

# The program around the planner: a case per line of FIELDS on stdin, its plan as one JSON array (PLAN) per line on stdout
PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "cu_layout.h"
#include "launch_plan.h"
using namespace vimg;
using Facts = LaunchFacts;
static void fill_facts(Facts& f, const long* v, const VimgHipOptions& o) {
  f.res_x = int(v[0]), f.res_y = int(v[1]), f.num_nodes = uint32_t(v[2]), f.max_depth = uint32_t(v[3]);
  f.num_cus = uint32_t(v[4]), f.num_leaf_prims = uint32_t(v[5]), f.num_tris = uint32_t(v[6]), f.num_spheres = uint32_t(v[7]);
  f.num_meshes = uint32_t(v[8]), f.num_materials = uint32_t(v[9]);
  f.textured = v[10] != 0, f.too_wide = v[11] != 0, f.force_general = v[12] != 0, f.no_lds_tables = v[13] != 0, f.has_other = v[14] != 0;
  f.waves_per_simd = int(v[15]);
  f.opt = o;
}
static LaunchCfg plan(const Facts& f, const VimgRenderParams& p, int sx, int sy, int per_cu) { return plan_launch(f, p, sx, sy, per_cu); }
static uint32_t fold(const Facts& f, const LaunchCfg& c, bool stats) { return plain_fold_of(f, c, stats); }
static const char* name(const Facts& f, const VimgRenderParams& p) { return launch_kernel_name(f, p); }
static void print_layout(const LaunchCfg& c) {
  const RenderArgs& a = c.args;
  const CuLayout l = cu_layout(a.lds_nodes, a.cu_walkers, cu_stack_rows_of(a.stack_entries, a.stack_lds), a.pool_slots, CU_WAVES, a.lds_leaf);
  std::printf(",%u,%u,%u,%u,%u,%u,%u,%u,%u,%u", l.stacks, l.recs, l.hitx, l.ring_v, l.ring_w, l.tq, l.ctl, l.wave_recs, l.leaf, l.end);
}
// one case per line of 49 integers on stdin (tests/test_launch_plan.py: FIELDS); one JSON array per case on stdout
int main(int argc, char** argv) {
  const bool layout = argc > 1 && !std::strcmp(argv[1], "--layout");
  long v[49];
  for (;;) {
    for (int k = 0; k < 49; ++k)
      if (std::scanf("%ld", &v[k]) != 1) return k == 0 ? 0 : 1;
    VimgHipOptions o{};
    o.struct_size = uint32_t(sizeof(o));
    int32_t* of = &o.scheduler;
    for (int k = 0; k < 25; ++k) of[k] = int32_t(v[24 + k]);
    Facts f{};
    fill_facts(f, v, o);
    const VimgRenderParams p{uint32_t(v[16]), uint32_t(v[17]), uint32_t(v[18]), uint32_t(v[19]), uint32_t(v[20])};
    const LaunchCfg c = plan(f, p, int(v[21]), int(v[22]), int(v[23]));
    const RenderArgs& a = c.args;
    if (c.error) std::printf("[\"%s\"", c.error); else std::printf("[null");
    std::printf(",%u,%u,%u,%d,%d,%d,%d,%zu,%zu", c.grid, c.lds_bytes, c.table_bytes, c.sched, c.wps, int(c.deep), int(c.feature),
                c.cold_bytes, c.ovf_bytes);
    const uint32_t u[] = {a.integrator, a.samples, a.depth, a.tile_rank, a.tile_world, a.tiles_x, a.tiles_y, a.num_local_tiles,
                          a.full_stats, a.stack_entries, a.lds_nodes, a.stack_lds, a.lds_leaf, a.pool_segments, a.pool_seg_len,
                          a.pool_epoch, a.pool_slots, a.pool_refill, a.pool_vbatch, a.pool_boxmin, a.pool_starve, a.pool_gbreak,
                          a.pool_classes, a.cu_walkers, a.cu_flex, a.cu_lowwater, a.cu_patience, a.cu_join, a.cu_sleep,
                          a.cu_watchdog, a.cu_magic_v, a.cu_shift_v, a.cu_magic_w, a.cu_shift_w};
    for (uint32_t x : u) std::printf(",%u", x);
    std::printf(",%d,%d,%u,%.9g,%u,%u", a.single_x, a.single_y, a.sample_base, double(a.spp_div), a.item_count, a.lds_tables);
    for (uint32_t t = 0; t < TAB_COUNT; ++t) std::printf(",%u", a.tab_off[t]);
    for (uint32_t t = 0; t < TAB_COUNT; ++t) std::printf(",%u", a.tab_rows[t]);
    std::printf(",%u,%u,%u,%u,%u,\"%s\"", a.leaf_perm, a.leaf_perm_off, a.leaf_perm_stride, fold(f, c, false), fold(f, c, true), name(f, p));
    if (layout) print_layout(c);
    std::printf("]\n");
  }
}
"""


def build_program(directory):
    """Compiles PROGRAM with the planner for the host alone; returns the executable."""
    src, exe = os.path.join(directory, "plans.hip"), os.path.join(directory, "plans")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([HIPCC, "--cuda-host-only", "-std=c++20", "-O1", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"),
                    "-I", CSRC, src, os.path.join(CSRC, "launch_plan.hip"), "-o", exe], check=True)
    return exe


def run_plans(exe, inputs, layout=False):
    """The plans of `inputs` (rows of FIELDS), each a list in PLAN's order (REGIONS behind it with `layout`)."""
    text = "".join(" ".join(str(int(x)) for x in row) + "\n" for row in inputs)
    out = subprocess.run([exe] + (["--layout"] if layout else []), input=text, check=True, capture_output=True, text=True).stdout
    plans = [json.loads(line) for line in out.splitlines()]
    assert len(plans) == len(inputs)
    return plans


def record_text(plans):
    """The record of CASES with their `plans`, as the file holds it."""
    rows = ",\n".join(f"{json.dumps(name)}:{json.dumps([CASES[name], plan], separators=(',', ':'))}" for name, plan in zip(CASES, plans))
    return (f'{{"fields":{json.dumps(FIELDS, separators=(",", ":"))},\n"plan":{json.dumps(PLAN, separators=(",", ":"))},\n'
            f'"cases":{{\n{rows}\n}}}}\n')


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return build_program(str(tmp_path_factory.mktemp("launch_plan")))


@pytest.fixture(scope="module")
def record():
    with open(RECORD) as f:
        return json.load(f)


def test_every_recorded_plan_is_made_again(planner, record):
    """Every case of the record, through the planner as it is now: the complete plan - error, grid, LDS and scratch
    bytes, every scalar of RenderArgs, the serving PLAIN fold without and with statistics, the kernel's name."""
    assert record["fields"] == FIELDS and record["plan"] == PLAN
    assert {n: v[0] for n, v in record["cases"].items()} == CASES, "the record's inputs are not CASES: make it again on the commit it pins"
    names = list(record["cases"])
    got = run_plans(planner, [record["cases"][n][0] for n in names])
    wrong = {}
    for n, g in zip(names, got):
        want = record["cases"][n][1]
        if g != want:
            wrong[n] = {f: (w, h) for f, w, h in zip(PLAN, want, g) if w != h}
    assert not wrong, wrong


def _eligible(i, p):
    """What the policy knows of a launch that a PLAIN build could serve (plain_build.h: plain_build_serves)."""
    return (p["sched"] == SCHED_CU and p["error"] is None and not i["textured"] and not p["deep"] and not i["force_general"]
            and p["a_integrator"] == MIS and p["a_pool_classes"] == 3 and p["a_lds_leaf"] != 0 and p["a_single_x"] < 0
            and (p["a_cu_flex"] & ~32) == 1)


def test_the_record_covers_the_policy(record):
    """The record holds a case on either side of every threshold of the policy, so that a planner that moves one cannot
    make all its plans again."""
    rows = {n: (dict(zip(FIELDS, v[0])), dict(zip(PLAN, v[1]))) for n, v in record["cases"].items()}
    assert 100 <= len(rows) <= 400

    def some(pred):
        return [n for n, (i, p) in rows.items() if pred(i, p)]

    def cu(i, p):
        return p["sched"] == SCHED_CU and p["error"] is None

    def auto(i, *options):
        return all(i["o_" + o] == -1 for o in options)

    def per_group(i, p):
        items = 1 if i["sx"] >= 0 else p["a_num_local_tiles"] * 64
        return -(-items // i["num_cus"])

    def tables_room(i, p):   # table groups and leaf copies may be asked for
        return _eligible(i, p) and not i["no_lds_tables"]

    covered = {
        # tree depth: 82 nodes fill the 4 608-byte budget, 32 entries the LDS stack
        "82 nodes in LDS": lambda i, p: cu(i, p) and i["num_nodes"] == 82 and p["a_lds_nodes"] == 82 and not p["deep"],
        "83 nodes: deep": lambda i, p: cu(i, p) and i["num_nodes"] == 83 and p["a_lds_nodes"] == 82 and p["deep"] and i["max_depth"] <= 30,
        "max_depth 30": lambda i, p: cu(i, p) and i["max_depth"] == 30 and not p["deep"] and auto(i, "lds_stack"),
        "max_depth 31: deep": lambda i, p: cu(i, p) and i["max_depth"] == 31 and p["deep"] and i["num_nodes"] <= 82 and p["a_stack_lds"] == 32,
        "85 leaves in LDS": lambda i, p: cu(i, p) and i["num_leaf_prims"] == 85 and p["a_lds_leaf"] == 85,
        "86 leaves stay out": lambda i, p: cu(i, p) and i["num_leaf_prims"] == 86 and p["a_lds_leaf"] == 0 and auto(i, "lds_leaf"),
        "8 walkers": lambda i, p: cu(i, p) and auto(i, "cu_walkers") and p["a_cu_walkers"] == 8 and not p["deep"],
        "10 walkers": lambda i, p: cu(i, p) and auto(i, "cu_walkers") and p["a_cu_walkers"] == 10 and p["deep"],
        "every wave walks": lambda i, p: cu(i, p) and auto(i, "cu_walkers") and p["a_cu_walkers"] == 16,
        "1 280-slot cap": lambda i, p: cu(i, p) and auto(i, "pool_slots") and p["a_pool_slots"] == 1280 and per_group(i, p) * 10 >= 1280 * 27,
        "2.7 pools": lambda i, p: cu(i, p) and auto(i, "pool_slots") and p["a_pool_slots"] == (per_group(i, p) * 10 // 27) & ~7
                                  and p["a_pool_slots"] < per_group(i, p),
        "slots by pixels": lambda i, p: cu(i, p) and auto(i, "pool_slots") and p["a_pool_slots"] == (per_group(i, p) + 8) & ~7 and p["a_pool_slots"] > 8,
        "early rays by policy": lambda i, p: cu(i, p) and auto(i, "cu_flex") and p["a_cu_flex"] & 32,
        "no early rays": lambda i, p: cu(i, p) and auto(i, "cu_flex") and not p["a_cu_flex"] & 32,
        "pool_boxmin 8": lambda i, p: cu(i, p) and auto(i, "pool_boxmin") and p["a_pool_boxmin"] == 8,
        "pool_boxmin 16 on a deep tree": lambda i, p: cu(i, p) and auto(i, "pool_boxmin") and p["a_pool_boxmin"] == 16 and p["deep"],
        "tables staged": lambda i, p: cu(i, p) and p["a_lds_tables"] == 64 and p["table_bytes"] > 0 and p["tab_off_prims"] > 0,
        "tables: no room": lambda i, p: tables_room(i, p) and p["a_lds_tables"] == 0,
        "tables: no PLAIN build": lambda i, p: cu(i, p) and not _eligible(i, p) and not i["no_lds_tables"] and p["a_lds_tables"] == 0
                                               and not p["deep"] and not i["textured"] and p["a_pool_slots"] <= 1280,
        "leaf copies staged": lambda i, p: cu(i, p) and p["a_leaf_perm"] == 1 and p["a_leaf_perm_stride"] == 48 * p["a_lds_leaf"] > 0
                                           and p["a_leaf_perm_off"] >= p["a_leaf_perm_stride"],
        "leaf copies: no triangles": lambda i, p: cu(i, p) and i["num_tris"] == 0 and p["a_leaf_perm"] == 1 and p["a_leaf_perm_stride"] == 0
                                                  and p["a_leaf_perm_off"] == 0,
        "leaf copies: no room": lambda i, p: _eligible(i, p) and i["num_tris"] > 0 and p["a_leaf_perm"] == 0,
        "nodes shrunk to 1 KB": lambda i, p: cu(i, p) and auto(i, "lds_budget_kb") and p["a_lds_nodes"] == 1024 // 56 < min(i["num_nodes"], 82),
        "error: both": lambda i, p: p["error"] == ERRORS["both"],
        "error: lds_budget_kb": lambda i, p: p["error"] == ERRORS["nodes"],
        "error: lds_stack": lambda i, p: p["error"] == ERRORS["stack"],
        "segments": lambda i, p: cu(i, p) and auto(i, "pool_segments") and p["a_pool_segments"] > 1,
        "pool_segments option": lambda i, p: cu(i, p) and i["o_pool_segments"] > 1 and p["a_pool_segments"] == i["o_pool_segments"],
        "no local tiles": lambda i, p: cu(i, p) and p["a_num_local_tiles"] == 0 and i["sx"] < 0,
        "trace_pixel": lambda i, p: cu(i, p) and p["a_single_x"] >= 0 and p["grid"] == 1,
        "lane by name": lambda i, p: i["o_scheduler"] == SCHED_LANE and p["sched"] == SCHED_LANE and not p["feature"] and not i["too_wide"],
        "lane: too wide": lambda i, p: i["too_wide"] and auto(i, "scheduler") and p["sched"] == SCHED_LANE and p["kernel"].startswith("render_kernel<"),
        "feature integrator": lambda i, p: p["feature"] and p["kernel"].startswith("feature_kernel<"),
        "general build by name": lambda i, p: p["kernel"] == "render_cu_kernel<false,general>",
        "PLAIN build, other materials": lambda i, p: i["has_other"] and p["plain_fold"] != 0 and p["plain_fold"] & 512 == 0,
        "PLAIN build": lambda i, p: p["plain_fold"] & 512 and p["plain_fold_stats"] == 0 and p["kernel"] == "render_cu_kernel<false>",
    }
    for flag in ("textured", "force_general", "no_lds_tables", "has_other"):
        covered["flag " + flag] = lambda i, p, flag=flag: cu(i, p) and i[flag]
    for o in OPTIONS:
        covered["option " + o] = lambda i, p, o=o: i["o_" + o] != -1
    for w, h in ((1, 1), (8, 8), (136, 72)):
        covered[f"frame {w}x{h}"] = lambda i, p, w=w, h=h: cu(i, p) and (i["res_x"], i["res_y"]) == (w, h)
    for tw in (1, 2, 3, 4, 8):
        covered[f"1800x800 at tile_world {tw}"] = lambda i, p, tw=tw: cu(i, p) and (i["res_x"], i["res_y"], i["tile_world"]) == (1800, 800, tw)
    missing = [what for what, pred in covered.items() if not some(pred)]
    assert not missing, missing

    # the stacks shrink in at least two rounds: the first attempt (the policy's 32 entries, named) says by how much it is
    # too large; the stack one round arrives at from there is too large again; the policy's own answer lies below it
    (i0, first), (i1, one), (_, final) = rows["stack shrink: the first attempt"], rows["stack shrink: one round"], rows["stack shrink"]
    assert first["error"] == ERRORS["both"] and first["a_stack_lds"] == 32
    per_row = first["a_cu_walkers"] * 256
    assert i1["o_lds_stack"] == 32 - -(-(first["lds_bytes"] - LDS_LIMIT) // per_row) - 1
    assert one["error"] == ERRORS["both"] and one["lds_bytes"] > LDS_LIMIT
    assert final["error"] is None and 1 <= final["a_stack_lds"] < i1["o_lds_stack"] and final["lds_bytes"] <= LDS_LIMIT


def _magic_is_exact(d, magic, shift, rng):
    ns = [0, 1, d - 1, d, 2 ** 31 - 1] + [rng.randrange(2 ** 31) for _ in range(100)]
    return all(((n * magic) >> 32) >> shift == n // d for n in ns)


def test_a_sweep_of_inputs_keeps_the_layouts_invariants(planner):
    """About 2 000 seeded inputs: whatever the policy is asked, a plan without error fits the compute unit, its regions
    ascend without overlap to lds_bytes, what is read in 16-byte words is aligned, the ring divisions are exact, and
    only a named option can make a launch impossible."""
    rng = random.Random(4242)
    inputs = [[dict(BASE, **random_case(rng))[f] for f in FIELDS] for _ in range(2000)]
    plans = run_plans(planner, inputs, layout=True)
    seen = dict(cu=0, error=0, tables=0, perm=0, deep=0)
    for row, out in zip(inputs, plans):
        i, p, r = dict(zip(FIELDS, row)), dict(zip(PLAN, out)), dict(zip(REGIONS, out[len(PLAN):]))
        if p["sched"] != SCHED_CU:
            assert p["error"] is None and p["lds_bytes"] <= max(40, i["o_lds_budget_kb"]) * 1024 + 4 * 256 * p["a_stack_entries"], (i, p)
            continue
        seen["cu"] += 1
        if p["error"] is not None:
            seen["error"] += 1
            assert i["o_lds_budget_kb"] != -1 or i["o_lds_stack"] != -1, (i, p)
            assert p["lds_bytes"] > LDS_LIMIT, (i, p)
            continue
        assert p["lds_bytes"] <= LDS_LIMIT, (i, p)
        slots = p["a_pool_slots"]
        assert slots % 8 == 0 and 8 <= slots <= 4096, (i, p)
        # the regions in the carve's order, each as large as the kernel makes it
        stack_rows = p["a_stack_lds"] + 1 if p["a_stack_lds"] < p["a_stack_entries"] else p["a_stack_entries"]
        sizes = [("stacks", p["a_cu_walkers"] * stack_rows * 256), ("recs", 4 * 16 * slots), ("hitx", 8 * slots), ("ring_v", 4 * 2 * slots),
                 ("ring_w", 2 * 2 * slots), ("tq", 4 * slots), ("ctl", 96), ("wave_recs", 16 * 416), ("leaf", 48 * p["a_lds_leaf"])]
        assert r["stacks"] >= 56 * p["a_lds_nodes"] and r["stacks"] % 256 == 0, (i, p, r)
        for (name, size), nxt in zip(sizes, REGIONS[1:]):
            assert r[name] + size <= r[nxt], (name, i, p, r)
        for name in ("stacks", "recs", "ctl", "leaf", "end"):
            assert r[name] % 16 == 0, (name, i, p, r)
        # behind them the tail: the tables of the staged groups in staging order, then the two leaf copies
        at = r["end"]
        for t, row_bytes in zip(TABS, (8, 64, 32, 4, 48, 80, 304)):   # (device_scene.h: tab_row_bytes)
            if not p["a_lds_tables"] & (64 if TABS.index(t) < 5 else 128):
                assert p["tab_off_" + t] == 0 and p["tab_rows_" + t] == 0, (t, i, p)
                continue
            assert p["tab_off_" + t] == at and at % 16 == 0, (t, i, p, r)
            at += (p["tab_rows_" + t] * row_bytes + 15) & ~15
        if p["a_lds_tables"]:
            seen["tables"] += 1
        if p["a_leaf_perm_stride"]:
            seen["perm"] += 1
            assert p["a_leaf_perm"] == 1 and p["a_leaf_perm_stride"] == 48 * p["a_lds_leaf"], (i, p)
            assert (r["leaf"] + p["a_leaf_perm_off"]) % 16 == 0 and p["a_leaf_perm_off"] >= p["a_leaf_perm_stride"], (i, p, r)
            assert r["leaf"] + p["a_leaf_perm_off"] + 2 * p["a_leaf_perm_stride"] == p["lds_bytes"], (i, p, r)
            assert r["leaf"] + p["a_leaf_perm_off"] == at, (i, p, r)
            at += 2 * p["a_leaf_perm_stride"]
        else:
            assert p["a_leaf_perm_off"] == 0, (i, p)
        assert at == p["lds_bytes"], (i, p, r)
        assert p["lds_bytes"] - p["table_bytes"] == r["end"], (i, p, r)   # table_bytes is the tail of the layout
        assert _magic_is_exact(slots, p["a_cu_magic_v"], p["a_cu_shift_v"], rng), (i, p)
        assert _magic_is_exact(2 * slots, p["a_cu_magic_w"], p["a_cu_shift_w"], rng), (i, p)
        seen["deep"] += p["deep"]
    assert seen["cu"] > 1000 and min(seen.values()) >= 10, seen   # (the sweep reaches every kind of plan it speaks of)
