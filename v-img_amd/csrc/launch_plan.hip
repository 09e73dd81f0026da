// The launch planner: which kernel family a launch runs and with what grid, LDS layout and scheduler parameters.
// Policy (AUTO): the CU-wide scheduler (render_cu_kernel) for every launch - whole frames, thin shards, trace_pixel.
// The lane-bound kernel runs when asked for by name and for frames wider than the 16-bit pixel coordinates of the slot
// records.  The feature integrators (ALBEDO .. COVERAGE) have one kernel, feature_kernel, in the lane launch's shape,
// whatever the scheduler option says.
// Host arithmetic only: no HIP runtime call, no kernel, no device scene (launch_plan.h; launch_policy.hip is the HIP
// side).  The workgroup's LDS is laid out by cu_layout.h, as the kernel carves it.
#include "launch_plan.h"

#include <algorithm>
#include <cmath>

#include "cu_layout.h"
#include "plain_build.h"

namespace vimg {

uint32_t local_tiles(const LaunchFacts& f, const VimgRenderParams& p) {
  const uint32_t total = tiles_of(f.res_x) * tiles_of(f.res_y);
  if (p.tile_rank >= total) return 0;
  return (total - p.tile_rank + p.tile_world - 1) / p.tile_world;
}

namespace {

// what every launch builder fills the same way
RenderArgs base_args(const LaunchFacts& f, const VimgRenderParams& p, int sx, int sy) {
  const VimgHipOptions& o = f.opt;
  RenderArgs a{};
  a.integrator = p.integrator;
  a.samples = p.samples;
  a.spp_div = static_cast<float>(p.samples);   // (a progressive launch sets the base and the divisor of its total)
  a.depth = p.depth;
  a.tile_rank = p.tile_rank;
  a.tile_world = p.tile_world;
  a.tiles_x = tiles_of(f.res_x);
  a.tiles_y = tiles_of(f.res_y);
  a.num_local_tiles = local_tiles(f, p);
  a.full_stats = 0;
  a.single_x = sx;
  a.single_y = sy;
  a.stack_entries = f.max_depth + 2;
  a.stack_ovf = nullptr;
  a.pool_refill = 16u;
  a.pool_vbatch = std::min(64u, std::max(1u, opt_or(o.pool_vbatch, 64u)));
  a.pool_boxmin = std::min(64u, opt_or(o.pool_boxmin, 16u));
  a.pool_segments = 1;
  a.pool_seg_len = p.samples;
  return a;
}

// Splits a pixel's samples into segments handed out as separate work items (sets pool_segments, pool_seg_len;
// returns the length): about `per_gen` segments per pool generation of the frame, at most `most`
uint32_t segments_for(const LaunchFacts& f, const VimgRenderParams& p, uint64_t items, uint64_t in_flight, double per_gen,
                      double most, RenderArgs* a) {
  const double gens = double(items) / double(in_flight);
  uint32_t k = gens >= 10.0 ? 1u : uint32_t(std::min(most, std::max(1.0, std::floor(per_gen / gens + 0.5))));
  k = std::min<uint32_t>(k, std::max<uint32_t>(p.samples / 4u, 1u));
  if (items * 2u < in_flight * 3u) k = 1u;
  if (f.opt.pool_segments != VIMG_OPT_AUTO) k = uint32_t(std::max(1, f.opt.pool_segments));
  k = std::min<uint32_t>(k, 4096u);
  while (k > 1u && items * k >= 0xfff00000ull) --k;   // (segment, pixel) items must fit the 32-bit counter
  const uint32_t len = std::max<uint32_t>((p.samples + k - 1) / k, 1u);
  a->pool_seg_len = len;
  a->pool_segments = std::max<uint32_t>((p.samples + len - 1) / len, 1u);
  return len;
}

// n / d == mulhi(n, magic) >> shift for every n < 2^31 (Granlund & Montgomery, "Division by invariant
// integers using multiplication", fig. 4.1 with N = 31): the ring index of render_cu_kernel's tickets
void magic_div(uint32_t d, uint32_t* magic, uint32_t* shift) {
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;   // ceil(log2 d), d >= 2
  *magic = static_cast<uint32_t>((1ull << (31u + l)) / d + 1ull);
  *shift = l - 1u;
}

// The launch of the CU-wide scheduler (render_cu_kernel.h): one workgroup of CU_WAVES waves per compute unit,
// a pool of as many slots as the CU's LDS holds behind the top of the tree, the
// walking waves' stacks and the rings - never more than the launch has pixels per workgroup.
// `node_budget`: bytes of LDS for the top of the tree; `stack_cap`: most stack entries of a lane kept in LDS
// (make_launch_cu below decides both)
LaunchCfg cu_launch_with(const LaunchFacts& f, const VimgRenderParams& p, int sx, int sy, uint32_t node_budget, uint32_t stack_cap) {
  LaunchCfg c{};
  const VimgHipOptions& o = f.opt;
  const uint64_t items = (sx >= 0) ? 1 : uint64_t(local_tiles(f, p)) * 64u;
  c.sched = VIMG_SCHED_CU;
  c.wps = 4;
  RenderArgs& a = c.args = base_args(f, p, sx, sy);
  a.stack_lds = std::min(a.stack_entries, std::max(1u, stack_cap));
  // walking waves: five of eight by policy (config 2: the walk is 60 % of the wave cycles); when every
  // wave walks, every wave must be allowed to shade too
  a.cu_walkers = 0;   // (set below, once the tree's place is known)
  a.cu_flex = opt_or(o.cu_flex, 1u);   // (bit 1 / 2: shading / walking at wave priority 1; bit 4: no split batches; bit 5: early rays, by policy below)
  a.cu_lowwater = std::max(1u, opt_or(o.cu_lowwater, 64u));
  a.cu_patience = opt_or(o.cu_patience, 4u);
  a.cu_join = std::max(1u, opt_or(o.cu_join, 1u));
  a.cu_sleep = std::min(127u, std::max(1u, opt_or(o.cu_sleep, 4u)));
  a.pool_starve = std::min(64u, std::max(1u, opt_or(o.pool_starve, 16u)));   // smallest partial batch worth a wave at once
  a.pool_classes = std::min(3u, std::max(1u, opt_or(o.pool_classes, 3u)));
  // LDS of the workgroup: the whole CU's, minus a margin
  constexpr uint32_t share = CU_LDS_LIMIT - CU_LDS_MARGIN;
  a.lds_nodes = std::min(node_budget / CU_NODE_BYTES, f.num_nodes);
  // the build with the overflow path and the global node fetch serves both trees beyond the LDS
  // node cache and stacks deeper than their LDS rows
  c.deep = a.lds_nodes < f.num_nodes || a.stack_lds < a.stack_entries;
  // walking waves: trees in LDS 8 of 16.  It was 9 (profiles/r3_cu/sweeps.txt, config 2 at 512 spp: 8 waves 307,
  // 9: 304, 10: 325, 11: 337 ms) until the late builds stopped walking shadow rays whose light sample adds zero
  // (render_cu_kernel.h: ELIDE): 7 % fewer rays for the same shading, and 8: 243.0, 9: 258.1, 10: 267.5 ms
  // (profiles/r9_nee_elide/); trees in global memory 10 (stand-ins of configs 4 / 5 at 32 spp:
  // 8 waves 2 650 / 3 436, 10: 2 796 / 4 019, 12: 2 649 / 3 762 Mrays/s); when every wave walks, every
  // wave must be allowed to shade too
  a.cu_walkers = std::min(CU_WAVES, std::max(1u, opt_or(o.cu_walkers, c.deep ? 10u : 8u)));
  // finished rays that send a walking wave to its rings (hand-over, then refill): 16 on trees in LDS; on
  // trees in global memory, where a pass waits for memory and a finished ray would wait with it, 2
  // (stand-ins of configs 4 / 5: an eighth of the frame at 128 spp 82.8 / 77.9 against 93.3 / 82.3 ms,
  // a quarter 87.7 against 92.2, a half 101.9 against 107.8, the whole frame unchanged)
  a.pool_refill = std::max(1u, opt_or(o.pool_refill, c.deep ? 2u : 16u));
  const uint32_t stack_rows = cu_stack_rows_of(a.stack_entries, a.stack_lds);
  a.lds_leaf = (f.num_leaf_prims * CU_LEAF_BYTES <= 4096u && o.lds_leaf != 0) ? f.num_leaf_prims : 0u;
  // the workgroup's regions (cu_layout.h) with so many walking waves and slots
  auto layout_with = [&](uint32_t walkers, uint32_t slots) { return cu_layout(a.lds_nodes, walkers, stack_rows, slots, CU_WAVES, a.lds_leaf); };
  auto slots_with = [&](uint32_t walkers) {
    const uint32_t fixed = layout_with(walkers, 0u).end + CU_LDS_SLACK;
    uint32_t n = share > fixed ? (share - fixed) / CU_LDS_BYTES : 0u;
    n = std::min(n, 4096u);
    // (trees in LDS: the rate is flat from 1 152 slots on - config 2 at 512 spp: 896 slots 323, 1 024: 305,
    // 1 152: 297.7, 1 280: 297.7, 1 408: 298.4, all 1 490 the LDS holds: 300.2 ms; smaller cold regions stay in L2)
    if (!c.deep && o.pool_slots == VIMG_OPT_AUTO) n = std::min(n, 1280u);
    if (o.pool_slots != VIMG_OPT_AUTO) n = std::min(n, uint32_t(std::max(0, o.pool_slots)));
    return n;
  };
  // never more slots than the launch has pixels per workgroup (a thin shard's pixels each own a slot
  // from the first sample to the last)
  const uint64_t per_group = (items + f.num_cus - 1) / f.num_cus;
  // a launch whose pixels all own a slot, on a tree in LDS: every wave walks AND shades (a quarter of
  // config 2: 135.0 against 142.4 ms; an eighth and a third: no difference)
  if (o.cu_walkers == VIMG_OPT_AUTO && !c.deep && o.pool_slots == VIMG_OPT_AUTO && per_group + 8u <= slots_with(CU_WAVES)) a.cu_walkers = CU_WAVES;
  if (a.cu_walkers == CU_WAVES) a.cu_flex |= 1u;
  uint32_t slots = slots_with(a.cu_walkers);
  // ... and when the pixels are more than the slots but fewer than 2.7 pools' worth (half a frame of
  // config 2), a pool of pixels / 2.7: the segments of a pixel are handed from slot to slot, and a
  // slot that draws a segment whose predecessor is still running can only wait - with 1.65
  // generations of slots per pixel half of config 2 took 253 ms, with 2.7 (1 040 slots) 176, with 3.5 180
  if (o.pool_slots == VIMG_OPT_AUTO && per_group > slots && per_group * 10u < uint64_t(slots) * 27u)
    slots = static_cast<uint32_t>(per_group * 10u / 27u);
  slots = static_cast<uint32_t>(std::min<uint64_t>(slots, per_group + 8u));
  slots = std::max(slots & ~7u, 8u);
  // EARLY rays (cu_flex bit 5: a vertex stage queues each ray as soon as it is known and finishes beside
  // the walk) wherever a slot's hop latency is on the frame's critical path: launches of fewer than three
  // pools' worth of pixels, and trees in global memory (whose walks are long).  Config 2: an eighth 110.4 ->
  // 99.9 ms, a quarter 132.5 -> 118.3, a half 170.6 -> 164.5, the whole frame 300.4 -> 309.7 (it only pays the
  // two extra ring operations per vertex: off there); stand-ins of configs 4 / 5: whole frame 121.4 -> 118.4 /
  // 127.0 -> 124.1, an eighth 81.3 -> 79.4 / 76.8 -> 69.9
  if (o.cu_flex == VIMG_OPT_AUTO && (c.deep || per_group * 10u <= uint64_t(slots) * 30u)) a.cu_flex |= 32u;
  // a tree in global memory on a launch whose pixels all own a slot: the box loop yields to waiting leaves
  // below 8 descending lanes instead of 16 (stand-ins of configs 4 / 5, a quarter at 128 spp: 79.3 / 69.9
  // against 80.8 / 72.7 ms, an eighth 76.7 / 65.5 against 76.9 / 70.1; halves and whole frames want 16)
  if (c.deep && o.pool_boxmin == VIMG_OPT_AUTO && per_group + 8u >= slots && per_group <= slots) a.pool_boxmin = 8u;
  a.pool_slots = slots;
  magic_div(slots, &a.cu_magic_v, &a.cu_shift_v);
  magic_div(2u * slots, &a.cu_magic_w, &a.cu_shift_w);
  const CuLayout lay = layout_with(a.cu_walkers, slots);
  c.lds_bytes = lay.end;
  // The launch-constant shading tables of a small scene behind the leaf records (render_cu_kernel.h: stage_tables),
  // in the room the pool leaves: group by group (hit records, then materials), each whole or not at all, and
  // never at the price of a slot - the pool is sized first.  Only for the builds that read them from there: a launch
  // that, as far as the policy knows it here, a PLAIN build serves, by the groups those builds fold (enqueue_render
  // takes the tables out again where statistics or an item list send the launch to another build: drop_unread_tables).
  // VIMG_HIP_LDS_TABLES=0 at upload: none.
  a.lds_tables = 0u;
  c.table_bytes = 0u;
  if (!f.no_lds_tables && plain_build_serves(plain_launch_of(true, f.textured, c.deep, int(CU_WAVES), false, f.force_general, a))) {
    const uint32_t n_mat = f.num_materials;
    uint32_t rows[TAB_COUNT];
    rows[TAB_PRIMS] = f.num_leaf_prims, rows[TAB_TRI_SHADE] = f.num_tris, rows[TAB_SPHERES] = f.num_spheres;
    rows[TAB_MATERIAL_FLAGS] = n_mat, rows[TAB_MESHES] = f.num_meshes;
    rows[TAB_MATERIALS] = n_mat, rows[TAB_DMATERIALS] = n_mat;
    static const struct { uint32_t bit, first, end; } groups[2] = {{PF_TAB_HIT, TAB_PRIMS, TAB_MATERIALS}, {PF_TAB_MAT, TAB_MATERIALS, TAB_COUNT}};
    const uint64_t used = uint64_t(c.lds_bytes) + CU_LDS_SLACK;
    uint64_t room = share > used ? share - used : 0u;
    for (const auto& gr : groups) {
      if (!(PLAIN_FOLD & gr.bit)) continue;
      uint64_t bytes = 0;
      for (uint32_t t = gr.first; t < gr.end; ++t) bytes += (uint64_t(rows[t]) * tab_row_bytes(t) + 15u) & ~uint64_t(15);
      if (bytes > room) continue;
      for (uint32_t t = gr.first; t < gr.end; ++t) {
        a.tab_off[t] = c.lds_bytes, a.tab_rows[t] = rows[t];
        c.lds_bytes += (rows[t] * tab_row_bytes(t) + 15u) & ~15u;
      }
      c.table_bytes += uint32_t(bytes);
      room -= bytes;
      a.lds_tables |= gr.bit;
    }
  }
  // The permuted copies of the leaf records (plain_build.h: PF_LEAF_PERM; render_cu_kernel.h: stage_leaf_perm) are one
  // more group by the same rules: behind the table groups, in the room pool and tables leave, both copies or none,
  // never at the price of a slot or of a table group, and only for a launch a PLAIN build serves.  A scene without
  // triangles needs none (the sphere test permutes nothing): its launch is ready with a layout that is the parent's.
  a.leaf_perm = 0u, a.leaf_perm_off = 0u, a.leaf_perm_stride = 0u;
  if ((PLAIN_FOLD & PF_LEAF_PERM) && a.lds_leaf != 0u &&
      plain_build_serves(plain_launch_of(true, f.textured, c.deep, int(CU_WAVES), false, f.force_general, a))) {
    const uint64_t used = uint64_t(c.lds_bytes) + CU_LDS_SLACK;
    const uint32_t stride = a.lds_leaf * CU_LEAF_BYTES;
    if (f.num_tris == 0u) {
      a.leaf_perm = 1u;
    } else if (used + 2u * uint64_t(stride) <= share) {
      a.leaf_perm = 1u;
      a.leaf_perm_off = c.lds_bytes - lay.leaf, a.leaf_perm_stride = stride;
      c.lds_bytes += 2u * stride;
      c.table_bytes += 2u * stride;
    }
  }
  // one workgroup is a whole compute unit: the grid has one per CU, never more than the work (the runtime is asked
  // nothing: its answer for a kernel of 1 024 threads could only ever be one)
  const uint64_t need_blocks = (items + slots - 1) / slots;
  c.grid = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(need_blocks, f.num_cus)));
  // segments (the tail of a frame is one segment long)
  a.cu_watchdog = static_cast<uint32_t>(1000000000ull >> 20);
  if (sx < 0) {
    const uint32_t len = segments_for(f, p, items, uint64_t(c.grid) * slots, 176.0, 64.0, &a);
    a.cu_watchdog = static_cast<uint32_t>(std::min<uint64_t>((1000000000ull + 5000000ull * len) >> 20, 0x7fffffffull));   // 10 s + 50 ms per sample of a segment
  }
  return c;
}

// The one place that fits a CU launch into the compute unit's LDS.  What the policy chooses itself gives way to what
// the caller asked for: past the workgroup's share the node cache shrinks first (to the 1 KB the smallest option
// gives), then the stack entries kept in LDS (to one), each only where its option was left to the policy.  A launch
// that still cannot fit has its options to blame: c.error names the one, and nothing is launched (VIMG_E_INVALID).
LaunchCfg make_launch_cu(const LaunchFacts& f, const VimgRenderParams& p, int sx, int sy) {
  const VimgHipOptions& o = f.opt;
  const bool own_nodes = o.lds_budget_kb == VIMG_OPT_AUTO, own_stack = o.lds_stack == VIMG_OPT_AUTO;
  uint32_t node_budget = own_nodes ? 4608u : uint32_t(std::min(std::max(1, o.lds_budget_kb), 1 << 20)) * 1024u;
  uint32_t stack_cap = opt_or(o.lds_stack, 32u);
  const uint32_t limit = CU_LDS_LIMIT;
  LaunchCfg c = cu_launch_with(f, p, sx, sy, node_budget, stack_cap);
  if (c.lds_bytes > limit && own_nodes) c = cu_launch_with(f, p, sx, sy, node_budget = 1024u, stack_cap);
  // (a smaller stack may turn the launch into one of the DEEP build, with one more walking wave: a few rounds)
  for (int round = 0; round < 8 && c.lds_bytes > limit && own_stack && c.args.stack_lds > 1u; ++round) {
    const uint32_t per_row = std::max(1u, c.args.cu_walkers) * CU_STACK_ROW_BYTES;
    const uint32_t rows_over = (c.lds_bytes - limit + per_row - 1u) / per_row;
    stack_cap = c.args.stack_lds > rows_over + 1u ? c.args.stack_lds - rows_over - 1u : 1u;
    c = cu_launch_with(f, p, sx, sy, node_budget, stack_cap);
  }
  // (with both options left to the policy the smallest layout - 1 KB of nodes, one stack row per walking wave, eight
  // slots, at most 4 KB of leaves - always fits: that case names no option)
  if (c.lds_bytes > limit)
    c.error = !own_nodes && !own_stack ? "options: lds_budget_kb and lds_stack together are beyond the compute unit's 160 KB of LDS"
              : !own_nodes           ? "options: lds_budget_kb is beyond the compute unit's 160 KB of LDS"
              : !own_stack           ? "options: lds_stack is beyond the compute unit's 160 KB of LDS"
                                     : "the launch does not fit the compute unit's 160 KB of LDS";
  return c;
}

// the scene-owned scratch of a CU launch: one cold region per workgroup, one overflow stack per walking wave
void cu_scratch(const LaunchFacts& f, LaunchCfg& c) {
  const RenderArgs& a = c.args;
  c.cold_bytes = size_t(c.grid) * cu_cold_records(f.textured) * a.pool_slots * 16u;
  if (a.stack_lds < a.stack_entries)
    c.ovf_bytes = size_t(c.grid) * a.cu_walkers * (a.stack_entries - a.stack_lds) * CU_STACK_ROW_BYTES;
}

// The lane launch's shape for `feature` or the lane-bound kernel: arguments and LDS layout (stacks, then the top of the
// tree); the grid is lane_launch's
LaunchCfg lane_shape(const LaunchFacts& f, const VimgRenderParams& p, int sx, int sy, bool feature) {
  LaunchCfg c{};
  c.feature = feature;
  const VimgHipOptions& o = f.opt;
  c.sched = VIMG_SCHED_LANE;
  // register budget: the lane-bound kernel wants 3 waves per SIMD on scenes beyond the on-chip
  // caches (latency-bound) and 2 on small ones (VALU-bound, fewest spills)
  c.wps = f.waves_per_simd;
  if (o.waves_per_simd != VIMG_OPT_AUTO) c.wps = o.waves_per_simd >= 3 ? 3 : 2;
  RenderArgs& a = c.args = base_args(f, p, sx, sy);
  a.stack_lds = a.stack_entries;
  // LDS budget per 256-thread workgroup: stacks first, then as much of the top of the tree as
  // fits in 40 KiB total (keeps >= 4 workgroups per CU inside the 160 KiB)
  const uint32_t stack_bytes = 4u * a.stack_entries * CU_STACK_ROW_BYTES;
  uint32_t budget = 40u * 1024u;
  if (o.lds_budget_kb != VIMG_OPT_AUTO) budget = uint32_t(std::max(1, o.lds_budget_kb)) * 1024u;
  uint32_t nodes = 0;
  if (stack_bytes + 512 < budget) nodes = (budget - stack_bytes - 256) / CU_NODE_BYTES;
  a.lds_nodes = std::min(nodes, f.num_nodes);
  c.lds_bytes = cu_node_plane_bytes(a.lds_nodes) + stack_bytes;
  return c;
}

// ... with its persistent grid: as many 4-wave workgroups as the kernel's registers and LDS let a CU hold (`per_cu`:
// the caller asked the runtime), never more than the work.  (A masked launch's item list is set after this, by
// enqueue_render: its grid is still sized by the shard's items, and a wave without work leaves after one claim.)
LaunchCfg lane_launch(const LaunchFacts& f, const VimgRenderParams& p, int sx, int sy, bool feature, int per_cu) {
  LaunchCfg c = lane_shape(f, p, sx, sy, feature);
  const uint64_t items = (sx >= 0) ? 1 : uint64_t(local_tiles(f, p)) * 64u;
  const uint64_t need_blocks = (items + 255) / 256;
  c.grid = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(need_blocks, uint64_t(f.num_cus) * std::max(per_cu, 1))));
  return c;
}

}  // namespace

LaunchCfg lane_layout(const LaunchFacts& f, const VimgRenderParams& p) { return lane_shape(f, p, -1, -1, false); }

LaunchCfg plan_launch(const LaunchFacts& f, const VimgRenderParams& p, int sx, int sy, int lane_per_cu) {
  if (is_feature_integrator(p.integrator)) return lane_launch(f, p, sx, sy, true, lane_per_cu);
  // (the upload admits the schedulers AUTO, LANE and CU only)
  if (f.too_wide || f.opt.scheduler == VIMG_SCHED_LANE) return lane_launch(f, p, sx, sy, false, lane_per_cu);   // slots pack pixel coordinates in 16 bits
  LaunchCfg c = make_launch_cu(f, p, sx, sy);
  if (c.error) return c;
  cu_scratch(f, c);
  return c;
}

// The one place that decides between a PLAIN build and the general one: the launch as its arguments stand
// (enqueue_render asks after it has set the item list and the statistics flag) against plain_build.h's list.
// plain_fold_of: which of them - PLAIN_FOLD, or PLAIN_FOLD_OTHER where the resident scene holds a material of class 3
// (VimgDeviceScene::has_other: set at upload, again by every material edit); 0 = the general build.  The two folds
// differ in PF_NO_OTHER only, so tables and leaf copies serve both alike.
uint32_t plain_fold_of(const LaunchFacts& f, const LaunchCfg& c, bool stats) {
  if (!plain_tables_serve(c.args.lds_tables) || !plain_leaf_perm_serves(c.args.leaf_perm)) return 0u;
  return plain_fold_serving(plain_launch_of(c.sched == VIMG_SCHED_CU, f.textured, c.deep, int(CU_WAVES), stats, f.force_general, c.args,
                                            f.has_other));
}

// A launch whose arguments, now complete, send it to the general or the statistics build reads no table from LDS:
// and no permuted leaf copy: their room goes back (they are the last things in the layout) and RenderArgs::lds_tables
// and ::leaf_perm say what is staged
void drop_unread_tables(const LaunchFacts& f, LaunchCfg& c, bool stats) {
  if (c.sched != VIMG_SCHED_CU || (c.args.lds_tables == 0u && c.args.leaf_perm == 0u) || plain_fold_of(f, c, stats) != 0u) return;
  c.lds_bytes -= c.table_bytes;
  c.table_bytes = 0u;
  c.args.lds_tables = 0u;
  c.args.leaf_perm = 0u, c.args.leaf_perm_off = 0u, c.args.leaf_perm_stride = 0u;
}

const char* launch_kernel_name(const LaunchFacts& f, const VimgRenderParams& p) {
  static const char* lane_names[2][2] = {{"render_kernel<false,2>", "render_kernel<false,3>"},
                                         {"render_kernel<true,2>", "render_kernel<true,3>"}};
  static const char* cu_names[2][2] = {{"render_cu_kernel<false>", "render_cu_kernel<false,deep>"},
                                       {"render_cu_kernel<true>", "render_cu_kernel<true,deep>"}};
  if (p.tile_world == 0 || p.tile_rank >= p.tile_world) return "";
  if (is_feature_integrator(p.integrator)) return f.textured ? "feature_kernel<true>" : "feature_kernel<false>";
  const LaunchCfg c = plan_launch(f, p, -1, -1, 1);   // (the name does not depend on the grid)
  if (c.error) return "";
  // The build whole frames are timed on keeps the name it has always had: that is a PLAIN build now (plain_build.h).
  // Where the general build of the same scene class runs instead - another integrator, other options, the override
  // VIMG_HIP_PLAIN=0 - the name says so.  (Builds for textures or trees in global memory have no PLAIN counterpart.)
  if (c.sched == VIMG_SCHED_CU && !f.textured && !c.deep && plain_fold_of(f, c, false) == 0u) return "render_cu_kernel<false,general>";
  if (c.sched == VIMG_SCHED_CU) return cu_names[f.textured ? 1 : 0][c.deep ? 1 : 0];
  return lane_names[f.textured ? 1 : 0][c.wps >= 3 ? 1 : 0];
}

}  // namespace vimg
