// The host side of the schedulers no launch policy picks - POOL (round 1's pooled kernel), POOL4 / POOL4G
// (round 2's) and STAGE (global queues): their launch configuration, their scene-owned buffers, their
// argument blocks and launches.  Like their kernels (k_dev.hip, k_pool4.hip) this is real in the
// development build only (make dev, -DVIMG_DEV_SCHEDULERS); the product gets stubs that answer what the
// upload says of these schedulers.
#include "hip_internal.h"
#ifdef VIMG_DEV_SCHEDULERS
#include "render_pool_kernel.h"
#include "render_stage_kernel.h"
#include "render_pool4_kernel.h"

// staged kernel: control block, queue rings, ready-pixel ring, per-pixel records, slot records; and the
// argument block (StageKArgs / Pool4KArgs) of the launch in flight
struct DevSchedState {
  void* ctl = nullptr;
  void* kargs = nullptr;
  void* rings = nullptr;
  size_t rings_bytes = 0;
  void* pix_ring = nullptr;
  size_t pix_ring_bytes = 0;
  void* pix_state = nullptr;
  size_t pix_state_bytes = 0;
  void* slots = nullptr;
  size_t slots_bytes = 0;
};

namespace vimg {
namespace {

uint32_t ceil_pow2(uint64_t v) {
  uint32_t p = 1;
  while (p < v) p <<= 1;
  return p;
}
uint32_t log2_of(uint32_t pow2) {
  uint32_t k = 0;
  while ((1u << k) < pow2) ++k;
  return k;
}

uint32_t stage_wchunk(const VimgHipOptions& o) { return std::min(STAGE_WCHUNK_MAX, std::max(128u, opt_or(o.stage_wchunk, 128u))); }

// the staged kernel's queue parameters and buffer sizes for a configured launch (pointers: ensure_stage)
StageArgs stage_args(const VimgDeviceScene* s, const LaunchCfg& c) {
  const VimgHipOptions& o = s->opt;
  const uint64_t items = (c.args.single_x >= 0) ? 1 : uint64_t(c.args.num_local_tiles) * 64u;
  StageArgs g{};
  g.wchunk = stage_wchunk(o);
  g.walk_quota = std::max(g.wchunk, opt_or(o.stage_walk_quota, 2048u));
  g.seg_len = std::max(1u, opt_or(o.stage_seg_len, 4u));
  // slots in flight: twice the resident lanes (every stage then finds full batches queued while
  // as many paths are being worked on), never more than the pixels of the launch, which are the
  // unit of parallelism (one sequential RNG stream per pixel, include/integrators.h:116-127)
  const uint64_t lanes = uint64_t(c.grid) * 256u;
  uint64_t n = opt_or(o.stage_slots, static_cast<uint32_t>(std::min<uint64_t>(lanes * 2u, STAGE_MAX_SLOTS)));
  n = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(n, items), STAGE_MAX_SLOTS));
  g.n_slots = static_cast<uint32_t>(n);
  g.ring_cap = std::max(64u, ceil_pow2(n));
  g.ring_shift = log2_of(g.ring_cap);
  g.pix_cap = std::max(64u, ceil_pow2(items));
  g.pix_shift = log2_of(g.pix_cap);
  g.rings_bytes = GQ_COUNT * GQ_SHARDS * g.ring_cap * 4u;
  g.pix_ring_bytes = g.pix_cap * 4u;
  g.pix_state_bytes = static_cast<uint32_t>(items * 32u);
  g.slots_bytes = g.n_slots * GR_BYTES;
  return g;
}

// (AUTO is the CU scheduler's since round 3, so this is reached by name only and `by_policy` is false:
// the policy branches below record what round 2 measured)
LaunchCfg make_launch_dev(const VimgDeviceScene* s, const VimgRenderParams* p, int sx, int sy, bool lds_stack_all) {
  LaunchCfg c{};
  const VimgHipOptions& o = s->opt;
  const uint64_t items = (sx >= 0) ? 1 : uint64_t(local_tiles(s, p)) * 64u;
  int sched = o.scheduler;
  const bool by_policy = (sched == VIMG_OPT_AUTO);
  c.group = (sched == VIMG_SCHED_POOL4G);
  if (c.group) sched = VIMG_SCHED_POOL4;   // the same launch in everything but the pool's layout and the kernel build
  if (sched == VIMG_SCHED_STAGE && items > (1ull << 26)) sched = VIMG_SCHED_POOL4;   // 32-bit byte offsets of the pixel records
  c.sched = sched;
  c.pooled = (sched == VIMG_SCHED_POOL || sched == VIMG_SCHED_POOL4);
  // register budget: the lane-bound kernel wants 3 waves per SIMD on scenes beyond the on-chip
  // caches (latency-bound) and 2 on small ones (VALU-bound, fewest spills); the pooled kernel
  // hides latency with its slots and always takes the 256-register build (config 4/5: 2 waves
  // 1.02 / 1.70 Grays/s, 3 waves 0.66 / 0.91); the staged kernel has one build (128 registers)
  c.wps = 2;
  if (o.waves_per_simd != VIMG_OPT_AUTO) c.wps = o.waves_per_simd >= 3 ? 3 : 2;
  if (sched == VIMG_SCHED_STAGE) c.wps = 4;
  // pool4: three waves per SIMD by policy (config 2: 12.2 Grays/s at three, 11.3 at four; the stand-ins
  // of configs 3 / 4 / 5: 6.6 / 1.56 / 2.62 against 6.1 / 1.15 / 1.52 - a wave's LDS share, i.e. its
  // pool, shrinks faster than the fourth wave pays, most of all under the deep trees' stacks)
  if (sched == VIMG_SCHED_POOL4) c.wps = (o.waves_per_simd == 4) ? 4 : 3;
  c.rays = 1;
  RenderArgs& a = c.args = base_args(s, p, sx, sy);
  a.stack_lds = a.stack_entries;
  // pool4 on trees that do not fit in LDS: the first `lds_stack` (AUTO 32) entries of a lane's stack in LDS, the rest in
  // global memory (the LDS goes to path slots instead); `lds_stack_all`: second pass, when the tree
  // turned out to fit (the build without the overflow path)
  if (sched == VIMG_SCHED_POOL4 && !lds_stack_all)
    a.stack_lds = std::min(a.stack_entries, std::max(1u, opt_or(o.lds_stack, 32u)));
  const uint32_t stack_rows = (sched == VIMG_SCHED_POOL4) ? pool4_stack_rows_of(a.stack_entries, a.stack_lds) : a.stack_entries;
  // LDS budget per 256-thread workgroup: stacks first, then as much of the top of the tree as
  // fits in 40 KiB total (keeps >= 4 workgroups per CU inside the 160 KiB)
  const uint32_t stack_bytes = 4u * stack_rows * 64u * 4u * uint32_t(c.rays);
  // (the pooled and staged kernels spend LDS on path slots / queue chunks instead: they keep the
  // first six levels of the tree, 4 KiB - config 5: 40 KiB budget 1.69, 28 KiB 1.78 Grays/s)
  uint32_t budget = std::min(40u * 1024u, stack_bytes + 4608u);
  if (o.lds_budget_kb != VIMG_OPT_AUTO) budget = uint32_t(std::max(1, o.lds_budget_kb)) * 1024u;
  uint32_t nodes = 0;
  if (stack_bytes + 512 < budget) nodes = (budget - stack_bytes - 256) / 56u;
  a.lds_nodes = std::min(nodes, s->d.num_nodes);
  c.lds_bytes = ((a.lds_nodes * 56u + 255u) & ~255u) + stack_bytes;
  // (pool_boxmin, 16 lanes in base_args:)
  // config 4 / 5 stand-ins: never 1.02 / 1.74, 8 lanes 1.19 / 2.10, 16: 1.18 / 2.13, 24: 1.20 / 2.13,
  // 40: 1.15 / 1.93 Grays/s
  a.pool_gbreak = std::min(64u, opt_or(o.pool_gbreak, 32u));

  c.deep = a.lds_nodes < s->d.num_nodes;   // the other build reads every node from LDS
  if (!c.deep && a.stack_lds < a.stack_entries) return make_launch_dev(s, p, sx, sy, true);
  // Vertex queues and the starvation threshold.  Trees in LDS (pools of 150-190 slots): one queue per
  // material class, a partial batch when 24 walk lanes idle.  Trees in global memory leave a pool of
  // about 100 slots, which three class queues drain to 21-27 slots per batch and 20 rays per walk
  // pass: there ONE queue of shading vertices (next to the finishers') and 32 idle lanes measure best
  // (stand-ins of configs 4 / 5, 32 spp: 1.60 -> 1.72, 2.68 -> 2.81 Grays/s;
  // profiles/r2_pool4/deep_policy_sweeps.txt)
  a.pool_classes = std::min(3u, std::max(1u, opt_or(o.pool_classes, c.deep ? 1u : 3u)));
  a.pool_starve = std::min(64u, std::max(1u, opt_or(o.pool_starve, c.deep ? 32u : 24u)));
  // small scenes: all leaf records in LDS too (they cost a few slots, the walk gains more)
  uint32_t leaf_bytes = 0;
  a.lds_leaf = 0;
  if (s->num_leaf_prims * 48u <= 4096u && o.lds_leaf != 0) {
    a.lds_leaf = s->num_leaf_prims;
    leaf_bytes = a.lds_leaf * 48u;
  }
  if (c.pooled) {
    // Pixels are the unit of parallelism (one sequential RNG stream per pixel): a launch with few
    // pixels per wave is fastest with pools of about pixels / 2.4 slots, and with very few the
    // lane-bound kernel wins - the pooled scheduler's hop latency times the longest pixel's chain of
    // path vertices is then the whole frame time.  By policy only; what is asked for by name stands.
    const bool policy_pool4 = sched == VIMG_SCHED_POOL4 && by_policy && o.pool_slots == VIMG_OPT_AUTO;
    uint64_t want = ~0ull;
    if (policy_pool4) {
      if (sx >= 0) return make_launch_lane(s, p, sx, sy);   // trace_pixel: one path
      const uint64_t waves = uint64_t(s->num_cus) * 3u * 4u;   // three workgroups per CU (checked against the runtime below)
      want = items * 10u / (waves * 24u);
      // (trees in global memory never go there: the lane-bound kernel pays a memory round trip per
      // phase of its machine - quarter / eighth of the config-4 stand-in, 128 spp: 261 / 243 ms against
      // 134 / 112 ms with group pools of 32 slots per wave)
      if (want < 40u && !c.deep) return make_launch_lane(s, p, sx, sy);
      // A full frame on a tree in LDS: FOUR waves per SIMD with group pools (config 2, 512 spp: 13.4
      // against 12.7 Grays/s with three waves and per-wave pools - the fourth wave's issue slots pay
      // now that its smaller LDS share no longer thins the batches; config 3: 7.63 against 7.47).
      // Shards keep three (half of config 2: 209 against 226 ms), and so do trees in global memory
      // (their stacks leave a four-wave workgroup no LDS for slots: 1.34 against 2.09 Grays/s).
      if (!c.deep && o.waves_per_simd == VIMG_OPT_AUTO && want >= 160u) {
        c.wps = 4;
        want = want * 3u / 4u;   // per wave of the larger grid
      }
    }
    // the pool takes what is left of this workgroup's share of the CU's 160 KiB
    const uint32_t share = (160u * 1024u) / uint32_t(c.wps) - 1024u;
    if (sched == VIMG_SCHED_POOL4) c.lds_bytes += 4u * uint32_t(sizeof(Pool4Wave) + sizeof(Pool4Diag));
    auto slots_for = [&](uint32_t slot_bytes, uint32_t extra) {
      const uint32_t used = c.lds_bytes + extra + leaf_bytes + 64u;
      return std::min(share > used ? (share - used) / (slot_bytes * 4u) : 0u, 256u);
    };
    uint32_t slots = slots_for((sched == VIMG_SCHED_POOL4) ? P4_LDS_BYTES : POOL_LDS_BYTES, 0);
    // Which pool4 build (by policy).  One pool per WAVE only when three waves per SIMD are asked for
    // on a full frame of a tree in LDS (config 2 12.3 against 11.9 Grays/s - there the group's lock
    // costs more than its fuller batches earn).  One pool per WORKGROUP otherwise: at four waves per
    // SIMD (above), and wherever pools are small - trees in global memory, whose
    // stacks take half the LDS (stand-ins of configs 4 / 5, 32 spp: 1.72 -> 2.07, 2.81 -> 3.22
    // Grays/s), and frames with few pixels per wave (half of config 2: 238 -> 209 ms; a quarter:
    // lane-bound 205 -> 180 ms with 64 slots; an eighth stays with the lane-bound kernel, 139 ms).
    if (policy_pool4) c.group = c.wps == 4 || c.deep || want < slots;
    if (c.group) {
      c.lds_bytes += pool4g_group_bytes(0);   // group record, batch rows
      slots = slots_for(P4G_LDS_BYTES, 0);
    }
    const uint32_t slot_bytes = c.group ? P4G_LDS_BYTES : (sched == VIMG_SCHED_POOL4) ? P4_LDS_BYTES : POOL_LDS_BYTES;
    if (o.pool_slots != VIMG_OPT_AUTO) slots = std::min(slots, uint32_t(std::max(0, o.pool_slots)));
    a.pool_slots = std::max(slots, 8u);
    if (sched == VIMG_SCHED_POOL4) {
      if (policy_pool4)
        a.pool_slots = static_cast<uint32_t>(std::min<uint64_t>(a.pool_slots, std::max<uint64_t>(want, c.deep ? 32u : 64u)));
      a.pool_slots &= ~1u;   // even: every wave's cold region starts on a 64-byte line (and a group's tables on 16 bytes)
    }
    c.lds_bytes += (c.group ? slot_bytes * 4u * a.pool_slots : 4u * ((slot_bytes * a.pool_slots + 15u) & ~15u)) + leaf_bytes;
    // vertex queues and thresholds of the group build: one queue per material class again (the
    // group's queues fill), 32 idle lanes before a partial batch, a full batch taken by a wave with
    // at most 32 rays in its lanes
    if (c.group) {
      a.pool_classes = std::min(3u, std::max(1u, opt_or(o.pool_classes, 3u)));
      a.pool_gbreak = std::min(64u, opt_or(o.pool_gbreak, 32u));
    }
  }
  if (sched == VIMG_SCHED_STAGE) c.lds_bytes += 4u * (5u * stage_wchunk(o) * 4u + 256u) + leaf_bytes;
  // persistent grid: as many 4-wave workgroups as the kernel's registers and LDS let a CU hold
  // (asked of the runtime), never more than the work
  int per_cu = 0;
  hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel_of(s, c), 256, c.lds_bytes);
  if (oe != hipSuccess || per_cu < 1) per_cu = 1;
  const uint64_t need_blocks = (items + 255) / 256;
  c.grid = static_cast<uint32_t>(
      std::max<uint64_t>(1, std::min<uint64_t>(need_blocks, uint64_t(s->num_cus) * per_cu)));
  // pooled kernel: split every pixel's samples into segments handed out as separate work items
  // when the image is large against the slots in flight (then the previous segment of a pixel
  // has long been published when its next one is drawn); small images keep one segment
  if (a.pool_slots && sx < 0) {
    const uint64_t in_flight = uint64_t(c.grid) * 4u * a.pool_slots;
    // Segments: the tail of a frame is one segment long, and every hand-over costs a little
    // (config 2, 3.5 pool generations per frame: 1 segment 6.8, 4: 7.5, 8: 7.6, 16-32: 7.6 Grays/s;
    // 3600x1600, 14 generations: 1 segment 7.9, 4: 7.7) - about 56 segments per generation count,
    // at most 16, of at least 4 samples; frames of 10 generations and more keep their pixels whole
    // (group pools at four waves, config 2 at 512 spp, 2.75 generations: 8 segments 322.5 ms, 16: 315.3,
    // 32: 312.9, 64: 311.4 - the pooled kernels before it were flat from 16 on)
    const bool more = c.group && c.wps == 4;
    segments_for(s, p, items, in_flight, more ? 176.0 : 56.0, more ? 64.0 : 16.0, &a);
  }
  // scene-owned scratch: one cold region and one overflow stack per resident wave
  if (c.pooled) {
    const size_t ncold = (sched == VIMG_SCHED_POOL4) ? pool4_cold_records(s->textured) : (s->textured ? SC_COUNT : SC_COUNT - 1u);
    c.cold_bytes = size_t(c.grid) * 4u * ncold * a.pool_slots * 16u;
    if (a.stack_lds < a.stack_entries)
      c.ovf_bytes = size_t(c.grid) * 4u * uint32_t(c.rays) * (a.stack_entries - a.stack_lds) * 256u;
  }
  return c;
}

// The staged kernel keeps all path state in global memory, owned by the scene and grown on demand:
// control block, queue rings, ready-pixel ring, per-pixel records, slot records (config 2 on 256
// CUs: 0.01 + 42 + 8 + 46 + 50 MB).  Counters, rings and the ready-pixel ring are cleared per launch.
int ensure_stage(DevSchedState* v, const LaunchCfg& c, StageArgs& g, hipStream_t st) {
  if (!v->ctl) HIP_TRY(hipMalloc(&v->ctl, sizeof(StageCtl)));
  if (int rc = grow(&v->rings, &v->rings_bytes, g.rings_bytes)) return rc;
  if (int rc = grow(&v->pix_ring, &v->pix_ring_bytes, g.pix_ring_bytes)) return rc;
  if (int rc = grow(&v->pix_state, &v->pix_state_bytes, g.pix_state_bytes)) return rc;
  if (int rc = grow(&v->slots, &v->slots_bytes, g.slots_bytes)) return rc;
  g.ctl = (VIMG_GLOBAL StageCtl*)v->ctl;
  g.rings = (VIMG_GLOBAL uint32_t*)v->rings;
  g.pix_ring = (VIMG_GLOBAL uint32_t*)v->pix_ring;
  g.pix_state = (VIMG_GLOBAL v4u*)v->pix_state;
  g.slots = (VIMG_GLOBAL v4u*)v->slots;
  HIP_TRY(hipMemsetAsync(v->ctl, 0, sizeof(StageCtl), st));
  HIP_TRY(hipMemsetAsync(v->rings, 0, g.rings_bytes, st));
  HIP_TRY(hipMemsetAsync(v->pix_ring, 0, g.pix_ring_bytes, st));
  // pixels nobody has started: all of them but one per slot (the slots start "fresh")
  const uint64_t items = (c.args.single_x >= 0) ? 1 : uint64_t(c.args.num_local_tiles) * 64u;
  const uint32_t surplus = static_cast<uint32_t>(items - g.n_slots);
  StageCtl* ctl = static_cast<StageCtl*>(v->ctl);
  HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&ctl->surplus.v), static_cast<int>(surplus), 1, st));
  return VIMG_OK;
}

}  // namespace

LaunchCfg dev_make_launch(const VimgDeviceScene* s, const VimgRenderParams* p, int sx, int sy) {
  return make_launch_dev(s, p, sx, sy, false);
}

const void* dev_kernel_of(const VimgDeviceScene* s, const LaunchCfg& c, const char** name) {
  static const char* pool_names[2][2][2] = {
      {{"render_pool_kernel<false,2>", "render_pool_kernel<false,3>"}, {"render_pool_kernel<true,2>", "render_pool_kernel<true,3>"}},
      {{"render_pool_kernel<false,2,deep>", "render_pool_kernel<false,3,deep>"},
       {"render_pool_kernel<true,2,deep>", "render_pool_kernel<true,3,deep>"}}};
  static const char* stage_names[2][2] = {{"render_stage_kernel<false>", "render_stage_kernel<false,deep>"},
                                          {"render_stage_kernel<true>", "render_stage_kernel<true,deep>"}};
  static const char* pool4_names[2][2] = {{"render_pool4_kernel<false>", "render_pool4_kernel<false,deep>"},
                                          {"render_pool4_kernel<true>", "render_pool4_kernel<true,deep>"}};   // (+ waves per SIMD, rays per lane)
  static const char* pool4g_names[2][2] = {{"render_pool4_kernel<false,group>", "render_pool4_kernel<false,deep,group>"},
                                           {"render_pool4_kernel<true,group>", "render_pool4_kernel<true,deep,group>"}};
  const int t = s->textured ? 1 : 0, dp = c.deep ? 1 : 0;
  if (c.sched == VIMG_SCHED_STAGE) {
    if (name) *name = stage_names[t][dp];
    return reinterpret_cast<const void*>(vimg_stage_kernel(s->textured, c.deep));
  }
  if (c.sched == VIMG_SCHED_POOL4) {
    if (name) *name = (c.group ? pool4g_names : pool4_names)[t][dp];
    return reinterpret_cast<const void*>(vimg_pool4_kernel(s->textured, c.deep, c.wps, c.group));
  }
  if (name) *name = pool_names[dp][t][c.wps >= 3 ? 1 : 0];
  return reinterpret_cast<const void*>(vimg_pool_kernel(s->textured, c.wps, c.deep));
}

int dev_enqueue(VimgDeviceScene* s, const LaunchCfg& c, float* d_out, DeviceStats* stats, hipStream_t st, hipEvent_t ev0) {
  if (c.sched == VIMG_SCHED_POOL) {
    if (ev0) HIP_TRY(hipEventRecord(ev0, st));
    hipLaunchKernelGGL(vimg_pool_kernel(s->textured, c.wps, c.deep), dim3(c.grid), dim3(256), c.lds_bytes, st, s->d, c.args,
                       d_out, stats, s->d_counter);
    return VIMG_OK;
  }
  if (!s->dev) s->dev = new DevSchedState();
  DevSchedState* v = s->dev;
  StageArgs g = stage_args(s, c);
  if (c.sched == VIMG_SCHED_STAGE)
    if (int rc = ensure_stage(v, c, g, st)) return rc;
  if (!v->kargs) HIP_TRY(hipMalloc(&v->kargs, std::max(sizeof(StageKArgs), sizeof(Pool4KArgs))));
  if (c.sched == VIMG_SCHED_STAGE) {
    // scene + launch parameters go to the block the stage functions read (stream-ordered, by value)
    StageKArgs* blk = static_cast<StageKArgs*>(v->kargs);
    hipLaunchKernelGGL(stage_args_kernel, dim3(1), dim3(64), 0, st, StageKArgs{s->d, c.args, g, d_out, stats}, blk);
    if (ev0) HIP_TRY(hipEventRecord(ev0, st));
    hipLaunchKernelGGL(vimg_stage_kernel(s->textured, c.deep), dim3(c.grid), dim3(256), c.lds_bytes, st,
                       static_cast<const StageKArgs*>(blk));
  } else {
    Pool4KArgs* blk = static_cast<Pool4KArgs*>(v->kargs);
    hipLaunchKernelGGL(pool4_args_kernel, dim3(1), dim3(64), 0, st, Pool4KArgs{s->d, c.args, d_out, stats, s->d_counter}, blk);
    if (ev0) HIP_TRY(hipEventRecord(ev0, st));
    hipLaunchKernelGGL(vimg_pool4_kernel(s->textured, c.deep, c.wps, c.group), dim3(c.grid), dim3(256), c.lds_bytes, st,
                       static_cast<const Pool4KArgs*>(blk));
  }
  return VIMG_OK;
}

int dev_error_word(const VimgDeviceScene* s, unsigned int* word) {
  *word = 0;
  if (s->dev && s->dev->ctl)
    HIP_TRY(hipMemcpy(word, &static_cast<StageCtl*>(s->dev->ctl)->error.v, sizeof(*word), hipMemcpyDeviceToHost));
  return VIMG_OK;
}

void dev_free(VimgDeviceScene* s) {
  if (!s->dev) return;
  for (void* q : {s->dev->ctl, s->dev->kargs, s->dev->rings, s->dev->pix_ring, s->dev->pix_state, s->dev->slots})
    if (q) (void)hipFree(q);
  delete s->dev;
  s->dev = nullptr;
}

}  // namespace vimg
#else
namespace vimg {
LaunchCfg dev_make_launch(const VimgDeviceScene*, const VimgRenderParams*, int, int) { return LaunchCfg{}; }
const void* dev_kernel_of(const VimgDeviceScene*, const LaunchCfg&, const char**) { return nullptr; }
int dev_enqueue(VimgDeviceScene*, const LaunchCfg&, float*, DeviceStats*, hipStream_t, hipEvent_t) {
  return fail(VIMG_E_UNSUPPORTED, kNoDevSchedulers);
}
int dev_error_word(const VimgDeviceScene*, unsigned int* word) {
  *word = 0;
  return VIMG_OK;
}
void dev_free(VimgDeviceScene*) {}
}  // namespace vimg
#endif
