// libvimg_hip.so - C ABI (include/vimg_hip.h) over the gfx950 kernels in render_kernels.h.  This unit holds
// the render entry points and the one path every render takes (enqueue_render); the scene's upload, the
// launch policy, the ray queries and the pre / post steps have units of their own (hip_internal.h).  There is
// no CPU render path in this library.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "hip_internal.h"
#include "aux_kernels.h"
#include "render_cu_kernel.h"
#include "heatmap_kernel.h"

namespace vimg {

hipStream_t g_stream = nullptr;
int g_device = -1;

namespace {
thread_local std::string g_err;
}

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

}  // namespace vimg

using namespace vimg;

namespace vimg {

int check_params(const VimgDeviceScene* s, const VimgRenderParams* p) {
  if (!s || !p) return fail(VIMG_E_INVALID, "null scene or params");
  if (p->tile_world == 0 || p->tile_rank >= p->tile_world)
    return fail(VIMG_E_INVALID, "tile_rank must be < tile_world");
  if (p->samples == 0) return fail(VIMG_E_INVALID, "samples must be > 0");
  if (p->integrator == VIMG_INTEGRATOR_MATERIAL && p->depth == 0)
    return fail(VIMG_E_INVALID, "material integrator with depth 0 renders nothing");
  if (p->integrator > VIMG_INTEGRATOR_COVERAGE) return fail(VIMG_E_INVALID, "unknown integrator");
  if (p->integrator == VIMG_INTEGRATOR_MIS && s->d.num_lights == 0)
    return fail(VIMG_E_INVALID, "mis integrator needs at least one light (the reference's "
                                "GroupOfEmitters::sample is undefined without one)");
  return VIMG_OK;
}

int check_render(const VimgDeviceScene* s, const VimgRenderParams* p, const void* d_out) {
  if (int rc = check_params(s, p)) return rc;
  if (!d_out) return fail(VIMG_E_INVALID, "null output pointer");
  return VIMG_OK;
}

}  // namespace vimg

namespace {

// The CU scheduler keeps the cold records of its path slots in global memory, and deep trees the stack
// entries beyond the LDS part: one region per workgroup (per walking wave), owned by the scene and grown on
// demand (42 MB for config 2 on 256 CUs); and a per-pixel record between sample segments.
int ensure_pool(VimgDeviceScene* s, LaunchCfg& c) {
  c.args.pool_cold = nullptr;
  if (!c.cold_bytes) return VIMG_OK;
  if (int rc = s->pool_cold.grow(c.cold_bytes)) return rc;
  c.args.pool_cold = (VIMG_GLOBAL v4u*)s->pool_cold.p;
  if (c.ovf_bytes) {
    if (int rc = s->stack_ovf.grow(c.ovf_bytes)) return rc;
    c.args.stack_ovf = (VIMG_GLOBAL uint32_t*)s->stack_ovf.p;
  }
  c.args.pool_state = nullptr;
  c.args.pool_epoch = 0;
  if (c.args.pool_segments > 1) {
    const size_t had = s->pool_state.bytes;
    if (int rc = s->pool_state.grow(size_t(c.args.num_local_tiles) * 64u * 32u)) return rc;
    if (s->pool_state.bytes != had) s->pool_epoch = 0xffff0000u;   // a new buffer starts like a wrapped epoch: wiped
    // tags are epoch + segment index (< 4096): one epoch step per launch, wrap with a wipe
    s->pool_epoch += 4096u;
    if (s->pool_epoch >= 0xffff0000u) {
      HIP_TRY(hipMemset(s->pool_state.p, 0, s->pool_state.bytes));
      s->pool_epoch = 4096u;
    }
    c.args.pool_state = (VIMG_GLOBAL v4u*)s->pool_state.p;
    c.args.pool_epoch = s->pool_epoch;
  }
  return VIMG_OK;
}

}  // namespace

namespace vimg {

int enqueue_render(VimgDeviceScene* s, const VimgRenderParams* p, const RenderLaunch& r) {
  const ProgLaunch* prog = r.prog;
  const hipStream_t st = r.st;
  float* d_out = r.d_out;
  LaunchCfg c = make_launch(s, p, r.sx, r.sy);
  if (c.error) return fail(VIMG_E_INVALID, c.error);   // (options no launch can be made of: nothing has been enqueued)
  if (prog) {
    c.args.sample_base = prog->base;
    c.args.spp_div = static_cast<float>(prog->base + p->samples);   // (the caller keeps the total <= UINT32_MAX)
    c.args.prog_in = (const VIMG_GLOBAL v4u*)prog->in;
    c.args.prog_out = (VIMG_GLOBAL v4u*)prog->out;
    c.args.item_list = (const VIMG_GLOBAL uint32_t*)prog->item_list;
    c.args.item_count = prog->item_count;
  }
  if (int rc = ensure_pool(s, c)) return rc;
  c.args.full_stats = r.stats ? 1u : 0u;
  drop_unread_tables(facts_of(s), c, r.stats);
  if (c.args.num_local_tiles == 0 && r.sx < 0) return VIMG_OK;
  // (the work counter only: the error word behind it is sticky until a blocking call or vimg_hip_check reads it)
  HIP_TRY(hipMemsetAsync(s->counter.p, 0, sizeof(unsigned int), st));
  if (r.stats && !(prog && prog->keep_stats)) HIP_TRY(hipMemsetAsync(s->stats.p, 0, sizeof(DeviceStats), st));
  DeviceStats* stats = r.stats ? s->stats.as<DeviceStats>() : nullptr;
  const void* kernel = launched_kernel_of(s, c, r.stats);
  if (c.lds_bytes > 48u * 1024u)   // ask for the large dynamic-LDS carve-out
    HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(c.lds_bytes)));
  if (r.ev0) HIP_TRY(hipEventRecord(r.ev0, st));
  if (c.sched == VIMG_SCHED_CU) {
    CuKArgs ka{s->d, c.args, d_out, stats, s->counter.as<unsigned int>()};
    void* kargs[] = {&ka};
    HIP_TRY(hipLaunchKernel(kernel, dim3(c.grid), dim3(CU_WAVES * 64u), kargs, c.lds_bytes, st));
  } else {
    void* kargs[] = {&s->d, &c.args, &d_out, &stats, &s->counter.p};
    HIP_TRY(hipLaunchKernel(kernel, dim3(c.grid), dim3(256), kargs, c.lds_bytes, st));
  }
  if (r.ev1) HIP_TRY(hipEventRecord(r.ev1, st));
  HIP_TRY(hipGetLastError());
  return VIMG_OK;
}

// d_counter[1] is the error word of the last launch (raised by render_cu_kernel's watchdog)
int check_kernel_error(VimgDeviceScene* s) {
  unsigned int words[2] = {0, 0};
  HIP_TRY(hipMemcpy(words, s->counter.p, sizeof(words), hipMemcpyDeviceToHost));
  if (words[1] != 0) HIP_TRY(hipMemset(s->counter.as<unsigned int>() + 1, 0, sizeof(unsigned int)));   // read once
  if (words[1] != 0) {
    // bits of the launch's error word (render_cu_kernel.h: raise): 1 a wave found nothing to do for ten seconds
    // while slots were live, 4 a ring entry was reserved and never written, 8 a compute unit queued more than 2^31 rays or slots in one launch
    const std::string what = (words[1] & 8u) ? "a compute unit queued more than 2^31 rays in one launch: render fewer samples per launch "
                                               "(vimg_hip_progressive_render adds a frame's samples in increments)"
                                             : "a wave waited for work that never came";
    return fail(VIMG_E_DEVICE, "render kernel watchdog: " + what + " (the frame is incomplete), code " +
                                   std::to_string(words[1]));
  }
  return VIMG_OK;
}

// pixels owned by this shard (ragged edge tiles counted exactly)
uint64_t fetch_shard_pixels(const VimgDeviceScene* s, const VimgRenderParams* p) {
  const uint32_t W = s->d.res_x, H = s->d.res_y, ty_n = tiles_of(H), total = tiles_of(W) * ty_n;
  uint64_t px = 0;
  for (uint32_t t = p->tile_rank; t < total; t += p->tile_world) {
    uint32_t tx = t / ty_n, ty = t % ty_n;
    px += uint64_t(std::min(8u, W - tx * 8)) * std::min(8u, H - ty * 8);
  }
  return px;
}

int fetch_stats(VimgDeviceScene* s, const VimgRenderParams* p, VimgRenderStats* out) {
  DeviceStats ds{};
  HIP_TRY(hipMemcpy(&ds, s->stats.p, sizeof(ds), hipMemcpyDeviceToHost));
  *out = VimgRenderStats{};
  out->closest_rays = ds.closest;
  out->shadow_rays = ds.shadow;
  out->internal_visits = ds.internal;
  out->leaf_visits = ds.leaf;
  out->prim_tests = ds.prim;
  out->sphere_tests = ds.sphere;
  out->nan_samples = ds.nan_samples;
  out->paths = fetch_shard_pixels(s, p) * p->samples;
  if (getenv("VIMG_HIP_DIAG"))
    std::fprintf(stderr, "[vimg diag] wave trips: descend %llu (lane visits %llu, util %.3f)  prim %llu (lane tests %llu, util %.3f)  main-loop iterations %llu\n",
                 ds.trip_descend, ds.internal, ds.trip_descend ? double(ds.internal) / (64.0 * ds.trip_descend) : 0.0,
                 ds.trip_prim, ds.prim, ds.trip_prim ? double(ds.prim) / (64.0 * ds.trip_prim) : 0.0, ds.iterations);
  if (getenv("VIMG_HIP_DIAG") && ds.prof[6 + 4]) {   // statistics build of render_cu_kernel: cycles and batch fill per stage
    static const char* st_names[6] = {"finisher", "lambertian", "principled", "other", "walk", "looking for work"};
    unsigned long long total = 0;
    for (int k = 0; k < 6; ++k) total += ds.prof[k];
    for (int k = 0; k < 6; ++k)
      std::fprintf(stderr, "[vimg stage] %-18s %14llu cyc %6.2f %%  batches %10llu  slots/batch %7.2f\n", st_names[k],
                   ds.prof[k], 100.0 * double(ds.prof[k]) / double(total ? total : 1), k < 5 ? ds.prof[6 + k] : 0ull,
                   (k < 4 && ds.prof[6 + k]) ? double(ds.prof[11 + k]) / double(ds.prof[6 + k]) : 0.0);   // (prof[15] is no slot count)
    // the rays a late build of the kernel does not queue (cu_vertex, ELIDE); this build walked and counted them
    std::fprintf(stderr, "[vimg walk] would-elide shadow rays %llu of %llu (%.2f %%): their light sample adds exactly zero\n",
                 ds.prof[15], ds.shadow, 100.0 * double(ds.prof[15]) / double(ds.shadow ? ds.shadow : 1));
    if (ds.prof[16])   // render_cu_kernel: passes of the walk loops and the lanes that took part
      std::fprintf(stderr, "[vimg walk] box passes %llu lanes/pass %.2f   leaf rounds %llu lanes/round %.2f   sessions %llu   refills %llu rays/refill %.2f\n",
                   ds.prof[16], double(ds.prof[17]) / double(ds.prof[16]), ds.prof[18], double(ds.prof[19]) / double(ds.prof[18] ? ds.prof[18] : 1),
                   ds.prof[20], ds.prof[21], double(ds.prof[22]) / double(ds.prof[21] ? ds.prof[21] : 1));
    if (ds.wait_n[4])
      std::fprintf(stderr, "[vimg wait] mean cycles in a ring before a wave takes the slot: finisher %.0f  lambertian %.0f  principled %.0f  other %.0f  walk %.0f\n",
                   double(ds.wait_cyc[0]) / double(ds.wait_n[0] ? ds.wait_n[0] : 1), double(ds.wait_cyc[1]) / double(ds.wait_n[1] ? ds.wait_n[1] : 1),
                   double(ds.wait_cyc[2]) / double(ds.wait_n[2] ? ds.wait_n[2] : 1), double(ds.wait_cyc[3]) / double(ds.wait_n[3] ? ds.wait_n[3] : 1),
                   double(ds.wait_cyc[4]) / double(ds.wait_n[4]));
    if (ds.ray_cyc[1])
      std::fprintf(stderr, "[vimg wait] mean cycles of a ray in a walking lane (pop to hand-over) %.0f; of a vertex batch: finisher %.0f lambertian %.0f principled %.0f other %.0f\n",
                   double(ds.ray_cyc[0]) / double(ds.ray_cyc[1]), double(ds.prof[0]) / double(ds.prof[6] ? ds.prof[6] : 1), double(ds.prof[1]) / double(ds.prof[7] ? ds.prof[7] : 1),
                   double(ds.prof[2]) / double(ds.prof[8] ? ds.prof[8] : 1), double(ds.prof[3]) / double(ds.prof[9] ? ds.prof[9] : 1));
    if (ds.pv_cyc[6])
      std::fprintf(stderr, "[vimg wait] a Principled batch, mean cycles: state loads %.0f  hit record + path logic %.0f  light sample %.0f  BSDF sample %.0f  evaluations %.0f  stores + hand-over %.0f\n",
                   double(ds.pv_cyc[0]) / double(ds.pv_cyc[6]), double(ds.pv_cyc[1]) / double(ds.pv_cyc[6]), double(ds.pv_cyc[2]) / double(ds.pv_cyc[6]),
                   double(ds.pv_cyc[3]) / double(ds.pv_cyc[6]), double(ds.pv_cyc[4]) / double(ds.pv_cyc[6]), double(ds.pv_cyc[5]) / double(ds.pv_cyc[6]));
    if (ds.px_done[1])
      std::fprintf(stderr, "[vimg wait] pixels finished (last sample written) after: mean %.3f ms, latest %.3f ms\n",
                   double(ds.px_done[0]) / double(ds.px_done[1]) * 1e-5, double(ds.px_done[2]) * 1e-5);
    if (ds.px_done[1])
      std::fprintf(stderr, "[vimg wait] vertex-stage visits per pixel: mean %.1f, most %llu; the pixel that finished last: %llu visits in %.3f ms = %.2f us per visit (walks included)\n",
                   double(ds.px_hops[0]) / double(ds.px_done[1]), ds.px_hops[1], ds.px_hops[2] & 0xffffffull, double(ds.px_hops[2] >> 24) * 1e-5,
                   double(ds.px_hops[2] >> 24) * 1e-2 / double((ds.px_hops[2] & 0xffffffull) ? (ds.px_hops[2] & 0xffffffull) : 1));
    if (ds.prof[23])
      std::fprintf(stderr, "[vimg walk] cycles: refill+setup %llu  box %llu  leaf %llu  hand-over %llu   |  looks %llu  mean ring counts seen: finisher %.1f lambertian %.1f principled %.1f walk %.1f\n",
                   ds.walk_cyc[0], ds.walk_cyc[1], ds.walk_cyc[2], ds.walk_cyc[3], ds.prof[23], double(ds.prof[24]) / double(ds.prof[23]),
                   double(ds.prof[25]) / double(ds.prof[23]), double(ds.prof[26]) / double(ds.prof[23]), double(ds.prof[27]) / double(ds.prof[23]));
#ifdef VIMG_WALK_DIAG
    static const char* wd_names[12] = {"walk: refill+setup cyc", "walk: box loop cyc", "walk: leaf rounds cyc", "walk: retire cyc",
                                       "box trips", "box lanes", "leaf rounds", "leaf lanes", "leaf prim trips",
                                       "retire: cyc to get lock", "retire: cyc to unlock", "retire: lock takes"};
    for (int k = 0; k < 12; ++k) std::fprintf(stderr, "[vimg walk] %-24s %14llu\n", wd_names[k], ds.prof[16 + k]);
#endif
  }
  return VIMG_OK;
}

}  // namespace vimg

extern "C" {

const char* vimg_hip_last_error(void) { return g_err.c_str(); }

int vimg_hip_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(VIMG_E_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  return n;
}

int vimg_hip_init(int device_ordinal) {
  HIP_TRY(hipSetDevice(device_ordinal));
  if (!g_stream) HIP_TRY(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
  g_device = device_ordinal;
  return VIMG_OK;
}

void vimg_hip_options_default(VimgHipOptions* o) {
  if (!o) return;
  int32_t* f = reinterpret_cast<int32_t*>(o);
  for (size_t i = 1; i < sizeof(VimgHipOptions) / sizeof(int32_t); ++i) f[i] = VIMG_OPT_AUTO;
  o->struct_size = sizeof(VimgHipOptions);
}

int64_t vimg_hip_shard_pixels(const VimgDeviceScene* s, const VimgRenderParams* p) {
  int rc = check_params(s, p);
  if (rc) return rc;
  return int64_t(local_tiles(facts_of(s), *p)) * 64;
}

int vimg_hip_render_async(VimgDeviceScene* s, const VimgRenderParams* p, void* d_out, void* stream) {
  if (int rc = check_render(s, p, d_out)) return rc;
  return enqueue_render(s, p, {.d_out = static_cast<float*>(d_out), .st = stream_of(stream)});
}

int vimg_hip_check(VimgDeviceScene* s) {
  if (!s) return fail(VIMG_E_INVALID, "null scene");
  return check_kernel_error(s);
}

int vimg_hip_render(VimgDeviceScene* s, const VimgRenderParams* p, void* d_out, void* stream,
                    VimgRenderStats* stats) {
  if (int rc = check_render(s, p, d_out)) return rc;
  hipStream_t st = stream_of(stream);
  if (int rc = enqueue_render(s, p, {.d_out = static_cast<float*>(d_out), .st = st, .stats = stats != nullptr})) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (int rc2 = check_kernel_error(s)) return rc2;
  if (stats) return fetch_stats(s, p, stats);
  return VIMG_OK;
}

// ---- progressive rendering: a frame's samples in increments, bit for bit the one-shot render of their total.
// Between increments a pixel rests in a 32-byte record {rng lo, rng hi, -, -}{acc.xyz, -} per work item (the
// launch's compact tile-major order); a launch reads the records of the last good state and writes the other
// buffer, so a launch that fails leaves the accumulator where it was.
int vimg_hip_progressive_create(VimgDeviceScene* s, const VimgRenderParams* p, VimgProgressive** out) {
  if (!out) return fail(VIMG_E_INVALID, "progressive: null output handle");
  *out = nullptr;
  if (!s || !p) return fail(VIMG_E_INVALID, "progressive: null scene or params");
  VimgRenderParams q = *p;
  q.samples = 1;   // (ignored: every increment says how many)
  if (int rc = check_params(s, &q)) return rc;
  auto a = std::make_unique<VimgProgressive>();
  a->scene = s;
  a->generation = s->generation;
  a->params = q;
  a->items = uint64_t(local_tiles(facts_of(s), q)) * 64u;
  const size_t bytes = std::max<size_t>(a->items, 1) * 32u;
  for (auto& r : a->rec) {
    if (int rc = r.alloc(bytes)) return rc;
    HIP_TRY(hipMemset(r.p, 0, bytes));   // counts, increments and M2 of every pixel start at 0
  }
  a->valid_items = fetch_shard_pixels(s, &q);
  *out = a.release();
  return VIMG_OK;
}

// (the increments themselves, masked or not, and the accumulator's read-outs: progressive_adaptive.hip)
int vimg_hip_progressive_render(VimgDeviceScene* s, VimgProgressive* a, uint32_t samples, void* d_out, void* stream,
                                VimgRenderStats* stats) {
  return vimg_hip_progressive_render_masked(s, a, samples, nullptr, d_out, stream, stats);
}

uint64_t vimg_hip_progressive_samples(const VimgProgressive* a) { return a ? a->samples : 0u; }

int vimg_hip_progressive_reset(VimgProgressive* a) {
  if (!a) return fail(VIMG_E_INVALID, "progressive: null accumulator");
  // (_state and _error only enqueue, on any stream: they must have read the records before these are wiped)
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(a->rec[a->cur].p, 0, a->rec[a->cur].bytes));   // every pixel's count, increments and M2
  a->samples = 0;   // the next increment seeds every pixel again
  a->uniform = true;
  a->launches = 0;
  a->generation = a->scene->generation;
  return VIMG_OK;
}

int vimg_hip_progressive_free(VimgProgressive* a) {
  if (!a) return VIMG_OK;
  delete a;
  return VIMG_OK;
}

// heatmap_img (reference src/integrators/heatmap.cpp:38-147) behind the same boundary: the
// integrator field of the parameters is not used, samples and the tile shard are.
int vimg_hip_render_heatmap(VimgDeviceScene* s, const VimgRenderParams* p, float factor, void* d_out,
                            void* stream) {
  if (int rc = check_render(s, p, d_out)) return rc;
  if (factor <= 0) factor = 20.f;   // heatmap.cpp:137-139
  hipStream_t st = stream_of(stream);
  const LaunchCfg c = lane_layout(facts_of(s), *p);
  if (c.args.num_local_tiles == 0) return VIMG_OK;
  if (c.lds_bytes > 48u * 1024u)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(heatmap_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, int(c.lds_bytes)));
  const uint32_t grid = (c.args.num_local_tiles * 64u + 255u) / 256u;
  hipLaunchKernelGGL(heatmap_kernel, dim3(grid), dim3(256), c.lds_bytes, st, s->d, c.args, factor,
                     static_cast<float*>(d_out));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return VIMG_OK;
}

int vimg_hip_render_to_host(VimgDeviceScene* s, const VimgRenderParams* p, float* out_host,
                            VimgRenderStats* stats) {
  int rc = check_render(s, p, out_host);
  if (rc) return rc;
  if (p->tile_world != 1) return fail(VIMG_E_INVALID, "render_to_host needs tile_world == 1");
  const size_t floats = size_t(s->d.res_x) * s->d.res_y * 3;
  if ((rc = s->frame.grow(floats * sizeof(float)))) return rc;
  rc = vimg_hip_render(s, p, s->frame.p, nullptr, stats);
  if (rc) return rc;
  HIP_TRY(hipMemcpy(out_host, s->frame.p, floats * sizeof(float), hipMemcpyDeviceToHost));
  return VIMG_OK;
}

int vimg_hip_trace_pixel(VimgDeviceScene* s, const VimgRenderParams* p, int x, int y,
                         float* out_host) {
  int rc = check_params(s, p);
  if (rc) return rc;
  if (!out_host || x < 0 || y < 0 || x >= s->d.res_x || y >= s->d.res_y)
    return fail(VIMG_E_INVALID, "trace_pixel: pixel out of range");
  if ((rc = s->frame.grow(3 * sizeof(float)))) return rc;
  rc = enqueue_render(s, p, {.d_out = s->frame.as<float>(), .st = g_stream, .sx = x, .sy = y});
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(g_stream));
  HIP_TRY(hipMemcpy(out_host, s->frame.p, 3 * sizeof(float), hipMemcpyDeviceToHost));
  return VIMG_OK;
}

int vimg_hip_assemble_shards(const VimgDeviceScene* s, uint32_t world, int64_t shard_stride_pixels,
                             const void* d_shards, void* d_out, void* stream) {
  if (!s || !d_shards || !d_out || world == 0) return fail(VIMG_E_INVALID, "assemble: bad arguments");
  const uint32_t tx = tiles_of(s->d.res_x), ty = tiles_of(s->d.res_y);
  const uint64_t max_local = (uint64_t(tx) * ty + world - 1) / world;
  if (shard_stride_pixels < int64_t(max_local * 64))
    return fail(VIMG_E_INVALID, "assemble: shard stride smaller than the largest shard");
  hipStream_t st = stream_of(stream);
  const uint32_t threads = tx * ty * 64;
  hipLaunchKernelGGL(assemble_kernel, dim3((threads + 255) / 256), dim3(256), 0, st,
                     static_cast<const float*>(d_shards), static_cast<float*>(d_out),
                     uint32_t(s->d.res_x), uint32_t(s->d.res_y), tx, ty, world,
                     static_cast<long long>(shard_stride_pixels));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return VIMG_OK;
}

int vimg_hip_time_renders(VimgDeviceScene* s, const VimgRenderParams* p, void* d_out, int steps,
                          float* ms_per_launch) {
  int rc = check_params(s, p);
  if (rc) return rc;
  if (!d_out || steps <= 0 || !ms_per_launch) return fail(VIMG_E_INVALID, "time_renders: bad arguments");
  std::vector<DevEvent> ev(size_t(steps) * 2);
  for (auto& e : ev)
    if (int rc2 = e.create()) return rc2;
  for (int i = 0; i < steps; ++i) {
    // the counter / queue resets are part of a launch's prologue; the events bracket the kernel only
    if (int rc2 = enqueue_render(s, p, {.d_out = static_cast<float*>(d_out), .st = g_stream, .ev0 = ev[2 * i].e, .ev1 = ev[2 * i + 1].e}))
      return rc2;
  }
  HIP_TRY(hipStreamSynchronize(g_stream));
  if (int rc2 = check_kernel_error(s)) return rc2;
  for (int i = 0; i < steps; ++i) HIP_TRY(hipEventElapsedTime(&ms_per_launch[i], ev[2 * i].e, ev[2 * i + 1].e));
  return VIMG_OK;
}

// Unit-level probe (declared here, not in vimg_hip.h: it is a test hook, not part of the seam).
int vimg_hip_probe(VimgDeviceScene* s, int kind, int n, const float* in_host, float* out_host) {
  static const int n_in[11] = {0, 4, 6, 7, 12, 8, 4, 5, 1, 8, 12};
  static const int n_out[11] = {0, 8, 28, 1, 5, 7, 10, 4, 5, 8, 8};
  // 11 LAUNCH_BUILD (host only): in integrator samples depth tile_rank tile_world, out the fold of the PLAIN build a frame
  // with these parameters is launched with (plain_build.h: a mask of PF_*; 0 = the general build, or no CU launch at all)
  if (s && kind == 11 && n > 0 && in_host && out_host) {
    for (int i = 0; i < n; ++i) {
      const float* v = in_host + size_t(i) * 5;
      const VimgRenderParams p{uint32_t(v[0]), uint32_t(v[1]), uint32_t(v[2]), uint32_t(v[3]), uint32_t(v[4])};
      out_host[i] = 0.f;
      if (p.tile_world == 0 || p.tile_rank >= p.tile_world || is_feature_integrator(p.integrator)) continue;
      const LaunchCfg c = make_launch(s, &p, -1, -1);
      if (!c.error && c.sched == VIMG_SCHED_CU) out_host[i] = float(plain_fold_of(facts_of(s), c, false));
    }
    return VIMG_OK;
  }
  if (!s || kind < 1 || kind > 10 || n <= 0 || !in_host || !out_host)
    return fail(VIMG_E_INVALID, "probe: bad arguments");
  DevBuf d_in, d_out;
  if (int rc = d_in.alloc(size_t(n) * n_in[kind] * sizeof(float))) return rc;
  if (int rc = d_out.alloc(size_t(n) * n_out[kind] * sizeof(float))) return rc;
  HIP_TRY(hipMemcpy(d_in.p, in_host, size_t(n) * n_in[kind] * sizeof(float), hipMemcpyHostToDevice));
  VimgRenderParams p{VIMG_INTEGRATOR_MIS, 1, 1, 0, 1};
  const LaunchCfg c = lane_layout(facts_of(s), p);
  const uint32_t grid = (uint32_t(n) + 255) / 256;
  if (s->textured)
    hipLaunchKernelGGL(probe_kernel<true>, dim3(grid), dim3(256), c.lds_bytes, g_stream, s->d, c.args,
                       kind, n, d_in.as<float>(), d_out.as<float>());
  else
    hipLaunchKernelGGL(probe_kernel<false>, dim3(grid), dim3(256), c.lds_bytes, g_stream, s->d, c.args,
                       kind, n, d_in.as<float>(), d_out.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(g_stream));
  HIP_TRY(hipMemcpy(out_host, d_out.p, size_t(n) * n_out[kind] * sizeof(float), hipMemcpyDeviceToHost));
  return VIMG_OK;
}

}  // extern "C"
