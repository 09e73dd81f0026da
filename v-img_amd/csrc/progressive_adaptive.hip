// Adaptive sampling on a progressive accumulator (include/vimg_hip.h): increments that reach
// only the pixels of a mask, the per-pixel error they leave, and the mask of the pixels that still need samples.
// The samples themselves are the render kernels'; this unit builds their item lists and keeps the per-pixel
// counts and statistics in the accumulator's records (adaptive_kernels.h).
#include "hip_internal.h"
#include "adaptive_kernels.h"

using namespace vimg;

namespace {

AdaptGeom geom_of(const VimgProgressive* a) {
  const VimgDeviceScene* s = a->scene;
  return AdaptGeom{uint32_t(a->items), a->params.tile_rank, a->params.tile_world, tiles_of(s->d.res_x),
                   tiles_of(s->d.res_y), uint32_t(s->d.res_x), uint32_t(s->d.res_y)};
}
uint32_t blocks_of(uint64_t items, uint32_t per) { return uint32_t((items + per - 1) / per); }

int ensure_scratch(VimgProgressive* a) {
  if (int rc = a->ctl.grow(ACTL_WORDS * sizeof(uint32_t))) return rc;
  if (int rc = a->item_list.grow(std::max<size_t>(a->items, 1) * sizeof(uint32_t))) return rc;
  return a->block_counts.grow(std::max<size_t>(blocks_of(a->items, ADAPT_BLOCK), 1) * sizeof(uint32_t));
}

// what every call on an accumulator checks first
int check_acc(const VimgProgressive* a, const char* what) {
  if (!a) return fail(VIMG_E_INVALID, std::string(what) + ": null accumulator");
  return VIMG_OK;
}

}  // namespace

extern "C" {

int vimg_hip_progressive_render_masked(VimgDeviceScene* s, VimgProgressive* a, uint32_t samples, const uint8_t* d_mask,
                                       void* d_out, void* stream, VimgRenderStats* stats) {
  if (!s || !a) return fail(VIMG_E_INVALID, "progressive: null scene or accumulator");
  if (a->scene != s) return fail(VIMG_E_INVALID, "progressive: the accumulator belongs to another scene");
  if (a->generation != s->generation)
    return fail(VIMG_E_INVALID, "progressive: the scene changed (geometry or camera) since the accumulator's records "
                                "were made; reset it");
  if (samples == 0) return fail(VIMG_E_INVALID, "samples must be > 0");
  const bool everyone = a->uniform && !d_mask;   // the plain increment: one launch over every item, no list
  if (everyone && uint64_t(a->samples) + samples > 0xffffffffull)
    return fail(VIMG_E_INVALID, "progressive: more than 2^32 - 1 samples per pixel in all (the reference counts them in 32 bits)");
  VimgRenderParams p = a->params;
  p.samples = samples;
  if (int rc = check_params(s, &p)) return rc;
  hipStream_t st = stream_of(stream);
  void* d_user_out = d_out;
  if (!d_out) {   // advance only: the render kernels' means go to a buffer of the accumulator's
    const size_t floats = (p.tile_world == 1 ? size_t(s->d.res_x) * s->d.res_y : size_t(a->items)) * 3u;
    if (int rc = a->scratch.grow(std::max<size_t>(floats, 3) * sizeof(float))) return rc;
    d_out = a->scratch.p;
  }
  const AdaptGeom G = geom_of(a);
  const v4u* old_rec = a->rec[a->cur].as<v4u>();
  v4u* new_rec = a->rec[a->cur ^ 1].as<v4u>();
  const uint32_t carry_blocks = blocks_of(a->items, 256u);
  uint64_t launches = 0, paths = 0;
  uint32_t top = a->samples;      // the largest count of any pixel after this call
  bool uniform_after = a->uniform;

  if (everyone) {
    const ProgLaunch pl{a->samples, old_rec, new_rec};
    if (int rc = enqueue_render(s, &p, {.d_out = static_cast<float*>(d_out), .st = st, .stats = stats != nullptr, .prog = &pl}))
      return rc;
    launches = a->items ? 1 : 0;
    paths = a->valid_items * samples;
    top = a->samples + samples;
  } else {
    if (int rc = ensure_scratch(a)) return rc;
    uint32_t* ctl = a->ctl.as<uint32_t>();
    const uint32_t list_blocks = blocks_of(a->items, ADAPT_BLOCK);
    if (a->items) {
      hipLaunchKernelGGL(adapt_ctl_init_kernel, dim3(1), dim3(64), 0, st, ctl);
      hipLaunchKernelGGL(adapt_first_class_kernel, dim3(list_blocks), dim3(ADAPT_BLOCK), 0, st, G, d_mask, old_rec, ctl);
    }
    // The 32-bit bound.  a->samples is the largest count of any pixel, so the usual call is cleared on the host
    // with no device work.  Only when that bound would be passed does the answer depend on WHICH pixels are
    // selected, and the mask lives on the device: then the largest selected count is read back first (two small
    // read-only kernels, the accumulator's control words the only thing written) and the call refused here.
    if (a->items && uint64_t(a->samples) + samples > 0xffffffffull) {
      uint32_t max_sel = 0;
      HIP_TRY(hipMemcpyAsync(&max_sel, ctl + ACTL_MAXSEL, sizeof(max_sel), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (uint64_t(max_sel) + samples > 0xffffffffull)
        return fail(VIMG_E_INVALID, "progressive: more than 2^32 - 1 samples in all for a selected pixel (the reference "
                                    "counts them in 32 bits)");
    }
    // one round per distinct count among the selected pixels: its list, then its launch (the sample base is a
    // launch constant).  The host reads three words per round: the class, its length, the next class.
    while (a->items) {
      hipLaunchKernelGGL(adapt_round_kernel, dim3(1), dim3(64), 0, st, ctl);
      hipLaunchKernelGGL(adapt_list_kernel<false>, dim3(list_blocks), dim3(ADAPT_BLOCK), 0, st, G, d_mask, old_rec, ctl,
                         a->block_counts.as<uint32_t>(), a->item_list.as<uint32_t>());
      hipLaunchKernelGGL(adapt_scan_kernel, dim3(1), dim3(ADAPT_BLOCK), 0, st, a->block_counts.as<uint32_t>(), list_blocks, ctl);
      hipLaunchKernelGGL(adapt_list_kernel<true>, dim3(list_blocks), dim3(ADAPT_BLOCK), 0, st, G, d_mask, old_rec, ctl,
                         a->block_counts.as<uint32_t>(), a->item_list.as<uint32_t>());
      HIP_TRY(hipGetLastError());
      uint32_t w[4] = {0, 0, 0, 0};
      HIP_TRY(hipMemcpyAsync(w, ctl, sizeof(w), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      const uint32_t cls = w[ACTL_CLASS], len = w[ACTL_LEN], next = w[ACTL_NEXT];
      if (len == 0) break;   // nothing selected
      const ProgLaunch pl{cls, old_rec, new_rec, a->item_list.as<uint32_t>(), len, launches != 0};
      if (int rc = enqueue_render(s, &p, {.d_out = static_cast<float*>(d_out), .st = st, .stats = stats != nullptr, .prog = &pl}))
        return rc;
      ++launches;
      paths += uint64_t(len) * samples;
      top = std::max(top, cls + samples);
      if (len != a->valid_items) uniform_after = false;
      if (next == 0xffffffffu) break;
    }
    if (launches > 1) uniform_after = false;
  }
  // the books: counts, increments and M2 of the rendered pixels, every other record carried into the new buffer
  if (a->items)
    hipLaunchKernelGGL(adapt_carry_kernel, dim3(carry_blocks), dim3(256), 0, st, G, d_mask, old_rec, new_rec, samples);
  if (!everyone && d_user_out && a->items)
    hipLaunchKernelGGL(adapt_resolve_kernel, dim3(carry_blocks), dim3(256), 0, st, G, (const v4u*)new_rec,
                       static_cast<float*>(d_user_out), (float*)nullptr, (uint8_t*)nullptr, 0.f, 0u, (uint32_t*)nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  if (int rc2 = check_kernel_error(s)) return rc2;
  // every launch succeeded: the accumulator advances
  a->cur ^= 1;
  a->samples = top;
  a->uniform = uniform_after;
  a->launches += launches;
  if (stats) {
    if (launches) {
      if (int rc = fetch_stats(s, &p, stats)) return rc;
    } else {
      *stats = VimgRenderStats{};
    }
    stats->paths = paths;
  }
  return VIMG_OK;
}

uint64_t vimg_hip_progressive_launches(const VimgProgressive* a) { return a ? a->launches : 0u; }

int vimg_hip_progressive_state(VimgProgressive* a, void* d_sum_rgb, void* d_count, void* d_batches, void* d_m2,
                               void* stream) {
  if (int rc = check_acc(a, "progressive_state")) return rc;
  hipStream_t st = stream_of(stream);
  if (!a->items || (!d_sum_rgb && !d_count && !d_batches && !d_m2)) return VIMG_OK;
  hipLaunchKernelGGL(adapt_state_kernel, dim3(blocks_of(a->items, 256u)), dim3(256), 0, st, geom_of(a),
                     (const v4u*)a->rec[a->cur].as<v4u>(), static_cast<float*>(d_sum_rgb), static_cast<uint32_t*>(d_count),
                     static_cast<uint32_t*>(d_batches), static_cast<float*>(d_m2));
  HIP_TRY(hipGetLastError());
  return VIMG_OK;
}

int vimg_hip_progressive_error(VimgProgressive* a, void* d_err, void* stream) {
  if (int rc = check_acc(a, "progressive_error")) return rc;
  if (!d_err) return fail(VIMG_E_INVALID, "progressive_error: null output pointer");
  hipStream_t st = stream_of(stream);
  if (!a->items) return VIMG_OK;
  hipLaunchKernelGGL(adapt_resolve_kernel, dim3(blocks_of(a->items, 256u)), dim3(256), 0, st, geom_of(a),
                     (const v4u*)a->rec[a->cur].as<v4u>(), (float*)nullptr, static_cast<float*>(d_err), (uint8_t*)nullptr,
                     0.f, 0u, (uint32_t*)nullptr);
  HIP_TRY(hipGetLastError());
  return VIMG_OK;
}

int vimg_hip_progressive_select(VimgProgressive* a, float target, uint32_t max_samples, uint8_t* d_mask, void* stream,
                                uint32_t* active_out) {
  if (int rc = check_acc(a, "progressive_select")) return rc;
  if (!d_mask || !active_out) return fail(VIMG_E_INVALID, "progressive_select: null mask or count pointer");
  if (!(target >= 0.f)) return fail(VIMG_E_INVALID, "progressive_select: the target must be a number >= 0");
  *active_out = 0;
  hipStream_t st = stream_of(stream);
  if (!a->items) return VIMG_OK;
  if (int rc = ensure_scratch(a)) return rc;
  uint32_t* ctl = a->ctl.as<uint32_t>();
  hipLaunchKernelGGL(adapt_ctl_init_kernel, dim3(1), dim3(64), 0, st, ctl);
  hipLaunchKernelGGL(adapt_resolve_kernel, dim3(blocks_of(a->items, 256u)), dim3(256), 0, st, geom_of(a),
                     (const v4u*)a->rec[a->cur].as<v4u>(), (float*)nullptr, (float*)nullptr, d_mask, target, max_samples, ctl);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(active_out, ctl + ACTL_ACTIVE, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return VIMG_OK;
}

}  // extern "C"
