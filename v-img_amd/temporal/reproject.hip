// libvimg_temporal.so: the temporal accumulation of include/vimg_temporal.h.
//
// One kernel over a history of three float4 planes [3][h][w]:
//   A    {r, g, b, L}         accumulated radiance, history length (0: no surface)
//   G0   {n.x, n.y, n.z, z}
//   G1   {P.x, P.y, P.z, 0}
// The reprojection itself - the projection, the tap tests, the means of the accepted taps - is frames/reproject.h's,
// which the moments and the weighted library build on too, and so are the checks of the histories and the output.
// Launch shape of frames/frame_lib.h: one lane per pixel, blockDim (64, 4), so a wave is 64 consecutive pixels of one
// row.  The current frame's reads (packed triples) and all writes are contiguous per wave; the up to four history taps
// are gathers wherever the old camera saw the pixel's surface point, a whole float4 of plane A and xyz of the guide
// planes.  The tail is a bounds test.  The matrix and the parameters travel as kernel arguments.
//
// The arithmetic is the header's contract, operation for operation: built with -ffp-contract=off and without
// fast-math, so + - * / round once each, and the select forms below are the contract's comparisons (a NaN compares
// false), never fmaxf / fminf.
#include "vimg_temporal.h"

#define FRAME_LIB "temporal"
#include "../frames/frame_lib.h"
#include "../frames/reproject.h"

namespace vimg_temporal {

using namespace vimg_frames;

struct Constants {
  Reprojection r;
  float max_history, current_weight;
};

// `color` and `out` may be the same buffer: neither is __restrict__, and a lane reads its colour before it writes
__global__ __launch_bounds__(WAVE_X * ROWS) void temporal_accumulate_kernel(
    uint32_t w, uint32_t h, const float* color, const float* __restrict__ normal, const float* __restrict__ position,
    const float* __restrict__ depth, const float4* __restrict__ prev, Constants k, float4* __restrict__ next, float* out) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t n = size_t(w) * h, p = size_t(y) * w + size_t(x), t = 3 * p;
  const float z = depth[t];
  const float cr = color[t], cg = color[t + 1], cb = color[t + 2];
  const float nx = normal[t], ny = normal[t + 1], nz = normal[t + 2];
  const float px = position[t], py = position[t + 1], pz = position[t + 2];
  next[n + p] = make_float4(nx, ny, nz, z);
  next[2 * n + p] = make_float4(px, py, pz, 0.f);

  float4 a = make_float4(cr, cg, cb, 0.f);      // not live: a miss or a NaN depth
  if (z > 0.f) {
    a.w = 1.f;                                  // live without history
    Reprojected hst;
    if (reproject(w, h, prev, k.r, nx, ny, nz, px, py, pz, z, hst, [](float, size_t) {})) {
      float cnt = hst.len + k.current_weight;
      if (cnt > k.max_history) cnt = k.max_history;
      float al = k.current_weight / cnt;
      if (al > 1.f) al = 1.f;
      a = make_float4(hst.hr + (cr - hst.hr) * al, hst.hg + (cg - hst.hg) * al, hst.hb + (cb - hst.hb) * al, cnt);
    }
  }
  next[p] = a;
  if (out) {
    out[t] = a.x;
    out[t + 1] = a.y;
    out[t + 2] = a.z;
  }
}

}  // namespace vimg_temporal

using namespace vimg_temporal;

extern "C" {

void vimg_temporal_defaults(VimgTemporalParams* params) {
  if (!params) return;
  params->struct_size = sizeof(VimgTemporalParams);
  params->reserved = 0;
  params->max_history = 32.f;      // the header's "Defaults": checked by error figures measured on the GPU
  params->current_weight = 1.f;
  params->sigma_normal = 0.1f;
  params->sigma_plane = 0.00005f;
}

uint64_t vimg_temporal_history_bytes(uint32_t width, uint32_t height) {
  return uint64_t(VIMG_TEMPORAL_HISTORY_PER_PIXEL) * width * height;
}

int vimg_temporal_accumulate(const VimgTemporalFrames* f, const void* d_prev_history, const float prev_world_to_pixel[12],
                             const VimgTemporalParams* a, void* d_next_history, void* d_out_rgb, void* stream) {
  if (const int rc = check_head(f, a, VIMG_TEMPORAL_MAX_EXTENT)) return rc;
  if (!d_next_history) return fail(VIMG_E_INVALID, "temporal: null next history");
  if (const int rc = check_float("max_history", a->max_history, 1.f, false, false)) return rc;
  if (const int rc = check_float("current_weight", a->current_weight, 1.f, false, false)) return rc;
  if (const int rc = check_float("sigma_normal", a->sigma_normal, 0.f, true, false)) return rc;
  if (const int rc = check_float("sigma_plane", a->sigma_plane, 0.f, true, false)) return rc;
  const uint32_t w = f->width, h = f->height;
  Constants k{};
  if (const int rc = check_reprojection(f, d_prev_history, prev_world_to_pixel, d_next_history, vimg_temporal_history_bytes(w, h), {},
                                        d_out_rgb, {}, k.r))
    return rc;
  k.max_history = a->max_history;
  k.current_weight = a->current_weight;
  k.r.sigma_normal = a->sigma_normal;
  k.r.sigma_plane = a->sigma_plane;

  clear_stale_error();
  temporal_accumulate_kernel<<<pixel_grid(w, h), pixel_block(), 0, static_cast<hipStream_t>(stream)>>>(
      w, h, static_cast<const float*>(f->color), static_cast<const float*>(f->normal), static_cast<const float*>(f->position),
      static_cast<const float*>(f->depth), static_cast<const float4*>(d_prev_history), k, static_cast<float4*>(d_next_history),
      static_cast<float*>(d_out_rgb));
  return launched();
}

const char* vimg_temporal_last_error(void) { return g_error; }

}  // extern "C"
