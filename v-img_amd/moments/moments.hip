// libvimg_moments.so: the temporal accumulation with luminance moments of include/vimg_moments.h.
//
// One kernel over a history of four float4 planes [4][h][w]:
//   A    {r, g, b, L}         accumulated radiance, history length (0: no surface)
//   G0   {n.x, n.y, n.z, z}
//   G1   {P.x, P.y, P.z, 0}
//   M    {m1, m2, V, 0}       accumulated moments of luminance, variance of Y(A.rgb) (NaN: unknown)
// Planes A, G0, G1 and the rgb output are vimg_temporal_accumulate's: both kernels get the reprojection from
// frames/reproject.h and end it with the same blend.  Launch shape of frames/frame_lib.h: one lane per pixel, blockDim
// (64, 4), so a wave is 64 consecutive pixels of one row.  The current frame's reads (packed triples, one float of
// variance) and all writes are contiguous per wave; the up to four history taps are gathers wherever the old camera saw
// the pixel's surface point - a float4 of plane A, of each guide plane and, for a tap that counts, of plane M, which is
// read last: a tap the surface tests reject never touches it.  The tail is a bounds test.  The matrix and the
// parameters travel as kernel arguments.
//
// The arithmetic is the header's contract: built with -ffp-contract=off and without fast-math, so + - * / round once
// each, and the select forms below are the contract's comparisons (a NaN compares false), never fmaxf / fminf.
#include "vimg_moments.h"

#define FRAME_LIB "moments"
#include "../frames/frame_lib.h"
#include "../frames/guides.h"
#include "../frames/reproject.h"

namespace vimg_moments {

using namespace vimg_frames;

struct Constants {
  Reprojection r;
  float max_history, current_weight, min_history;
};

// `color` and `out`, `variance` and `out_var` may be the same buffer: none of them is __restrict__, and a lane reads
// its colour and its variance before it writes
__global__ __launch_bounds__(WAVE_X * ROWS) void moments_accumulate_kernel(
    uint32_t w, uint32_t h, const float* color, const float* __restrict__ normal, const float* __restrict__ position,
    const float* __restrict__ depth, const float* variance, const float4* __restrict__ prev, Constants k,
    float4* __restrict__ next, float* out, float* out_var) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t n = size_t(w) * h, p = size_t(y) * w + size_t(x), t = 3 * p;
  const float z = depth[t];
  const float cr = color[t], cg = color[t + 1], cb = color[t + 2];
  const float nx = normal[t], ny = normal[t + 1], nz = normal[t + 2];
  const float px = position[t], py = position[t + 1], pz = position[t + 2];
  const float v = variance ? variance[p] : 0.f;
  const bool vk = variance && v >= 0.f && v < INFINITY;
  next[n + p] = make_float4(nx, ny, nz, z);
  next[2 * n + p] = make_float4(px, py, pz, 0.f);

  const float unknown = __int_as_float(0x7fc00000);
  const float lc = lum(cr, cg, cb);
  float x2 = lc * lc;
  if (vk) x2 = x2 + v * (k.current_weight - 1.f);

  float4 a = make_float4(cr, cg, cb, 0.f);      // not live: a miss or a NaN depth
  float4 m = make_float4(lc, x2, 0.f, 0.f);
  if (z > 0.f) {
    a.w = 1.f;                                  // live without history
    m.z = vk ? v : unknown;
    Reprojected hst;
    float s1 = 0.f, s2 = 0.f;
    const auto moments_of = [&](float b, size_t q) {      // plane M, of a tap that counts alone
      const float4 mq = prev[3 * n + q];
      s1 = s1 + b * mq.x;
      s2 = s2 + b * mq.y;
    };
    if (reproject(w, h, prev, k.r, nx, ny, nz, px, py, pz, z, hst, moments_of)) {
      float cnt = hst.len + k.current_weight;
      if (cnt > k.max_history) cnt = k.max_history;
      float al = k.current_weight / cnt;
      if (al > 1.f) al = 1.f;
      a = make_float4(hst.hr + (cr - hst.hr) * al, hst.hg + (cg - hst.hg) * al, hst.hb + (cb - hst.hb) * al, cnt);

      const float m1h = s1 / hst.sumb, m2h = s2 / hst.sumb;
      float sh = m2h - m1h * m1h;
      if (sh < 0.f) sh = 0.f;
      const float vh = sh / hst.len;
      const float m1 = m1h + (lc - m1h) * al, m2 = m2h + (x2 - m2h) * al;
      float sc = m2 - m1 * m1;
      if (sc < 0.f) sc = 0.f;
      const float vc = vk ? v : sc / k.current_weight;
      const float u = 1.f - al;
      float var = (u * u) * vh + (al * al) * vc;
      if (!(cnt >= k.min_history)) var = unknown;      // too short a history to trust: the filter estimates spatially
      m = make_float4(m1, m2, var, 0.f);
    }
  }
  next[p] = a;
  next[3 * n + p] = m;
  if (out) {
    out[t] = a.x;
    out[t + 1] = a.y;
    out[t + 2] = a.z;
  }
  if (out_var) out_var[p] = m.z;
}

}  // namespace vimg_moments

using namespace vimg_moments;

extern "C" {

void vimg_moments_defaults(VimgMomentsParams* params) {
  if (!params) return;
  params->struct_size = sizeof(VimgMomentsParams);
  params->reserved = 0;
  params->max_history = 32.f;      // the first four: vimg_temporal_defaults'
  params->current_weight = 1.f;
  params->sigma_normal = 0.1f;
  params->sigma_plane = 0.00005f;
  params->min_history = 4.f;       // the header's "Defaults": SVGF's value, kept by the sweep of DESIGN.md 4.22
}

uint64_t vimg_moments_history_bytes(uint32_t width, uint32_t height) {
  return uint64_t(VIMG_MOMENTS_HISTORY_PER_PIXEL) * width * height;
}

int vimg_moments_accumulate(const VimgMomentsFrames* f, const void* d_prev_history, const float prev_world_to_pixel[12],
                            const VimgMomentsParams* a, void* d_next_history, void* d_out_rgb, void* d_out_variance,
                            void* stream) {
  if (const int rc = check_head(f, a, VIMG_MOMENTS_MAX_EXTENT)) return rc;
  if (!d_next_history) return fail(VIMG_E_INVALID, "moments: null next history");
  if (const int rc = check_float("max_history", a->max_history, 1.f, false, false)) return rc;
  if (const int rc = check_float("current_weight", a->current_weight, 1.f, false, false)) return rc;
  if (const int rc = check_float("sigma_normal", a->sigma_normal, 0.f, true, false)) return rc;
  if (const int rc = check_float("sigma_plane", a->sigma_plane, 0.f, true, false)) return rc;
  if (const int rc = check_float("min_history", a->min_history, 1.f, false, false)) return rc;
  if (a->min_history > a->max_history)
    return fail(VIMG_E_INVALID, "moments: min_history %g is above max_history %g", double(a->min_history), double(a->max_history));
  const uint32_t w = f->width, h = f->height;
  const uint64_t plane = uint64_t(4) * w * h;
  const ReadFrame reads[] = {{f->variance, plane, "variance"}};
  Constants k{};      // only the variance frame itself may be the output variance
  if (const int rc = check_reprojection(f, d_prev_history, prev_world_to_pixel, d_next_history, vimg_moments_history_bytes(w, h), reads,
                                        d_out_rgb, {d_out_variance, plane, "output variance overlaps", 0}, k.r))
    return rc;
  k.max_history = a->max_history;
  k.current_weight = a->current_weight;
  k.r.sigma_normal = a->sigma_normal;
  k.r.sigma_plane = a->sigma_plane;
  k.min_history = a->min_history;

  clear_stale_error();
  moments_accumulate_kernel<<<pixel_grid(w, h), pixel_block(), 0, static_cast<hipStream_t>(stream)>>>(
      w, h, static_cast<const float*>(f->color), static_cast<const float*>(f->normal), static_cast<const float*>(f->position),
      static_cast<const float*>(f->depth), static_cast<const float*>(f->variance), static_cast<const float4*>(d_prev_history), k,
      static_cast<float4*>(d_next_history), static_cast<float*>(d_out_rgb), static_cast<float*>(d_out_variance));
  return launched();
}

const char* vimg_moments_last_error(void) { return g_error; }

}  // extern "C"
