// libvimg_wtemporal.so: the temporal accumulation with per-pixel weights of include/vimg_wtemporal.h.
//
// One kernel over libvimg_temporal's history of three float4 planes [3][h][w]:
//   A    {r, g, b, L}         accumulated radiance, history length (0: nothing to carry)
//   G0   {n.x, n.y, n.z, z}
//   G1   {P.x, P.y, P.z, 0}
// The reprojection is frames/reproject.h's and the launch shape frames/frame_lib.h's, as in temporal/reproject.hip:
// one lane per pixel, blockDim (64, 4), so a wave is 64 consecutive pixels of one row.  The current frame's reads
// (packed triples, and one float of the weight frame: 256 contiguous bytes per wave) and all writes are contiguous per
// wave - the code is 64 contiguous bytes per wave; the up to four history taps are gathers wherever the old camera saw
// the pixel's surface point, a whole float4 of plane A and xyz of the guide planes.  The tail is a bounds test.  The
// matrix and the parameters travel as kernel arguments.  Against temporal_accumulate_kernel: 4 bytes more read and at
// most 1 more written per pixel.
//
// The arithmetic is the header's contract, operation for operation: built with -ffp-contract=off and without
// fast-math, so + - * / round once each, and the select forms below are the contract's comparisons (a NaN compares
// false), never fmaxf / fminf.
#include "vimg_wtemporal.h"

#define FRAME_LIB "wtemporal"
#include "../frames/frame_lib.h"
#include "../frames/reproject.h"

namespace vimg_wtemporal {

using namespace vimg_frames;

struct Constants {
  Reprojection r;
  float max_history;
};

// `color` and `out` may be the same buffer: neither is __restrict__, and a lane reads its colour before it writes
__global__ __launch_bounds__(WAVE_X * ROWS) void wtemporal_accumulate_kernel(
    uint32_t w, uint32_t h, const float* color, const float* __restrict__ normal, const float* __restrict__ position,
    const float* __restrict__ depth, const float* __restrict__ weight, const float4* __restrict__ prev, Constants k,
    float4* __restrict__ next, float* out, uint8_t* __restrict__ code) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t n = size_t(w) * h, p = size_t(y) * w + size_t(x), t = 3 * p;
  const float z = depth[t];
  const float cr = color[t], cg = color[t + 1], cb = color[t + 2];
  const float nx = normal[t], ny = normal[t + 1], nz = normal[t + 2];
  const float px = position[t], py = position[t + 1], pz = position[t + 2];
  const float wp = weight[p];
  const float wt = wp > 0.f ? wp : 0.f;         // a NaN or negative weight is 0
  next[n + p] = make_float4(nx, ny, nz, z);
  next[2 * n + p] = make_float4(px, py, pz, 0.f);

  float4 a = make_float4(cr, cg, cb, 0.f);      // not live: a miss or a NaN depth
  uint8_t what = VIMG_WTEMPORAL_DEAD;
  if (z > 0.f) {
    const bool worth = wt > 0.f;
    a.w = worth ? (wt < 1.f ? wt : 1.f) : 0.f;  // live without history: started, or shown and not carried
    what = worth ? VIMG_WTEMPORAL_STARTED : VIMG_WTEMPORAL_SHOWN;
    Reprojected hst;
    if (reproject(w, h, prev, k.r, nx, ny, nz, px, py, pz, z, hst, [](float, size_t) {})) {
      if (worth) {
        float cnt = hst.len + wt;
        if (cnt > k.max_history) cnt = k.max_history;
        float al = wt / cnt;
        if (al > 1.f) al = 1.f;
        a = make_float4(hst.hr + (cr - hst.hr) * al, hst.hg + (cg - hst.hg) * al, hst.hb + (cb - hst.hb) * al, cnt);
        what = VIMG_WTEMPORAL_BLENDED;
      } else {                           // the history alone: a colour worth nothing does not enter it
        float cnt = hst.len;
        if (cnt > k.max_history) cnt = k.max_history;
        a = make_float4(hst.hr, hst.hg, hst.hb, cnt);
        what = VIMG_WTEMPORAL_CARRIED;
      }
    }
  }
  next[p] = a;
  if (out) {
    out[t] = a.x;
    out[t + 1] = a.y;
    out[t + 2] = a.z;
  }
  if (code) code[p] = what;
}

}  // namespace vimg_wtemporal

using namespace vimg_wtemporal;

extern "C" {

void vimg_wtemporal_defaults(VimgWTemporalParams* params) {
  if (!params) return;
  params->struct_size = sizeof(VimgWTemporalParams);
  params->reserved = 0;
  params->max_history = 32.f;      // libvimg_temporal's defaults (include/vimg_temporal.h, "Defaults")
  params->sigma_normal = 0.1f;
  params->sigma_plane = 0.00005f;
}

int vimg_wtemporal_accumulate(const VimgWTemporalFrames* f, const void* d_prev_history, const float prev_world_to_pixel[12],
                              const VimgWTemporalParams* a, void* d_next_history, void* d_out_rgb, void* d_out_code,
                              void* stream) {
  static_assert(VIMG_WTEMPORAL_HISTORY_PER_PIXEL == 3 * sizeof(float4), "the history is three float4 planes");
  if (const int rc = check_head(f, a, VIMG_WTEMPORAL_MAX_EXTENT)) return rc;
  if (!f->weight) return fail(VIMG_E_INVALID, "wtemporal: null weight frame");
  if (!d_next_history) return fail(VIMG_E_INVALID, "wtemporal: null next history");
  if (const int rc = check_float("max_history", a->max_history, 1.f, false, false)) return rc;
  if (const int rc = check_float("sigma_normal", a->sigma_normal, 0.f, true, false)) return rc;
  if (const int rc = check_float("sigma_plane", a->sigma_plane, 0.f, true, false)) return rc;
  const uint32_t w = f->width, h = f->height;
  const uint64_t hist = uint64_t(VIMG_WTEMPORAL_HISTORY_PER_PIXEL) * w * h;
  const ReadFrame reads[] = {{f->weight, uint64_t(4) * w * h, "weight", 4}};
  Constants k{};
  if (const int rc = check_reprojection(f, d_prev_history, prev_world_to_pixel, d_next_history, hist, reads, d_out_rgb,
                                        {d_out_code, uint64_t(w) * h, "output codes overlap"}, k.r))
    return rc;
  k.max_history = a->max_history;
  k.r.sigma_normal = a->sigma_normal;
  k.r.sigma_plane = a->sigma_plane;

  clear_stale_error();
  wtemporal_accumulate_kernel<<<pixel_grid(w, h), pixel_block(), 0, static_cast<hipStream_t>(stream)>>>(
      w, h, static_cast<const float*>(f->color), static_cast<const float*>(f->normal), static_cast<const float*>(f->position),
      static_cast<const float*>(f->depth), static_cast<const float*>(f->weight), static_cast<const float4*>(d_prev_history), k,
      static_cast<float4*>(d_next_history), static_cast<float*>(d_out_rgb), static_cast<uint8_t*>(d_out_code));
  return launched();
}

const char* vimg_wtemporal_last_error(void) { return g_error; }

}  // extern "C"
