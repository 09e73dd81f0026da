// libvimg_wtemporal.so: the temporal accumulation with per-pixel weights of include/vimg_wtemporal.h.
//
// One kernel over libvimg_temporal's history of three float4 planes [3][h][w]:
//   A    {r, g, b, L}         accumulated radiance, history length (0: nothing to carry)
//   G0   {n.x, n.y, n.z, z}
//   G1   {P.x, P.y, P.z, 0}
// The launch shape and the plane accesses are temporal/reproject.hip's (frames/frame_lib.h): one lane per pixel,
// blockDim (64, 4), so a wave is 64 consecutive pixels of one row.  The current frame's reads (packed triples, and
// one float of the weight frame: 256 contiguous bytes per wave) and all writes are contiguous per wave - the code is
// 64 contiguous bytes per wave; the up to four history taps are gathers wherever the old camera saw the pixel's
// surface point, a whole float4 of plane A and xyz of the guide planes.  The tail is a bounds test.  The matrix and the
// parameters travel as kernel arguments.  Against reproject: 4 bytes more read and at most 1 more written per pixel.
//
// The arithmetic is the header's contract, operation for operation: built with -ffp-contract=off and without
// fast-math, so + - * / round once each, and the select forms below are the contract's comparisons (a NaN compares
// false), never fmaxf / fminf.
#include "vimg_wtemporal.h"

#define FRAME_LIB "wtemporal"
#include "../frames/frame_lib.h"

namespace vimg_wtemporal {

using namespace vimg_frames;

struct Constants {
  float m[12];     // prev_world_to_pixel, row-major 3 x 4
  float max_history, sigma_normal, sigma_plane;
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
    if (prev) {
      const float hx = ((k.m[0] * px + k.m[1] * py) + k.m[2] * pz) + k.m[3];
      const float hy = ((k.m[4] * px + k.m[5] * py) + k.m[6] * pz) + k.m[7];
      const float hw = ((k.m[8] * px + k.m[9] * py) + k.m[10] * pz) + k.m[11];
      if (hw > 0.f) {
        const float fx = hx / hw - 0.5f, fy = hy / hw - 0.5f;
        if (fx > -1.f && fx < float(w) && fy > -1.f && fy < float(h)) {
          const float x0 = floorf(fx), y0 = floorf(fy);      // -1 .. w - 1, -1 .. h - 1: exact as int
          const float tx = fx - x0, ty = fy - y0;
          const float ux = 1.f - tx, uy = 1.f - ty;
          const float b[4] = {ux * uy, tx * uy, ux * ty, tx * ty};
          const int ix = int(x0), iy = int(y0);
          const float sz = k.sigma_plane * z;
          const float plane = sz * sz;
          float sumb = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sl = 0.f;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int qx = ix + (i & 1), qy = iy + (i >> 1);
            if (uint32_t(qx) >= w || uint32_t(qy) >= h) continue;
            if (!(b[i] > 0.f)) continue;
            const size_t q = size_t(qy) * w + size_t(qx);
            const float4 hq = prev[q];
            if (!(hq.w > 0.f)) continue;
            const float4 nq = prev[n + q];
            const float dn = 1.f - ((nx * nq.x + ny * nq.y) + nz * nq.z);
            if (!(dn < k.sigma_normal)) continue;
            const float4 pq = prev[2 * n + q];
            const float ex = pq.x - px, ey = pq.y - py, ez = pq.z - pz;
            const float d = (nx * ex + ny * ey) + nz * ez;
            if (!(d * d < plane)) continue;
            sumb = sumb + b[i];
            sr = sr + b[i] * hq.x;
            sg = sg + b[i] * hq.y;
            sb = sb + b[i] * hq.z;
            sl = sl + b[i] * hq.w;
          }
          if (sumb > 0.f) {
            const float hr = sr / sumb, hg = sg / sumb, hb = sb / sumb, len = sl / sumb;
            if (worth) {
              float cnt = len + wt;
              if (cnt > k.max_history) cnt = k.max_history;
              float al = wt / cnt;
              if (al > 1.f) al = 1.f;
              a = make_float4(hr + (cr - hr) * al, hg + (cg - hg) * al, hb + (cb - hb) * al, cnt);
              what = VIMG_WTEMPORAL_BLENDED;
            } else {                           // the history alone: a colour worth nothing does not enter it
              float cnt = len;
              if (cnt > k.max_history) cnt = k.max_history;
              a = make_float4(hr, hg, hb, cnt);
              what = VIMG_WTEMPORAL_CARRIED;
            }
          }
        }
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
  if (reinterpret_cast<uintptr_t>(d_next_history) % 16)
    return fail(VIMG_E_INVALID, "wtemporal: the next history must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(f->weight) % 4)
    return fail(VIMG_E_INVALID, "wtemporal: the weight frame must be 4-byte aligned");
  Constants k{};
  if (d_prev_history) {
    if (reinterpret_cast<uintptr_t>(d_prev_history) % 16)
      return fail(VIMG_E_INVALID, "wtemporal: the previous history must be 16-byte aligned");
    if (!prev_world_to_pixel)
      return fail(VIMG_E_INVALID, "wtemporal: a previous history needs its world-to-pixel matrix");
  }
  if (prev_world_to_pixel)
    for (int i = 0; i < 12; ++i) {
      if (!std::isfinite(prev_world_to_pixel[i]))
        return fail(VIMG_E_INVALID, "wtemporal: world-to-pixel entry %d is not finite (%g)", i, double(prev_world_to_pixel[i]));
      k.m[i] = prev_world_to_pixel[i];
    }
  const uint32_t w = f->width, h = f->height;
  const uint64_t hist = uint64_t(VIMG_WTEMPORAL_HISTORY_PER_PIXEL) * w * h, frame = uint64_t(12) * w * h;
  const uint64_t plane = uint64_t(4) * w * h, codes = uint64_t(w) * h;
  if (d_prev_history && overlaps(d_next_history, hist, d_prev_history, hist))
    return fail(VIMG_E_INVALID, "wtemporal: the next history overlaps the previous one");
  const void* frames[4] = {f->color, f->normal, f->position, f->depth};
  const char* names[4] = {"color", "normal", "position", "depth"};
  for (int i = 0; i < 4; ++i)
    if (overlaps(d_next_history, hist, frames[i], frame))
      return fail(VIMG_E_INVALID, "wtemporal: the next history overlaps the %s frame", names[i]);
  if (overlaps(d_next_history, hist, f->weight, plane))
    return fail(VIMG_E_INVALID, "wtemporal: the next history overlaps the weight frame");
  if (d_out_rgb) {      // other lanes gather from prev and read the guides; only the colour frame itself may be the output
    if (d_prev_history && overlaps(d_out_rgb, frame, d_prev_history, hist))
      return fail(VIMG_E_INVALID, "wtemporal: the output overlaps the previous history");
    if (overlaps(d_out_rgb, frame, d_next_history, hist))
      return fail(VIMG_E_INVALID, "wtemporal: the output overlaps the next history");
    for (int i = 0; i < 4; ++i)
      if (overlaps(d_out_rgb, frame, frames[i], frame) && !(i == 0 && d_out_rgb == f->color))
        return fail(VIMG_E_INVALID, i == 0 ? "wtemporal: the output overlaps the %s frame without being it"
                                           : "wtemporal: the output overlaps the %s frame", names[i]);
    if (overlaps(d_out_rgb, frame, f->weight, plane))
      return fail(VIMG_E_INVALID, "wtemporal: the output overlaps the weight frame");
  }
  if (d_out_code) {
    if (d_prev_history && overlaps(d_out_code, codes, d_prev_history, hist))
      return fail(VIMG_E_INVALID, "wtemporal: the output codes overlap the previous history");
    if (overlaps(d_out_code, codes, d_next_history, hist))
      return fail(VIMG_E_INVALID, "wtemporal: the output codes overlap the next history");
    for (int i = 0; i < 4; ++i)
      if (overlaps(d_out_code, codes, frames[i], frame))
        return fail(VIMG_E_INVALID, "wtemporal: the output codes overlap the %s frame", names[i]);
    if (overlaps(d_out_code, codes, f->weight, plane))
      return fail(VIMG_E_INVALID, "wtemporal: the output codes overlap the weight frame");
    if (d_out_rgb && overlaps(d_out_code, codes, d_out_rgb, frame))
      return fail(VIMG_E_INVALID, "wtemporal: the output codes overlap the output");
  }
  k.max_history = a->max_history;
  k.sigma_normal = a->sigma_normal;
  k.sigma_plane = a->sigma_plane;

  clear_stale_error();
  wtemporal_accumulate_kernel<<<pixel_grid(w, h), pixel_block(), 0, static_cast<hipStream_t>(stream)>>>(
      w, h, static_cast<const float*>(f->color), static_cast<const float*>(f->normal), static_cast<const float*>(f->position),
      static_cast<const float*>(f->depth), static_cast<const float*>(f->weight), static_cast<const float4*>(d_prev_history), k,
      static_cast<float4*>(d_next_history), static_cast<float*>(d_out_rgb), static_cast<uint8_t*>(d_out_code));
  return launched();
}

const char* vimg_wtemporal_last_error(void) { return g_error; }

}  // extern "C"
