// libvimg_filter.so: the edge-avoiding a-trous filter of include/vimg_filter.h.
//
// Three kernels - pack, one iteration, unpack - over planes of float4 in the caller's workspace:
//   C0, C1   the demodulated colour, ping-pong            {r, g, b, -}
//   G0       {n.x, n.y, n.z, z}   (z > 0: the pixel is live)
//   G1       {P.x, P.y, P.z, 0}
// Launch shape (frames/frame_lib.h): one lane per pixel, blockDim (64, 4), so a wave is 64 consecutive pixels of one
// row and every plane load of a tap is one contiguous 1 KiB request per wave, whatever the step.
//
// The arithmetic is the header's contract, operation for operation: built with -ffp-contract=off and without
// fast-math, so + - * / round once each, and the select forms below are the contract's comparisons (a NaN compares
// false), never fmaxf / fminf.
#include "vimg_filter.h"

#define FRAME_LIB "atrous"
#include "../frames/frame_lib.h"
#include "../frames/guides.h"

namespace vimg_filter {

using namespace vimg_frames;

struct Planes {
  float4* c0;
  float4* c1;
  float4* g0;
  float4* g1;
};

__global__ __launch_bounds__(WAVE_X * ROWS) void atrous_pack_kernel(
    uint32_t w, uint32_t h, const float* __restrict__ color, const float* __restrict__ normal,
    const float* __restrict__ position, const float* __restrict__ depth, const float* __restrict__ albedo, float floor,
    float4* __restrict__ c, float4* __restrict__ g0, float4* __restrict__ g1) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t p = size_t(y) * w + size_t(x), t = 3 * p;
  float r = color[t], g = color[t + 1], b = color[t + 2];
  if (albedo) {
    r = r / floored(albedo[t], floor);
    g = g / floored(albedo[t + 1], floor);
    b = b / floored(albedo[t + 2], floor);
  }
  c[p] = make_float4(r, g, b, 0.f);
  g0[p] = make_float4(normal[t], normal[t + 1], normal[t + 2], depth[t]);
  g1[p] = make_float4(position[t], position[t + 1], position[t + 2], 0.f);
}

// sigma_normal, the plane term's denominator and the colour term's are divided by, as the contract says: no reciprocals
__global__ __launch_bounds__(WAVE_X * ROWS) void atrous_iteration_kernel(
    uint32_t w, uint32_t h, int step, float sigma_normal, float sigma_plane, float sigma_color_i,
    const float4* __restrict__ cin, const float4* __restrict__ g0, const float4* __restrict__ g1, float4* __restrict__ cout) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t p = size_t(y) * w + size_t(x);
  const float4 cp = cin[p];
  const float4 np = g0[p];
  if (!(np.w > 0.f)) {      // a miss or a NaN depth: not live, keeps its colour
    cout[p] = cp;
    return;
  }
  const float4 pp = g1[p];
  const float sz = sigma_plane * np.w;
  const float plane_den = sz * sz;
  const float color_den = sigma_color_i * sigma_color_i;
  const float hk[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
  float sumw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const float k = hk[dx + 2] * hk[dy + 2];
      float wq;
      float4 cq;
      if (dx == 0 && dy == 0) {
        wq = k;
        cq = cp;
      } else {
        const int qx = x + step * dx, qy = y + step * dy;       // |step * d| <= 2^12, x, y < 2^15
        if (uint32_t(qx) >= w || uint32_t(qy) >= h) continue;
        const size_t q = size_t(qy) * w + size_t(qx);
        const float4 nq = g0[q];
        if (!(nq.w > 0.f)) continue;
        const float4 pq = g1[q];
        cq = cin[q];
        const float s_g = guide_score(np, pp, nq, pq, sigma_normal, plane_den);
        const float cx = cp.x - cq.x, cy = cp.y - cq.y, cz = cp.z - cq.z;
        const float s_c = ((cx * cx + cy * cy) + cz * cz) / color_den;
        const float S = s_g + s_c;
        const float one_s = 1.f - S;
        wq = S < 1.f ? k * (one_s * one_s) : 0.f;
      }
      if (wq > 0.f) {
        sumw = sumw + wq;
        sr = sr + wq * cq.x;
        sg = sg + wq * cq.y;
        sb = sb + wq * cq.z;
      }
    }
  }
  cout[p] = make_float4(sr / sumw, sg / sumw, sb / sumw, 0.f);
}

__global__ __launch_bounds__(WAVE_X * ROWS) void atrous_unpack_kernel(
    uint32_t w, uint32_t h, const float4* __restrict__ c, const float* __restrict__ albedo, float floor, float* __restrict__ out) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t p = size_t(y) * w + size_t(x), t = 3 * p;
  const float4 v = c[p];
  float r = v.x, g = v.y, b = v.z;
  if (albedo) {
    r = r * floored(albedo[t], floor);
    g = g * floored(albedo[t + 1], floor);
    b = b * floored(albedo[t + 2], floor);
  }
  out[t] = r;
  out[t + 1] = g;
  out[t + 2] = b;
}

}  // namespace vimg_filter

using namespace vimg_filter;

extern "C" {

void vimg_filter_atrous_defaults(VimgAtrousParams* params) {
  if (!params) return;
  params->struct_size = sizeof(VimgAtrousParams);
  params->iterations = 3;      // the header's "Defaults": chosen by error figures measured on the GPU
  params->sigma_color = 2.f;
  params->sigma_normal = 0.5f;
  params->sigma_plane = 0.005f;
  params->albedo_floor = 1.f / 64.f;
}

uint64_t vimg_filter_atrous_workspace(uint32_t width, uint32_t height) {
  return uint64_t(VIMG_ATROUS_WORKSPACE_PER_PIXEL) * width * height;
}

int vimg_filter_atrous(const VimgFilterFrames* f, const VimgAtrousParams* a, void* d_out_rgb, void* d_workspace,
                       uint64_t workspace_bytes, void* stream) {
  if (const int rc = check_head(f, a, VIMG_FILTER_MAX_EXTENT)) return rc;
  if (!d_out_rgb) return fail(VIMG_E_INVALID, "atrous: null output");
  if (a->iterations < 1 || a->iterations > VIMG_ATROUS_MAX_ITERATIONS)
    return fail(VIMG_E_INVALID, "atrous: iterations must be 1..%u, not %u", VIMG_ATROUS_MAX_ITERATIONS, a->iterations);
  if (const int rc = check_float("sigma_color", a->sigma_color, 0.f, true, true)) return rc;
  if (const int rc = check_float("sigma_normal", a->sigma_normal, 0.f, true, false)) return rc;
  if (const int rc = check_float("sigma_plane", a->sigma_plane, 0.f, true, false)) return rc;
  if (const int rc = check_float("albedo_floor", a->albedo_floor, 0.f, true, false)) return rc;
  const uint32_t w = f->width, h = f->height;
  if (const int rc = check_workspace(d_workspace, workspace_bytes, vimg_filter_atrous_workspace(w, h), w, h)) return rc;

  const size_t n = size_t(w) * h;
  float4* base = static_cast<float4*>(d_workspace);
  const Planes pl{base, base + n, base + 2 * n, base + 3 * n};
  const dim3 block = pixel_block(), grid = pixel_grid(w, h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* albedo = static_cast<const float*>(f->albedo);

  clear_stale_error();
  atrous_pack_kernel<<<grid, block, 0, s>>>(w, h, static_cast<const float*>(f->color), static_cast<const float*>(f->normal),
                                            static_cast<const float*>(f->position), static_cast<const float*>(f->depth), albedo,
                                            a->albedo_floor, pl.c0, pl.g0, pl.g1);
  if (const int rc = launched("pack")) return rc;
  float4 *src = pl.c0, *dst = pl.c1;
  float scale = 1.f;      // 2^-i
  for (uint32_t i = 0; i < a->iterations; ++i) {
    atrous_iteration_kernel<<<grid, block, 0, s>>>(w, h, 1 << i, a->sigma_normal, a->sigma_plane, a->sigma_color * scale, src,
                                                   pl.g0, pl.g1, dst);
    if (const int rc = launched("iteration")) return rc;
    float4* t = src;
    src = dst;
    dst = t;
    scale = scale * 0.5f;
  }
  atrous_unpack_kernel<<<grid, block, 0, s>>>(w, h, src, albedo, a->albedo_floor, static_cast<float*>(d_out_rgb));
  return launched("unpack");
}

const char* vimg_filter_last_error(void) { return g_error; }

}  // extern "C"
