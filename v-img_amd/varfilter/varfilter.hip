// libvimg_varfilter.so: the variance-guided a-trous filter of include/vimg_varfilter.h.
//
// Five kernels - pack, estimate, one iteration, unpack, and the accumulator's variance - over planes of float4 in the
// caller's workspace:
//   C0, C1   the demodulated colour and the variance of its luminance, ping-pong   {r, g, b, V}
//   G0       {n.x, n.y, n.z, z}   (z > 0: the pixel is live)
//   G1       {P.x, P.y, P.z, 0}
// Launch shape (frames/frame_lib.h): one lane per pixel, blockDim (64, 4), so a wave is 64 consecutive pixels of one
// row and every plane load of a tap is one contiguous 1 KiB request per wave, whatever the step.  The 3 x 3 prefilter
// of an iteration is the one stage whose taps (step 1) share a tile: the workgroup stages {z, V} of its 64 x 4 pixels
// and a ring of one around them in LDS (3 KiB) and every lane reads its nine taps from there - measured against nine
// loads of the two fourth components per lane, which it beats by 12 us per iteration at 1800 x 800.
//
// The arithmetic is the header's contract, operation for operation: built with -ffp-contract=off and without
// fast-math, so + - * / round once each, and the select forms below are the contract's comparisons (a NaN compares
// false), never fmaxf / fminf.
#include "vimg_varfilter.h"

#define FRAME_LIB "varfilter"
#include "../frames/frame_lib.h"
#include "../frames/guides.h"

namespace vimg_varfilter {

using namespace vimg_frames;

__device__ inline float w_of(const float4* plane, size_t p) { return reinterpret_cast<const float*>(plane)[4 * p + 3]; }

__global__ __launch_bounds__(WAVE_X * ROWS) void varfilter_pack_kernel(
    uint32_t w, uint32_t h, const float* __restrict__ color, const float* __restrict__ normal,
    const float* __restrict__ position, const float* __restrict__ depth, const float* __restrict__ albedo,
    const float* __restrict__ variance, float floor, float4* __restrict__ c, float4* __restrict__ g0, float4* __restrict__ g1) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t p = size_t(y) * w + size_t(x), t = 3 * p;
  float r = color[t], g = color[t + 1], b = color[t + 2], ya = 1.f;
  if (albedo) {
    const float ar = floored(albedo[t], floor), ag = floored(albedo[t + 1], floor), ab = floored(albedo[t + 2], floor);
    r = r / ar;
    g = g / ag;
    b = b / ab;
    ya = lum(ar, ag, ab);
  }
  const float z = depth[t];
  float V = 0.f;
  if (z > 0.f) {
    V = -1.f;      // unknown: the estimate kernel fills it in
    if (variance) {
      const float v = variance[p];
      if (v >= 0.f && v < __builtin_huge_valf()) V = v / (ya * ya);
    }
  }
  c[p] = make_float4(r, g, b, V);
  g0[p] = make_float4(normal[t], normal[t + 1], normal[t + 2], z);
  g1[p] = make_float4(position[t], position[t + 1], position[t + 2], 0.f);
}

// Writes the fourth component of the pixel's own C alone, and reads the first three of its neighbours': no lane
// reads what another writes, so the plane is updated in place.
__global__ __launch_bounds__(WAVE_X * ROWS) void varfilter_estimate_kernel(
    uint32_t w, uint32_t h, float sigma_normal, float sigma_plane, float4* c, const float4* __restrict__ g0,
    const float4* __restrict__ g1) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t p = size_t(y) * w + size_t(x);
  const float4 np = g0[p];
  if (!(np.w > 0.f)) return;
  float* vp = reinterpret_cast<float*>(c) + (4 * p + 3);
  if (!(*vp < 0.f)) return;
  const float* cf = reinterpret_cast<const float*>(c);
  const float4 pp = g1[p];
  const float sz = sigma_plane * np.w;
  const float plane_den = sz * sz;
  float sw = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int dy = -3; dy <= 3; ++dy) {
#pragma unroll
    for (int dx = -3; dx <= 3; ++dx) {
      float wq, lq;
      if (dx == 0 && dy == 0) {
        wq = 1.f;
        lq = lum(cf[4 * p], cf[4 * p + 1], cf[4 * p + 2]);
      } else {
        const int qx = x + dx, qy = y + dy;
        if (uint32_t(qx) >= w || uint32_t(qy) >= h) continue;
        const size_t q = size_t(qy) * w + size_t(qx);
        const float4 nq = g0[q];
        if (!(nq.w > 0.f)) continue;
        lq = lum(cf[4 * q], cf[4 * q + 1], cf[4 * q + 2]);
        if (!((lq - lq) == 0.f)) continue;      // not finite: no one's tap
        const float S = guide_score(np, pp, nq, g1[q], sigma_normal, plane_den);
        const float one_s = 1.f - S;
        wq = S < 1.f ? one_s * one_s : 0.f;
      }
      if (wq > 0.f) {
        sw = sw + wq;
        s1 = s1 + wq * lq;
        s2 = s2 + wq * (lq * lq);
      }
    }
  }
  const float m1 = s1 / sw, m2 = s2 / sw;
  const float V = m2 - m1 * m1;
  *vp = V < 0.f ? 0.f : V;
}

// sigma_normal, the plane term's denominator and the luminance term's are divided by, as the contract says: no reciprocals
__global__ __launch_bounds__(WAVE_X * ROWS) void varfilter_iteration_kernel(
    uint32_t w, uint32_t h, int step, float sigma_normal, float sigma_plane, float sl2, float variance_floor,
    const float4* __restrict__ cin, const float4* __restrict__ g0, const float4* __restrict__ g1, float4* __restrict__ cout) {
  // the prefilter's tile: {z, V} of the workgroup's pixels and a ring of one around them, z = 0 outside the image.
  // Every lane of the workgroup takes part, the ones past the image's edge too: they leave after the barrier
  __shared__ float2 tile[ROWS + 2][WAVE_X + 2];
  {
    const int bx = int(blockIdx.x * WAVE_X) - 1, by = int(blockIdx.y * ROWS) - 1;
    for (int i = int(threadIdx.y * WAVE_X + threadIdx.x); i < (ROWS + 2) * (WAVE_X + 2); i += WAVE_X * ROWS) {
      const int ty = i / (WAVE_X + 2), tx = i - ty * (WAVE_X + 2);
      const int rx = bx + tx, ry = by + ty;
      float2 v = make_float2(0.f, 0.f);
      if (uint32_t(rx) < w && uint32_t(ry) < h) {
        const size_t r = size_t(ry) * w + size_t(rx);
        v = make_float2(w_of(g0, r), w_of(cin, r));
      }
      tile[ty][tx] = v;
    }
  }
  __syncthreads();
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t p = size_t(y) * w + size_t(x);
  const float4 cp = cin[p];
  const float4 np = g0[p];
  if (!(np.w > 0.f)) {      // a miss or a NaN depth: not live, keeps its colour and its variance
    cout[p] = cp;
    return;
  }
  // the 3 x 3 Gaussian of the variance over the live taps (the centre is one of them: p is live)
  const float bk[3] = {1.f / 4.f, 1.f / 2.f, 1.f / 4.f};
  float sg = 0.f, sv = 0.f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const float g = bk[dx + 1] * bk[dy + 1];
      const float2 t = tile[int(threadIdx.y) + 1 + dy][int(threadIdx.x) + 1 + dx];
      if (!(t.x > 0.f)) continue;       // outside the image (z = 0) or not live
      sg = sg + g;
      sv = sv + g * t.y;
    }
  }
  const float Vg = sv / sg;
  const float den = sl2 * Vg + variance_floor;

  const float4 pp = g1[p];
  const float sz = sigma_plane * np.w;
  const float plane_den = sz * sz;
  const float lp = lum(cp.x, cp.y, cp.z);
  const float hk[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
  float sumw = 0.f, sr = 0.f, sgr = 0.f, sb = 0.f, sumv = 0.f;
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
        cq = cin[q];
        const float dl = lp - lum(cq.x, cq.y, cq.z);
        const float S = guide_score(np, pp, nq, g1[q], sigma_normal, plane_den) + (dl * dl) / den;
        const float one_s = 1.f - S;
        wq = S < 1.f ? k * (one_s * one_s) : 0.f;
      }
      if (wq > 0.f) {
        sumw = sumw + wq;
        sr = sr + wq * cq.x;
        sgr = sgr + wq * cq.y;
        sb = sb + wq * cq.z;
        sumv = sumv + (wq * wq) * cq.w;
      }
    }
  }
  cout[p] = make_float4(sr / sumw, sgr / sumw, sb / sumw, sumv / (sumw * sumw));
}

__global__ __launch_bounds__(WAVE_X * ROWS) void varfilter_unpack_kernel(
    uint32_t w, uint32_t h, const float4* __restrict__ c, const float* __restrict__ albedo, float floor, float* __restrict__ out,
    float* __restrict__ out_variance) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t p = size_t(y) * w + size_t(x), t = 3 * p;
  const float4 v = c[p];
  float r = v.x, g = v.y, b = v.z, ya = 1.f;
  if (albedo) {
    const float ar = floored(albedo[t], floor), ag = floored(albedo[t + 1], floor), ab = floored(albedo[t + 2], floor);
    r = r * ar;
    g = g * ag;
    b = b * ab;
    ya = lum(ar, ag, ab);
  }
  out[t] = r;
  out[t + 1] = g;
  out[t + 2] = b;
  if (out_variance) out_variance[p] = v.w * (ya * ya);
}

// out may be m2 itself: a lane reads its own item before it writes it
__global__ __launch_bounds__(WAVE_X * ROWS) void varfilter_variance_kernel(uint32_t w, uint32_t h, const uint32_t* count,
                                                                         const uint32_t* batches, const float* m2, float* out) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t p = size_t(y) * w + size_t(x);
  const uint32_t N = count[p], K = batches[p];
  const float m = m2[p];
  out[p] = (K < 2u || N == 0u) ? __builtin_nanf("") : ((m < 0.f ? 0.f : m) / static_cast<float>(K - 1u)) / static_cast<float>(N);
}

}  // namespace vimg_varfilter

using namespace vimg_varfilter;

extern "C" {

void vimg_varfilter_defaults(VimgVarFilterParams* params) {
  if (!params) return;
  params->struct_size = sizeof(VimgVarFilterParams);
  params->iterations = 3;      // the header's "Defaults": chosen by error figures measured on the GPU
  params->sigma_luminance = 8.f;
  params->sigma_normal = 0.5f;
  params->sigma_plane = 0.005f;
  params->albedo_floor = 1.f / 64.f;
  params->variance_floor = 1e-8f;
}

uint64_t vimg_varfilter_workspace(uint32_t width, uint32_t height) {
  return uint64_t(VIMG_VARFILTER_WORKSPACE_PER_PIXEL) * width * height;
}

int vimg_varfilter_atrous(const VimgVarFilterFrames* f, const VimgVarFilterParams* a, void* d_out_rgb, void* d_out_variance,
                          void* d_workspace, uint64_t workspace_bytes, void* stream) {
  if (const int rc = check_head(f, a, VIMG_VARFILTER_MAX_EXTENT)) return rc;
  if (!d_out_rgb) return fail(VIMG_E_INVALID, "varfilter: null output");
  if (a->iterations < 1 || a->iterations > VIMG_VARFILTER_MAX_ITERATIONS)
    return fail(VIMG_E_INVALID, "varfilter: iterations must be 1..%u, not %u", VIMG_VARFILTER_MAX_ITERATIONS, a->iterations);
  if (const int rc = check_float("sigma_luminance", a->sigma_luminance, 0.f, true, true)) return rc;
  if (const int rc = check_float("sigma_normal", a->sigma_normal, 0.f, true, false)) return rc;
  if (const int rc = check_float("sigma_plane", a->sigma_plane, 0.f, true, false)) return rc;
  if (const int rc = check_float("albedo_floor", a->albedo_floor, 0.f, true, false)) return rc;
  if (const int rc = check_float("variance_floor", a->variance_floor, 0.f, true, false)) return rc;
  const uint32_t w = f->width, h = f->height;
  if (const int rc = check_workspace(d_workspace, workspace_bytes, vimg_varfilter_workspace(w, h), w, h)) return rc;

  const size_t n = size_t(w) * h;
  float4* base = static_cast<float4*>(d_workspace);
  float4 *c0 = base, *c1 = base + n, *g0 = base + 2 * n, *g1 = base + 3 * n;
  const dim3 block = pixel_block(), grid = pixel_grid(w, h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* albedo = static_cast<const float*>(f->albedo);

  clear_stale_error();
  varfilter_pack_kernel<<<grid, block, 0, s>>>(w, h, static_cast<const float*>(f->color), static_cast<const float*>(f->normal),
                                               static_cast<const float*>(f->position), static_cast<const float*>(f->depth), albedo,
                                               static_cast<const float*>(f->variance), a->albedo_floor, c0, g0, g1);
  if (const int rc = launched("pack")) return rc;
  varfilter_estimate_kernel<<<grid, block, 0, s>>>(w, h, a->sigma_normal, a->sigma_plane, c0, g0, g1);
  if (const int rc = launched("estimate")) return rc;
  const float sl2 = a->sigma_luminance * a->sigma_luminance;
  float4 *src = c0, *dst = c1;
  for (uint32_t i = 0; i < a->iterations; ++i) {
    varfilter_iteration_kernel<<<grid, block, 0, s>>>(w, h, 1 << i, a->sigma_normal, a->sigma_plane, sl2, a->variance_floor, src, g0,
                                                      g1, dst);
    if (const int rc = launched("iteration")) return rc;
    float4* t = src;
    src = dst;
    dst = t;
  }
  varfilter_unpack_kernel<<<grid, block, 0, s>>>(w, h, src, albedo, a->albedo_floor, static_cast<float*>(d_out_rgb),
                                                 static_cast<float*>(d_out_variance));
  return launched("unpack");
}

int vimg_varfilter_variance(uint32_t width, uint32_t height, const void* d_count, const void* d_batches, const void* d_m2,
                            void* d_out_variance, void* stream) {
  if (width == 0 || height == 0 || width > VIMG_VARFILTER_MAX_EXTENT || height > VIMG_VARFILTER_MAX_EXTENT)
    return fail(VIMG_E_INVALID, "varfilter: width and height must be 1..%u, not %u x %u", VIMG_VARFILTER_MAX_EXTENT, width, height);
  if (!d_count || !d_batches || !d_m2 || !d_out_variance)
    return fail(VIMG_E_INVALID, "varfilter: null %s", !d_count ? "count" : !d_batches ? "batches" : !d_m2 ? "m2" : "output variance");
  clear_stale_error();
  varfilter_variance_kernel<<<pixel_grid(width, height), pixel_block(), 0, static_cast<hipStream_t>(stream)>>>(
      width, height, static_cast<const uint32_t*>(d_count), static_cast<const uint32_t*>(d_batches), static_cast<const float*>(d_m2),
      static_cast<float*>(d_out_variance));
  return launched("variance");
}

const char* vimg_varfilter_last_error(void) { return g_error; }

}  // extern "C"
