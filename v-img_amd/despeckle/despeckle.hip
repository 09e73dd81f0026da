// libvimg_despeckle.so: the clamp of fireflies of include/vimg_despeckle.h.
//
// Two kernels - pack, clamp - over two planes of float4 in the caller's workspace:
//   G0   {n.x, n.y, n.z, z}          (z > 0: the pixel is live)
//   G1   {P.x, P.y, P.z, L}          L: the luminance of the demodulated colour
// Launch shape (frames/frame_lib.h): one lane per pixel, blockDim (64, 4), so a wave is 64 consecutive pixels of one
// row.  The clamp kernel first stages its workgroup's tile of the two planes with an apron of R pixels,
// (64 + 2R) x (4 + 2R) float4 each, in LDS (21.9 KB at R = 3) - contiguous 1 KiB requests per wave, as
// infill_fill_kernel does - so the up to 48 taps of a pixel are LDS reads and every plane value is fetched once per
// workgroup, not once per tap; a cell outside the image reads as "not live", so the window needs no bounds test.  The
// radius is a template argument: the window unrolls.  A tap is straight-line code: an accepted tap goes on as its
// luminance, which is >= 0, and one that is not as -inf - the count and the sum take "v >= 0" as a select, and in the
// rank list -inf is above nothing - the list is four registers t1..t4 whatever the rank, each step of an insertion
// two selects, and t_rank is picked at the end: the first `rank` entries of the four largest ARE the `rank` largest, in the
// contract's order (entry k depends on the entries before it alone).  `color` and `albedo` are read again only to
// write the output, with the pack's own division, so a clamped pixel's C has the pack's bits.
//
// The arithmetic is the header's contract, operation for operation: built with -ffp-contract=off and without
// fast-math, so + - * / round once each, and the select forms below are the contract's comparisons (a NaN compares
// false), never fmaxf / fminf.
#include "vimg_despeckle.h"

#define FRAME_LIB "despeckle"
#include "../frames/frame_lib.h"
#include "../frames/guides.h"
#include "../frames/tile.h"

namespace vimg_despeckle {

using namespace vimg_frames;

__global__ __launch_bounds__(WAVE_X * ROWS) void despeckle_pack_kernel(
    uint32_t w, uint32_t h, const float* __restrict__ color, const float* __restrict__ normal,
    const float* __restrict__ position, const float* __restrict__ depth, const float* __restrict__ albedo, float floor,
    float4* __restrict__ g0, float4* __restrict__ g1) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t p = size_t(y) * w + size_t(x), t = 3 * p;
  const float z = depth[t];
  float r = color[t], g = color[t + 1], b = color[t + 2];
  if (albedo && z > 0.f) {
    r = r / floored(albedo[t], floor);
    g = g / floored(albedo[t + 1], floor);
    b = b / floored(albedo[t + 2], floor);
  }
  g0[p] = make_float4(normal[t], normal[t + 1], normal[t + 2], z);
  g1[p] = make_float4(position[t], position[t + 1], position[t + 2], lum(r, g, b));
}

// one step of an insertion into the descending list: the larger of v and t stays in t, the smaller goes on in v
__device__ inline void sift(float& v, float& t) {
  const bool above = v > t;
  const float hi = above ? v : t;
  v = above ? t : v;
  t = hi;
}

// `color` and `out` may be the same buffer: neither is __restrict__, and a lane touches its own pixel of them alone
template <int R>
__global__ __launch_bounds__(WAVE_X * ROWS) void despeckle_clamp_kernel(
    uint32_t w, uint32_t h, uint32_t rank, uint32_t min_taps, float gain, float sigma_normal, float sigma_plane, float floor,
    const float* color, const float* __restrict__ albedo, const float4* __restrict__ g0, const float4* __restrict__ g1,
    float* out, uint8_t* __restrict__ code) {
  int x, y;
  const bool inside = pixel_of(w, h, x, y);
  // the workgroup's tile with its apron, row-major; a cell outside the image reads as "not live"
  constexpr int TW = tile_width<R>;
  __shared__ float4 t0[tile_cells<R>], t1[tile_cells<R>];
  const int lp = stage_tile<R>([&](int i, int gx, int gy) {
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    if (uint32_t(gx) < w && uint32_t(gy) < h) {
      const size_t q = size_t(gy) * w + size_t(gx);
      v0 = g0[q];
      v1 = g1[q];
    }
    t0[i] = v0;
    t1[i] = v1;
  });
  if (!inside) return;
  const size_t p = size_t(y) * w + size_t(x), t = 3 * p;
  const float4 np = t0[lp], pp = t1[lp];
  const float cr = color[t], cg = color[t + 1], cb = color[t + 2];
  float r = cr, g = cg, b = cb;
  uint8_t what = VIMG_DESPECKLE_NOT_LIVE;
  if (np.w > 0.f) {
    const float sz = sigma_plane * np.w;
    const float plane_den = sz * sz;
    const float ninf = -__builtin_huge_valf();
    float k1 = ninf, k2 = ninf, k3 = ninf, k4 = ninf;      // t_1 .. t_4
    float sum = 0.f;
    uint32_t m = 0;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
      for (int dx = -R; dx <= R; ++dx) {
        if (dx == 0 && dy == 0) continue;
        const int lq = lp + dy * TW + dx;
        const float4 nq = t0[lq], pq = t1[lq];
        const float S = guide_score(np, pp, nq, pq, sigma_normal, plane_den);
        // accepted: v = L_q >= 0; not accepted: v = -inf, and the one value says which
        float v = nq.w > 0.f && S < 1.f && pq.w >= 0.f ? pq.w : ninf;
        const bool ok = v >= 0.f;
        m += ok ? 1u : 0u;
        sum = ok ? sum + v : sum;
        sift(v, k1);
        sift(v, k2);
        sift(v, k3);
        sift(v, k4);
      }
      // an empty statement that "writes" the six running values: a row of taps is finished before the next begins.
      // Without it the compiler runs t_1's 48 insertions first and keeps every comparison's wave mask for the other
      // three lists: 110 spilled SGPRs and 153 VGPRs at R = 3; with it none, and 60 (DESIGN.md 4.20's table)
      asm volatile("" : "+v"(k1), "+v"(k2), "+v"(k3), "+v"(k4), "+v"(sum), "+v"(m));
    }
    what = VIMG_DESPECKLE_FEW_TAPS;
    if (m >= min_taps) {
      what = VIMG_DESPECKLE_KEPT;
      const float t_rank = rank == 1 ? k1 : rank == 2 ? k2 : rank == 3 ? k3 : k4;
      const float mean = sum / float(m);
      const float bound = mean > t_rank ? mean : t_rank;
      const float T = gain * bound;
      const float Lp = pp.w;
      if (Lp > T && Lp < __builtin_huge_valf()) {
        const float f = T / Lp;
        if (albedo) {
          const float ar = floored(albedo[t], floor), ag = floored(albedo[t + 1], floor), ab = floored(albedo[t + 2], floor);
          r = ((cr / ar) * f) * ar;
          g = ((cg / ag) * f) * ag;
          b = ((cb / ab) * f) * ab;
        } else {
          r = cr * f;
          g = cg * f;
          b = cb * f;
        }
        what = VIMG_DESPECKLE_CLAMPED;
      }
    }
  }
  out[t] = r;
  out[t + 1] = g;
  out[t + 2] = b;
  if (code) code[p] = what;
}

}  // namespace vimg_despeckle

using namespace vimg_despeckle;

extern "C" {

void vimg_despeckle_defaults(VimgDespeckleParams* params) {
  if (!params) return;
  params->struct_size = sizeof(VimgDespeckleParams);
  params->radius = 1;      // the header's "Defaults": gain by the sweep of DESIGN.md 4.30
  params->rank = 3;
  params->min_taps = 4;
  params->gain = 3.f;
  params->sigma_normal = 0.5f;
  params->sigma_plane = 0.005f;
  params->albedo_floor = 1.f / 64.f;
}

uint64_t vimg_despeckle_workspace(uint32_t width, uint32_t height) {
  return uint64_t(VIMG_DESPECKLE_WORKSPACE_PER_PIXEL) * width * height;
}

int vimg_despeckle_clamp(const VimgDespeckleFrames* f, const VimgDespeckleParams* a, void* d_out_rgb, void* d_out_code,
                         void* d_workspace, uint64_t workspace_bytes, void* stream) {
  if (const int rc = check_head(f, a, VIMG_DESPECKLE_MAX_EXTENT)) return rc;
  if (!d_out_rgb) return fail(VIMG_E_INVALID, "despeckle: null output");
  const uint32_t w = f->width, h = f->height;
  const uint64_t need = vimg_despeckle_workspace(w, h);
  if (const int rc = check_workspace(d_workspace, workspace_bytes, need, w, h)) return rc;
  if (a->radius < 1 || a->radius > VIMG_DESPECKLE_MAX_RADIUS)
    return fail(VIMG_E_INVALID, "despeckle: radius must be 1..%u, not %u", VIMG_DESPECKLE_MAX_RADIUS, a->radius);
  if (a->rank < 1 || a->rank > VIMG_DESPECKLE_MAX_RANK)
    return fail(VIMG_E_INVALID, "despeckle: rank must be 1..%u, not %u", VIMG_DESPECKLE_MAX_RANK, a->rank);
  const uint32_t window = (2 * a->radius + 1) * (2 * a->radius + 1) - 1;
  if (a->min_taps < a->rank || a->min_taps > window)
    return fail(VIMG_E_INVALID, "despeckle: min_taps must be %u..%u, not %u", a->rank, window, a->min_taps);
  if (const int rc = check_float("gain", a->gain, 1.f, false, false)) return rc;
  if (const int rc = check_float("sigma_normal", a->sigma_normal, 0.f, true, false)) return rc;
  if (const int rc = check_float("sigma_plane", a->sigma_plane, 0.f, true, false)) return rc;
  if (const int rc = check_float("albedo_floor", a->albedo_floor, 0.f, true, false)) return rc;
  // other lanes read the planes, and pack reads every frame before clamp writes: only the colour frame itself may be
  // the output
  const uint64_t frame = uint64_t(12) * w * h, codes = uint64_t(w) * h;
  const Range others[] = {{f->color, frame, "color frame"}, {f->normal, frame, "normal frame"}, {f->position, frame, "position frame"},
                          {f->depth, frame, "depth frame"}, {f->albedo, frame, "albedo frame"}, {d_out_code, codes, "output codes"},
                          {d_workspace, need, "workspace"}};
  if (const Range* r = first_overlap(d_out_rgb, frame, std::span(others).subspan(d_out_rgb == f->color ? 1 : 0)))
    return fail(VIMG_E_INVALID, "despeckle: the output overlaps the %s%s", r->name, r == others ? " without being it" : "");
  if (d_out_code && overlaps(d_out_code, codes, d_workspace, need))
    return fail(VIMG_E_INVALID, "despeckle: the output codes overlap the workspace");

  const size_t n = size_t(w) * h;
  float4* g0 = static_cast<float4*>(d_workspace);
  float4* g1 = g0 + n;
  const dim3 block = pixel_block(), grid = pixel_grid(w, h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* color = static_cast<const float*>(f->color);
  const float* albedo = static_cast<const float*>(f->albedo);

  clear_stale_error();
  despeckle_pack_kernel<<<grid, block, 0, s>>>(w, h, color, static_cast<const float*>(f->normal),
                                               static_cast<const float*>(f->position), static_cast<const float*>(f->depth), albedo,
                                               a->albedo_floor, g0, g1);
  if (const int rc = launched("pack")) return rc;
  float* out = static_cast<float*>(d_out_rgb);
  uint8_t* code = static_cast<uint8_t*>(d_out_code);
  with_radius<VIMG_DESPECKLE_MAX_RADIUS>(a->radius, [&](auto R) {
    despeckle_clamp_kernel<R.value><<<grid, block, 0, s>>>(w, h, a->rank, a->min_taps, a->gain, a->sigma_normal, a->sigma_plane,
                                                           a->albedo_floor, color, albedo, g0, g1, out, code);
  });
  return launched("clamp");
}

const char* vimg_despeckle_last_error(void) { return g_error; }

}  // extern "C"
