// libvimg_rectify.so: the clamp of a long history to a short one of include/vimg_rectify.h.
//
// One kernel over two histories of libvimg_temporal's layout, three float4 planes [3][h][w] (A = {r, g, b, L},
// G0 = {n, z}, G1 = {P, 0}): slow's plane A is clamped in place, slow's guides and fast's plane A are read.  There is
// no pack pass and no workspace.  Launch shape (frames/frame_lib.h): one lane per pixel, blockDim (64, 4), so a wave
// is 64 consecutive pixels of one row.  The kernel first stages its workgroup's tile with an apron of R pixels,
// (64 + 2R) x (4 + 2R) cells of three float4 - slow's {n, z}, slow's {P, Lf} with the FAST length in the fourth
// component, and the fast colour demodulated by the cell's own floored albedo, {F, 0} - in LDS (33.6 KB at R = 3), as
// despeckle_clamp_kernel does: every cell is fetched and divided once per workgroup, not once per tap, the up to 49
// taps of a pixel are LDS reads, and a cell outside the image reads as z = 0, so the window needs no bounds test.  The
// radius is a template argument: the window unrolls into straight-line code, the seven running values (m and s1, s2 per
// channel) take "accepted" as a select.  A lane reads and writes its own slow.A_p alone; nothing a tap reads is written.
//
// The arithmetic is the header's contract, operation for operation: built with -ffp-contract=off and without
// fast-math, so + - * / round once each, sqrtf is the correctly rounded one (__builtin_sqrtf, as in csrc/adaptive_kernels.h), and the select forms below
// are the contract's comparisons (a NaN compares false), never fmaxf / fminf.
#include "vimg_rectify.h"

#define FRAME_LIB "rectify"
#include "../frames/frame_lib.h"
#include "../frames/guides.h"
#include "../frames/tile.h"

namespace vimg_rectify {

using namespace vimg_frames;

// one channel's bounds and the clamped value; true when H was outside
__device__ inline bool bounded(float H, float s1, float s2, float fm, float k, float& Hc) {
  const float mean = s1 / fm;
  float v = s2 / fm - mean * mean;
  if (v < 0.f) v = 0.f;
  const float w = k * __builtin_sqrtf(v);
  const float lo = mean - w, hi = mean + w;
  const bool below = H < lo, above = H > hi;
  Hc = below ? lo : above ? hi : H;
  return below || above;
}

template <int R>
__global__ __launch_bounds__(WAVE_X * ROWS) void rectify_clamp_kernel(
    uint32_t w, uint32_t h, uint32_t min_taps, float k, float cut, float sigma_normal, float sigma_plane, float floor,
    float4* slow_a, const float4* __restrict__ slow_g0, const float4* __restrict__ slow_g1, const float4* __restrict__ fast_a,
    const float* __restrict__ albedo, float* __restrict__ out, uint8_t* __restrict__ code) {
  int x, y;
  const bool inside = pixel_of(w, h, x, y);
  // the workgroup's tile with its apron, row-major; a cell outside the image reads as a miss
  constexpr int TW = tile_width<R>;
  __shared__ float4 t0[tile_cells<R>], t1[tile_cells<R>], t2[tile_cells<R>];
  const int lp = stage_tile<R>([&](int i, int gx, int gy) {
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0, v2 = v0;
    if (uint32_t(gx) < w && uint32_t(gy) < h) {
      const size_t q = size_t(gy) * w + size_t(gx);
      v0 = slow_g0[q];
      v1 = slow_g1[q];
      const float4 f = fast_a[q];
      v1.w = f.w;
      v2 = f;
      if (albedo) {
        v2.x = f.x / floored(albedo[3 * q], floor);
        v2.y = f.y / floored(albedo[3 * q + 1], floor);
        v2.z = f.z / floored(albedo[3 * q + 2], floor);
      }
    }
    t0[i] = v0;
    t1[i] = v1;
    t2[i] = v2;
  });
  if (!inside) return;
  const size_t p = size_t(y) * w + size_t(x);
  const float4 np = t0[lp], pp = t1[lp];
  const float4 a = slow_a[p];
  float r = a.x, g = a.y, b = a.z;
  uint8_t what = VIMG_RECTIFY_NOT_LIVE;
  if (np.w > 0.f && a.w > 0.f) {
    const float sz = sigma_plane * np.w;
    const float plane_den = sz * sz;
    float s1r = 0.f, s1g = 0.f, s1b = 0.f, s2r = 0.f, s2g = 0.f, s2b = 0.f;
    uint32_t m = 0;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
      for (int dx = -R; dx <= R; ++dx) {
        const int lq = lp + dy * TW + dx;
        const float4 nq = t0[lq], pq = t1[lq], fq = t2[lq];
        bool ok = nq.w > 0.f && pq.w > 0.f;
        if (dx != 0 || dy != 0) ok = ok && guide_score(np, pp, nq, pq, sigma_normal, plane_den) < 1.f;
        m += ok ? 1u : 0u;
        s1r = ok ? s1r + fq.x : s1r;
        s1g = ok ? s1g + fq.y : s1g;
        s1b = ok ? s1b + fq.z : s1b;
        s2r = ok ? s2r + fq.x * fq.x : s2r;
        s2g = ok ? s2g + fq.y * fq.y : s2g;
        s2b = ok ? s2b + fq.z * fq.z : s2b;
      }
      // an empty statement that "writes" the seven running values: a row of taps is finished before the next begins.
      // Without it the compiler issues the window's LDS reads ahead of the sums: 219 VGPRs at R = 3 (DESIGN.md 4.20's
      // table has what it takes with it)
      asm volatile("" : "+v"(s1r), "+v"(s1g), "+v"(s1b), "+v"(s2r), "+v"(s2g), "+v"(s2b), "+v"(m));
    }
    what = VIMG_RECTIFY_FEW_TAPS;
    if (m >= min_taps) {
      what = VIMG_RECTIFY_KEPT;
      float ar = 1.f, ag = 1.f, ab = 1.f;
      if (albedo) {
        ar = floored(albedo[3 * p], floor);
        ag = floored(albedo[3 * p + 1], floor);
        ab = floored(albedo[3 * p + 2], floor);
      }
      const float fm = float(m);
      float cr, cg, cb;
      const bool mr = bounded(a.x / ar, s1r, s2r, fm, k, cr);
      const bool mg = bounded(a.y / ag, s1g, s2g, fm, k, cg);
      const bool mb = bounded(a.z / ab, s1b, s2b, fm, k, cb);
      if (mr || mg || mb) {
        what = VIMG_RECTIFY_CLAMPED;
        r = cr * ar;
        g = cg * ag;
        b = cb * ab;
        const float Lf = pp.w;
        const float L = Lf > 0.f && a.w > Lf ? a.w - cut * (a.w - Lf) : a.w;
        slow_a[p] = make_float4(r, g, b, L);
      }
    }
  }
  if (out) {
    out[3 * p] = r;
    out[3 * p + 1] = g;
    out[3 * p + 2] = b;
  }
  if (code) code[p] = what;
}

}  // namespace vimg_rectify

using namespace vimg_rectify;

extern "C" {

void vimg_rectify_defaults(VimgRectifyParams* params) {
  if (!params) return;
  params->struct_size = sizeof(VimgRectifyParams);
  params->radius = 1;      // the header's "Defaults": by the sweep of DESIGN.md 4.33
  params->min_taps = 4;
  params->reserved = 0;
  params->k = 1.f;
  params->cut = 1.f;
  params->sigma_normal = 0.5f;
  params->sigma_plane = 0.005f;
  params->albedo_floor = 1.f / 64.f;
}

uint64_t vimg_rectify_workspace(uint32_t, uint32_t) { return 0; }

int vimg_rectify_clamp(const VimgRectifyFrames* f, const VimgRectifyParams* a, void* d_out_rgb, void* d_out_code, void*,
                       uint64_t, void* stream) {
  static_assert(VIMG_RECTIFY_HISTORY_PER_PIXEL == 3 * sizeof(float4), "a history is three float4 planes");
  if (const int rc = check_structs(f, a, "params", VIMG_RECTIFY_MAX_EXTENT)) return rc;
  if (const int rc = check_present({{f->slow, "slow"}, {f->fast, "fast"}}, "history")) return rc;
  const uint32_t w = f->width, h = f->height;
  if (misaligned(f->slow, 16) || misaligned(f->fast, 16))
    return fail(VIMG_E_INVALID, "rectify: the %s history must be 16-byte aligned", misaligned(f->slow, 16) ? "slow" : "fast");
  if (misaligned(f->albedo, 4)) return fail(VIMG_E_INVALID, "rectify: the albedo frame must be 4-byte aligned");
  if (misaligned(d_out_rgb, 4)) return fail(VIMG_E_INVALID, "rectify: the output must be 4-byte aligned");
  if (a->radius < 1 || a->radius > VIMG_RECTIFY_MAX_RADIUS)
    return fail(VIMG_E_INVALID, "rectify: radius must be 1..%u, not %u", VIMG_RECTIFY_MAX_RADIUS, a->radius);
  const uint32_t window = (2 * a->radius + 1) * (2 * a->radius + 1);
  if (a->min_taps < 1 || a->min_taps > window) return fail(VIMG_E_INVALID, "rectify: min_taps must be 1..%u, not %u", window, a->min_taps);
  if (const int rc = check_float("k", a->k, 0.f, false, true)) return rc;
  if (!(a->cut >= 0.f && a->cut <= 1.f)) return fail(VIMG_E_INVALID, "rectify: cut must be 0..1, not %g", double(a->cut));
  if (const int rc = check_float("sigma_normal", a->sigma_normal, 0.f, true, false)) return rc;
  if (const int rc = check_float("sigma_plane", a->sigma_plane, 0.f, true, false)) return rc;
  if (const int rc = check_float("albedo_floor", a->albedo_floor, 0.f, true, false)) return rc;
  // nothing is written where something else is read or written: the slow history against the fast one and the albedo
  // frame, then each output against both histories, the albedo frame and the output before it
  const uint64_t n = uint64_t(w) * h, frame = 12 * n, hist = uint64_t(VIMG_RECTIFY_HISTORY_PER_PIXEL) * n;
  const Range reads[] = {{f->slow, hist, "the slow history"}, {f->fast, hist, "the fast history"}, {f->albedo, frame, "the albedo frame"}};
  if (const Range* r = first_overlap(f->slow, hist, std::span(reads).subspan(1)))
    return fail(VIMG_E_INVALID, "rectify: the slow history overlaps %s", r->name);
  if (const Range* r = d_out_rgb ? first_overlap(d_out_rgb, frame, reads) : nullptr)
    return fail(VIMG_E_INVALID, "rectify: the output overlaps %s", r->name);
  if (const Range* r = d_out_code ? first_overlap(d_out_code, n, reads) : nullptr)
    return fail(VIMG_E_INVALID, "rectify: the output codes overlap %s", r->name);
  if (d_out_rgb && d_out_code && overlaps(d_out_rgb, frame, d_out_code, n))
    return fail(VIMG_E_INVALID, "rectify: the output overlaps the output codes");

  float4* slow = static_cast<float4*>(f->slow);
  const float4* fast = static_cast<const float4*>(f->fast);
  const dim3 block = pixel_block(), grid = pixel_grid(w, h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  clear_stale_error();
  with_radius<VIMG_RECTIFY_MAX_RADIUS>(a->radius, [&](auto R) {
    rectify_clamp_kernel<R.value><<<grid, block, 0, s>>>(w, h, a->min_taps, a->k, a->cut, a->sigma_normal, a->sigma_plane, a->albedo_floor,
                                                         slow, slow + n, slow + 2 * n, fast, static_cast<const float*>(f->albedo),
                                                         static_cast<float*>(d_out_rgb), static_cast<uint8_t*>(d_out_code));
  });
  return launched();
}

const char* vimg_rectify_last_error(void) { return g_error; }

}  // extern "C"
