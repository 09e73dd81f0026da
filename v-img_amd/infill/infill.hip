// libvimg_infill.so: the reconstruction of sparsely sampled frames of include/vimg_infill.h.
//
// Two kernels - pack, fill - over three planes of float4 in the caller's workspace:
//   C    {C.r, C.g, C.b, sampled}    the demodulated colour; 1 where the pixel has samples, else 0
//   G0   {n.x, n.y, n.z, z}          (z > 0: the pixel is live)
//   G1   {P.x, P.y, P.z, 0}
// Launch shape (frames/frame_lib.h): one lane per pixel, blockDim (64, 4), so a wave is 64 consecutive pixels of one
// row.  The fill kernel first stages its workgroup's tile of the three planes with an apron of R pixels,
// (64 + 2R) x (4 + 2R) float4 each, in LDS (41.5 KB at R = 4) - contiguous 1 KiB requests per wave - so the up to 81
// taps of a pixel are LDS reads and every plane value is fetched once per workgroup, not once per tap; a cell outside
// the image reads as "not sampled", so the window needs no bounds test.  Measured against reading the taps from the
// planes directly, the same bits: 0.072 against 0.093 ms at 1800 x 800 and radius 2.  A sampled pixel
// returns after its copy; an unsampled one walks the (2R + 1)^2 window once, reads plane C of every tap and the guide
// planes of the sampled ones only, and keeps both pairs of sums - the guided one and the unguided fallback - as it
// goes, each in tap order.  The radius is a template argument: the window unrolls and the tent weights are literals.
//
// The arithmetic is the header's contract, operation for operation: built with -ffp-contract=off and without
// fast-math, so + - * / round once each, and the select forms below are the contract's comparisons (a NaN compares
// false), never fmaxf / fminf.
#include "vimg_infill.h"

#define FRAME_LIB "infill"
#include "../frames/frame_lib.h"
#include "../frames/guides.h"

namespace vimg_infill {

using namespace vimg_frames;

__global__ __launch_bounds__(WAVE_X * ROWS) void infill_pack_kernel(
    uint32_t w, uint32_t h, const float* __restrict__ color, const float* __restrict__ normal,
    const float* __restrict__ position, const float* __restrict__ depth, const float* __restrict__ albedo,
    const uint32_t* __restrict__ count, float floor, float4* __restrict__ c, float4* __restrict__ g0, float4* __restrict__ g1) {
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
  c[p] = make_float4(r, g, b, count[p] > 0u ? 1.f : 0.f);
  g0[p] = make_float4(normal[t], normal[t + 1], normal[t + 2], z);
  g1[p] = make_float4(position[t], position[t + 1], position[t + 2], 0.f);
}

// the sums of one unsampled pixel: guided (taps of p's own kind) and unguided (every sampled tap)
struct Sums {
  float gw = 0.f, gr = 0.f, gg = 0.f, gb = 0.f;
  float fw = 0.f, fr = 0.f, fg = 0.f, fb = 0.f;
};

// one sampled tap inside the image: k its tent weight, cq / nq / pq its three planes
__device__ inline void add_tap(Sums& s, float k, bool live, const float4& np, const float4& pp, float sigma_normal,
                               float plane_den, const float4& cq, const float4& nq, const float4& pq) {
  s.fw = s.fw + k;
  s.fr = s.fr + k * cq.x;
  s.fg = s.fg + k * cq.y;
  s.fb = s.fb + k * cq.z;
  const bool live_q = nq.w > 0.f;
  if (live_q != live) return;
  float wq = k;
  if (live) {
    const float S = guide_score(np, pp, nq, pq, sigma_normal, plane_den);
    const float one_s = 1.f - S;
    wq = S < 1.f ? k * (one_s * one_s) : 0.f;
  }
  if (wq > 0.f) {
    s.gw = s.gw + wq;
    s.gr = s.gr + wq * cq.x;
    s.gg = s.gg + wq * cq.y;
    s.gb = s.gb + wq * cq.z;
  }
}

// `color` and `out` may be the same buffer: neither is __restrict__, and a lane touches its own pixel of them alone
template <int R>
__global__ __launch_bounds__(WAVE_X * ROWS) void infill_fill_kernel(
    uint32_t w, uint32_t h, float sigma_normal, float sigma_plane, float floor, const float* color,
    const float* __restrict__ albedo, const float4* __restrict__ c, const float4* __restrict__ g0,
    const float4* __restrict__ g1, float* out, uint8_t* __restrict__ code) {
  int x, y;
  const bool inside = pixel_of(w, h, x, y);
  // the workgroup's tile with its apron, row-major; a cell outside the image reads as "not sampled"
  // (its own loop, not frames/tile.h's stage_tile: through that the staging loads came out in another order and the
  // reconstruct call 0.2 - 0.7 us slower at stride 4, outside the parent's own spread)
  constexpr int TW = WAVE_X + 2 * R, TH = ROWS + 2 * R;
  __shared__ float4 tc[TH * TW], t0[TH * TW], t1[TH * TW];
  const int ox = int(blockIdx.x * WAVE_X) - R, oy = int(blockIdx.y * ROWS) - R;
  for (int i = int(threadIdx.y) * WAVE_X + int(threadIdx.x); i < TW * TH; i += WAVE_X * ROWS) {
    const int gx = ox + i % TW, gy = oy + i / TW;
    float4 vc = make_float4(0.f, 0.f, 0.f, 0.f), v0 = vc, v1 = vc;
    if (uint32_t(gx) < w && uint32_t(gy) < h) {
      const size_t q = size_t(gy) * w + size_t(gx);
      vc = c[q];
      v0 = g0[q];
      v1 = g1[q];
    }
    tc[i] = vc;
    t0[i] = v0;
    t1[i] = v1;
  }
  __syncthreads();
  if (!inside) return;
  const size_t p = size_t(y) * w + size_t(x), t = 3 * p;
  const int lp = (int(threadIdx.y) + R) * TW + int(threadIdx.x) + R;
  const float4 cp = tc[lp];
  if (cp.w > 0.f) {      // sampled: the colour's own bits
    const float r = color[t], g = color[t + 1], b = color[t + 2];
    out[t] = r;
    out[t + 1] = g;
    out[t + 2] = b;
    if (code) code[p] = VIMG_INFILL_SAMPLED;
    return;
  }
  const float4 np = t0[lp], pp = t1[lp];
  const bool live = np.w > 0.f;
  const float sz = sigma_plane * np.w;
  const float plane_den = sz * sz;
  Sums s;
#pragma unroll
  for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      const float k = float((R + 1 - (dx < 0 ? -dx : dx)) * (R + 1 - (dy < 0 ? -dy : dy)));
      const int lq = lp + dy * TW + dx;
      const float4 cq = tc[lq];
      if (!(cq.w > 0.f)) continue;
      add_tap(s, k, live, np, pp, sigma_normal, plane_den, cq, t0[lq], t1[lq]);
    }
  }
  float r = 0.f, g = 0.f, b = 0.f;
  uint8_t what = VIMG_INFILL_HOLE;
  if (s.gw > 0.f) {
    r = s.gr / s.gw;
    g = s.gg / s.gw;
    b = s.gb / s.gw;
    what = VIMG_INFILL_GUIDED;
  } else if (s.fw > 0.f) {
    r = s.fr / s.fw;
    g = s.fg / s.fw;
    b = s.fb / s.fw;
    what = VIMG_INFILL_UNGUIDED;
  }
  if (albedo && live) {
    r = r * floored(albedo[t], floor);
    g = g * floored(albedo[t + 1], floor);
    b = b * floored(albedo[t + 2], floor);
  }
  out[t] = r;
  out[t + 1] = g;
  out[t + 2] = b;
  if (code) code[p] = what;
}

}  // namespace vimg_infill

using namespace vimg_infill;

extern "C" {

void vimg_infill_defaults(VimgInfillParams* params) {
  if (!params) return;
  params->struct_size = sizeof(VimgInfillParams);
  params->radius = 2;      // the header's "Defaults": sigma_normal by the sweep of DESIGN.md 4.23
  params->sigma_normal = 1.f;
  params->sigma_plane = 0.005f;
  params->albedo_floor = 1.f / 64.f;
}

uint64_t vimg_infill_workspace(uint32_t width, uint32_t height) {
  return uint64_t(VIMG_INFILL_WORKSPACE_PER_PIXEL) * width * height;
}

int vimg_infill_reconstruct(const VimgInfillFrames* f, const VimgInfillParams* a, void* d_out_rgb, void* d_out_code,
                            void* d_workspace, uint64_t workspace_bytes, void* stream) {
  if (const int rc = check_head(f, a, VIMG_INFILL_MAX_EXTENT)) return rc;
  if (!f->count) return fail(VIMG_E_INVALID, "infill: null count frame");
  if (!d_out_rgb) return fail(VIMG_E_INVALID, "infill: null output");
  if (a->radius < 1 || a->radius > VIMG_INFILL_MAX_RADIUS)
    return fail(VIMG_E_INVALID, "infill: radius must be 1..%u, not %u", VIMG_INFILL_MAX_RADIUS, a->radius);
  if (const int rc = check_float("sigma_normal", a->sigma_normal, 0.f, true, false)) return rc;
  if (const int rc = check_float("sigma_plane", a->sigma_plane, 0.f, true, false)) return rc;
  if (const int rc = check_float("albedo_floor", a->albedo_floor, 0.f, true, false)) return rc;
  const uint32_t w = f->width, h = f->height;
  const uint64_t need = vimg_infill_workspace(w, h);
  if (const int rc = check_workspace(d_workspace, workspace_bytes, need, w, h)) return rc;
  // other lanes read the planes, and pack reads every frame before fill writes: only the colour frame itself may be
  // the output
  const uint64_t frame = uint64_t(12) * w * h, plane = uint64_t(4) * w * h, codes = uint64_t(w) * h;
  const Range others[] = {{f->color, frame, "color frame"}, {f->normal, frame, "normal frame"}, {f->position, frame, "position frame"},
                          {f->depth, frame, "depth frame"}, {f->albedo, frame, "albedo frame"}, {f->count, plane, "count frame"},
                          {d_out_code, codes, "output codes"}, {d_workspace, need, "workspace"}};
  if (const Range* r = first_overlap(d_out_rgb, frame, std::span(others).subspan(d_out_rgb == f->color ? 1 : 0)))
    return fail(VIMG_E_INVALID, "infill: the output overlaps the %s%s", r->name, r == others ? " without being it" : "");
  if (d_out_code && overlaps(d_out_code, codes, d_workspace, need))
    return fail(VIMG_E_INVALID, "infill: the output codes overlap the workspace");

  const size_t n = size_t(w) * h;
  float4* c = static_cast<float4*>(d_workspace);
  float4 *g0 = c + n, *g1 = c + 2 * n;
  const dim3 block = pixel_block(), grid = pixel_grid(w, h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* color = static_cast<const float*>(f->color);
  const float* albedo = static_cast<const float*>(f->albedo);

  clear_stale_error();
  infill_pack_kernel<<<grid, block, 0, s>>>(w, h, color, static_cast<const float*>(f->normal),
                                            static_cast<const float*>(f->position), static_cast<const float*>(f->depth), albedo,
                                            static_cast<const uint32_t*>(f->count), a->albedo_floor, c, g0, g1);
  if (const int rc = launched("pack")) return rc;
  float* out = static_cast<float*>(d_out_rgb);
  uint8_t* code = static_cast<uint8_t*>(d_out_code);
  with_radius<VIMG_INFILL_MAX_RADIUS>(a->radius, [&](auto R) {
    infill_fill_kernel<R.value><<<grid, block, 0, s>>>(w, h, a->sigma_normal, a->sigma_plane, a->albedo_floor, color, albedo, c, g0, g1,
                                                       out, code);
  });
  return launched("fill");
}

const char* vimg_infill_last_error(void) { return g_error; }

}  // extern "C"
