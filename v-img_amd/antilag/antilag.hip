// libvimg_antilag.so: the rescaling of a history's lengths of include/vimg_antilag.h.
//
// Two kernels over libvimg_temporal's history of float4 planes [3][h][w] (A {r, g, b, L}, G0 {n, z}, G1 {P, 0}) and one
// plane of float2 in the caller's workspace, {d, v}: the paired luminance difference of a history pixel and the
// current pixel it lands on, and 1 where there is such a pair.
//
// pair: frames/frame_lib.h's launch shape, one lane per HISTORY pixel, blockDim (64, 4), so a wave reads 1 KiB of
// plane A and, where the length is > 0, of the two guide planes, contiguously; the current frame's depth, normal,
// position and colour triples are one gather per lane at the nearest pixel its position projects to; 512 contiguous
// bytes of {d, v} are written per wave.  Built like temporal_accumulate_kernel, in the other direction.
//
// scale: the hot one.  A workgroup of (64, 4) lanes owns a tile of 64 x 16 history pixels.  It stages the tile's {d, v}
// with an apron of R cells, (64 + 2R) x (16 + 2R) float2, in LDS - a cell outside the picture reads as {0, 0} - then
// every lane forms, for its column and the apron's rows ty, ty + 4, ..., the three sums of the (2R + 1) cells of the
// row, columns ascending, and stores them as three planes of 64 floats per row; after a barrier every lane adds up,
// for each of its four pixels, the 2R + 1 row sums of its column, rows ascending.  These ARE the contract's sums, in
// its order, not a reordered reduction: a cell outside the picture adds +0 to a sum that started from +0, and x + 0
// has x's bits for every x such a sum can hold (it is never -0: 0 + -0 = +0), so padding and clipping agree bit for
// bit.  Halo against occupancy: a 64 x 4 tile would stage 6.25 cells per pixel at R = 8 and 3.4 at R = 4, 64 x 16 stages
// 2.5 and 1.7, for 22.8 / 31.5 / 44 KiB of LDS at R = 1 / 4 / 8, 7 / 5 / 3 workgroups per compute unit.  Banks: in the row
// pass consecutive lanes read consecutive float2 of one staged row (ds_read_b64: a 32-lane half covers one 256-byte
// bank row once, and the tap offset moves all lanes alike), and write consecutive floats; in the column pass they
// read consecutive floats of one row: no lane pair of a group meets on a bank.  The radius is a template argument:
// both loops unroll and the LDS is sized for it.
//
// The arithmetic is the header's contract, operation for operation: built with -ffp-contract=off and without
// fast-math, so + - * / round once each, and the select forms below are the contract's comparisons (a NaN compares
// false), never fmaxf / fminf.
#include "vimg_antilag.h"

#define FRAME_LIB "antilag"
#include "../frames/frame_lib.h"
#include "../frames/guides.h"

namespace vimg_antilag {

using namespace vimg_frames;

struct Projection {
  float m[12];     // cur_world_to_pixel, row-major 3 x 4
  float sigma_normal, sigma_plane;
};

struct Thresholds {
  float t_low, t_high, min_matches;
};

__global__ __launch_bounds__(WAVE_X * ROWS) void antilag_pair_kernel(
    uint32_t w, uint32_t h, const float* __restrict__ color, const float* __restrict__ normal,
    const float* __restrict__ position, const float* __restrict__ depth, const float4* __restrict__ hist, Projection k,
    float2* __restrict__ pairs) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t n = size_t(w) * h, q = size_t(y) * w + size_t(x);
  const float4 a = hist[q];
  float d = 0.f, v = 0.f;
  if (a.w > 0.f) {
    const float4 nq = hist[n + q], pq = hist[2 * n + q];
    const float hx = ((k.m[0] * pq.x + k.m[1] * pq.y) + k.m[2] * pq.z) + k.m[3];
    const float hy = ((k.m[4] * pq.x + k.m[5] * pq.y) + k.m[6] * pq.z) + k.m[7];
    const float hw = ((k.m[8] * pq.x + k.m[9] * pq.y) + k.m[10] * pq.z) + k.m[11];
    if (hw > 0.f) {
      const float fx = hx / hw - 0.5f, fy = hy / hw - 0.5f;
      const float cx = floorf(fx + 0.5f), cy = floorf(fy + 0.5f);
      if (cx >= 0.f && cx < float(w) && cy >= 0.f && cy < float(h)) {      // 0 .. w - 1, 0 .. h - 1: exact as int
        const size_t t = 3 * (size_t(int(cy)) * w + size_t(int(cx)));
        if (depth[t] > 0.f) {
          const float dn = 1.f - ((nq.x * normal[t] + nq.y * normal[t + 1]) + nq.z * normal[t + 2]);
          const float ex = position[t] - pq.x, ey = position[t + 1] - pq.y, ez = position[t + 2] - pq.z;
          const float dd = (nq.x * ex + nq.y * ey) + nq.z * ez;
          const float sz = k.sigma_plane * nq.w;
          if (dn < k.sigma_normal && dd * dd < sz * sz) {
            d = lum(color[t], color[t + 1], color[t + 2]) - lum(a.x, a.y, a.z);
            if (d - d == 0.f) v = 1.f;
            else d = 0.f;
          }
        }
      }
    }
  }
  pairs[q] = make_float2(d, v);
}

constexpr int TILE_ROWS = 16;                      // history rows per workgroup of the scale kernel
constexpr int PER_LANE = TILE_ROWS / ROWS;         // pixels per lane: rows ty, ty + 4, ty + 8, ty + 12 of the tile

inline dim3 tile_grid(uint32_t w, uint32_t h) { return dim3((w + WAVE_X - 1) / WAVE_X, (h + TILE_ROWS - 1) / TILE_ROWS); }

template <int R>
__global__ __launch_bounds__(WAVE_X * ROWS) void antilag_scale_kernel(uint32_t w, uint32_t h, const float2* __restrict__ pairs,
                                                                      Thresholds k, float4* __restrict__ hist,
                                                                      float* __restrict__ scale_out) {
  constexpr int TW = WAVE_X + 2 * R, TH = TILE_ROWS + 2 * R;
  __shared__ float2 cell[TH * TW];
  __shared__ float row1[TH * WAVE_X], row2[TH * WAVE_X], row0[TH * WAVE_X];
  const int tx = int(threadIdx.x), ty = int(threadIdx.y);
  const int ox = int(blockIdx.x * WAVE_X) - R, oy = int(blockIdx.y * TILE_ROWS) - R;
  for (int i = ty * WAVE_X + tx; i < TW * TH; i += WAVE_X * ROWS) {
    const int gx = ox + i % TW, gy = oy + i / TW;
    float2 c = make_float2(0.f, 0.f);
    if (uint32_t(gx) < w && uint32_t(gy) < h) c = pairs[size_t(gy) * w + size_t(gx)];
    cell[i] = c;
  }
  __syncthreads();
  for (int r = ty; r < TH; r += ROWS) {
    float s1 = 0.f, s2 = 0.f, s0 = 0.f;
#pragma unroll
    for (int j = 0; j <= 2 * R; ++j) {
      const float2 c = cell[r * TW + tx + j];
      s1 = s1 + c.x;
      s2 = s2 + c.x * c.x;
      s0 = s0 + c.y;
    }
    row1[r * WAVE_X + tx] = s1;
    row2[r * WAVE_X + tx] = s2;
    row0[r * WAVE_X + tx] = s0;
  }
  __syncthreads();
  const int x = int(blockIdx.x * WAVE_X) + tx;
  if (uint32_t(x) >= w) return;
  const float lo = k.t_low * k.t_low, hi = k.t_high * k.t_high;
#pragma unroll
  for (int i = 0; i < PER_LANE; ++i) {
    const int ly = ty + i * ROWS, y = int(blockIdx.y * TILE_ROWS) + ly;
    if (uint32_t(y) >= h) break;
    float sd = 0.f, sq = 0.f, c = 0.f;
#pragma unroll
    for (int j = 0; j <= 2 * R; ++j) {
      const int r = (ly + j) * WAVE_X + tx;
      sd = sd + row1[r];
      sq = sq + row2[r];
      c = c + row0[r];
    }
    float s = 1.f;
    if (c >= k.min_matches) {
      const float m = sd / c;
      float var = (sq - sd * m) / (c - 1.f);
      if (!(var > 0.f)) var = 0.f;
      const float t2 = (m * m) / (var / c);
      if (!(t2 > lo)) s = 1.f;
      else if (!(t2 < hi)) s = 0.f;
      else s = (hi - t2) / (hi - lo);
    }
    const size_t q = size_t(y) * w + size_t(x);
    const float len = hist[q].w;
    if (len > 0.f) hist[q].w = len * s;
    if (scale_out) scale_out[q] = s;
  }
}

}  // namespace vimg_antilag

using namespace vimg_antilag;

extern "C" {

void vimg_antilag_defaults(VimgAntilagParams* params) {
  if (!params) return;
  params->struct_size = sizeof(VimgAntilagParams);
  params->radius = 2;            // the header's "Defaults": the sweep of DESIGN.md 4.26
  params->t_low = 2.f;
  params->t_high = 3.f;
  params->min_matches = 8.f;
  params->sigma_normal = 0.1f;   // libvimg_temporal's (include/vimg_temporal.h, "Defaults")
  params->sigma_plane = 0.00005f;
}

uint64_t vimg_antilag_workspace_bytes(uint32_t width, uint32_t height) {
  return uint64_t(VIMG_ANTILAG_WORKSPACE_PER_PIXEL) * width * height;
}

int vimg_antilag_rescale(const VimgAntilagFrames* f, const float cur_world_to_pixel[12], void* d_history,
                         const VimgAntilagParams* a, void* d_workspace, uint64_t workspace_bytes, void* d_scale_out,
                         void* stream) {
  static_assert(VIMG_ANTILAG_HISTORY_PER_PIXEL == 3 * sizeof(float4), "the history's three float4 planes");
  static_assert(VIMG_ANTILAG_WORKSPACE_PER_PIXEL == sizeof(float2), "the workspace is one float2 plane");
  if (const int rc = check_head(f, a, VIMG_ANTILAG_MAX_EXTENT)) return rc;
  if (a->radius < 1 || a->radius > VIMG_ANTILAG_MAX_RADIUS)
    return fail(VIMG_E_INVALID, "antilag: radius must be 1..%u, not %u", VIMG_ANTILAG_MAX_RADIUS, a->radius);
  if (const int rc = check_float("t_low", a->t_low, 0.f, true, false)) return rc;
  if (const int rc = check_float("t_high", a->t_high, a->t_low, true, false)) return rc;
  if (const int rc = check_float("min_matches", a->min_matches, 2.f, false, false)) return rc;
  if (const int rc = check_float("sigma_normal", a->sigma_normal, 0.f, true, false)) return rc;
  if (const int rc = check_float("sigma_plane", a->sigma_plane, 0.f, true, false)) return rc;
  Projection k{};
  if (!cur_world_to_pixel) return fail(VIMG_E_INVALID, "antilag: null world-to-pixel matrix");
  for (int i = 0; i < 12; ++i) {
    if (!std::isfinite(cur_world_to_pixel[i]))
      return fail(VIMG_E_INVALID, "antilag: world-to-pixel entry %d is not finite (%g)", i, double(cur_world_to_pixel[i]));
    k.m[i] = cur_world_to_pixel[i];
  }
  k.sigma_normal = a->sigma_normal;
  k.sigma_plane = a->sigma_plane;
  if (!d_history) return fail(VIMG_E_INVALID, "antilag: null history");
  if (misaligned(d_history, 16)) return fail(VIMG_E_INVALID, "antilag: the history must be 16-byte aligned");
  const uint32_t w = f->width, h = f->height;
  const uint64_t need = vimg_antilag_workspace_bytes(w, h);
  if (const int rc = check_workspace(d_workspace, workspace_bytes, need, w, h)) return rc;
  if (misaligned(d_scale_out, 4)) return fail(VIMG_E_INVALID, "antilag: the scale output must be 4-byte aligned");
  // the history is written while other lanes read the frames, the workspace between the two kernels, the scales last
  const uint64_t frame = uint64_t(12) * w * h, hist = uint64_t(VIMG_ANTILAG_HISTORY_PER_PIXEL) * w * h, plane = uint64_t(4) * w * h;
  const Range reads[] = {{d_history, hist, "history"}, {f->color, frame, "color frame"}, {f->normal, frame, "normal frame"},
                         {f->position, frame, "position frame"}, {f->depth, frame, "depth frame"}, {d_workspace, need, "workspace"}};
  if (const Range* r = first_overlap(d_history, hist, std::span(reads).subspan(1, 4)))
    return fail(VIMG_E_INVALID, "antilag: the history overlaps the %s", r->name);
  if (const Range* r = first_overlap(d_workspace, need, std::span(reads).first(5)))
    return fail(VIMG_E_INVALID, "antilag: the workspace overlaps the %s", r->name);
  if (const Range* r = d_scale_out ? first_overlap(d_scale_out, plane, reads) : nullptr)
    return fail(VIMG_E_INVALID, "antilag: the scale output overlaps the %s", r->name);

  hipStream_t s = static_cast<hipStream_t>(stream);
  float4* history = static_cast<float4*>(d_history);
  float2* pairs = static_cast<float2*>(d_workspace);
  clear_stale_error();
  antilag_pair_kernel<<<pixel_grid(w, h), pixel_block(), 0, s>>>(
      w, h, static_cast<const float*>(f->color), static_cast<const float*>(f->normal), static_cast<const float*>(f->position),
      static_cast<const float*>(f->depth), history, k, pairs);
  if (const int rc = launched("pair")) return rc;
  const Thresholds t{a->t_low, a->t_high, a->min_matches};
  float* scale = static_cast<float*>(d_scale_out);
  with_radius<VIMG_ANTILAG_MAX_RADIUS>(a->radius, [&](auto R) {
    antilag_scale_kernel<R.value><<<tile_grid(w, h), pixel_block(), 0, s>>>(w, h, pairs, t, history, scale);
  });
  return launched("scale");
}

const char* vimg_antilag_last_error(void) { return g_error; }

}  // extern "C"
