// libvimg_demand.so: the sampling mask of a sparse preview of include/vimg_demand.h.
//
// One kernel over libvimg_temporal's history of three float4 planes [3][h][w] (A = {r, g, b, L}, G0 = {n, z},
// G1 = {P, 0}), which it only reads.  The reprojection is frames/reproject.h's and the launch shape
// frames/frame_lib.h's, as in wtemporal/wtemporal.hip: one lane per pixel, blockDim (64, 4), so a wave is 64
// consecutive pixels of one row.  The current frame's reads (packed triples) and both writes are contiguous per wave -
// the mask is 64 contiguous bytes per wave, the lengths 256; the up to four history taps are wtemporal's gathers.  No
// lane leaves before the end: the four counters are reduced per wave with a ballot and a population count, per
// workgroup in 64 bytes of LDS, and lanes 0..3 of the workgroup's first wave add the workgroup's sums to the caller's
// four words with one atomic add each, whose result nobody reads.  The words are cleared on the stream before the kernel.
//
// The arithmetic is the header's contract, operation for operation: built with -ffp-contract=off and without
// fast-math, so + - * / round once each, and every choice is a comparison (a NaN compares false).
#include "vimg_demand.h"

#define FRAME_LIB "demand"
#include "../frames/frame_lib.h"
#include "../frames/reproject.h"

namespace vimg_demand {

using namespace vimg_frames;

constexpr int COUNTS = int(VIMG_DEMAND_COUNTS);

struct Constants {
  Reprojection r;
  uint32_t stride, cx, cy;      // stride 0: no lattice
  float min_history;
};

__global__ __launch_bounds__(WAVE_X * ROWS) void demand_mask_kernel(
    uint32_t w, uint32_t h, const float* __restrict__ normal, const float* __restrict__ position, const float* __restrict__ depth,
    const float4* __restrict__ prev, Constants k, uint8_t* __restrict__ mask, float* __restrict__ length, uint32_t* __restrict__ counts) {
  __shared__ uint32_t part[ROWS][COUNTS];
  int x, y;
  const bool inside = pixel_of(w, h, x, y);
  bool live = false, lat = false, need = false;
  if (inside) {
    const size_t p = size_t(y) * w + size_t(x), t = 3 * p;
    const float z = depth[t];
    live = z > 0.f;
    lat = k.stride != 0 && uint32_t(x) % k.stride == k.cx && uint32_t(y) % k.stride == k.cy;
    float L = 0.f;
    if (live) {
      const float nx = normal[t], ny = normal[t + 1], nz = normal[t + 2];
      const float px = position[t], py = position[t + 1], pz = position[t + 2];
      Reprojected hst;
      if (reproject(w, h, prev, k.r, nx, ny, nz, px, py, pz, z, hst, [](float, size_t) {})) L = hst.len;
    }
    need = live && L < k.min_history;
    mask[p] = lat || need ? 1 : 0;
    if (length) length[p] = L;
  }
  if (!counts) return;          // (a kernel argument: the whole grid leaves or stays)
  // a wave is one row of the workgroup: its four ballots, counted, by its first lane
  const bool what[COUNTS] = {lat || need, need, need && !lat, live};
#pragma unroll
  for (int c = 0; c < COUNTS; ++c) {
    const uint32_t n = uint32_t(__popcll(__ballot(what[c])));
    if (threadIdx.x == 0) part[threadIdx.y][c] = n;
  }
  __syncthreads();
  if (threadIdx.y == 0 && threadIdx.x < COUNTS) {
    uint32_t sum = 0;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) sum += part[r][threadIdx.x];
    if (sum) atomicAdd(&counts[threadIdx.x], sum);
  }
}

}  // namespace vimg_demand

using namespace vimg_demand;

extern "C" {

void vimg_demand_defaults(VimgDemandParams* params) {
  if (!params) return;
  params->struct_size = sizeof(VimgDemandParams);
  params->stride = 2;              // the header's "Defaults"
  params->phase = 0;
  params->reserved = 0;
  params->min_history = 1.f;
  params->sigma_normal = 0.1f;     // libvimg_temporal's (include/vimg_temporal.h, "Defaults")
  params->sigma_plane = 0.00005f;
}

int vimg_demand_mask(const VimgDemandFrames* f, const void* d_prev_history, const float prev_world_to_pixel[12],
                     const VimgDemandParams* a, void* d_out_mask, void* d_out_length, void* d_out_counts, void* stream) {
  static_assert(VIMG_DEMAND_HISTORY_PER_PIXEL == 3 * sizeof(float4), "the history is three float4 planes");
  if (const int rc = check_structs(f, a, "params", VIMG_DEMAND_MAX_EXTENT)) return rc;
  if (const int rc = check_present({{f->normal, "normal"}, {f->position, "position"}, {f->depth, "depth"}})) return rc;
  const uint32_t w = f->width, h = f->height;
  if (!d_out_mask) return fail(VIMG_E_INVALID, "demand: null mask");
  if (a->stride == 1 || a->stride > VIMG_DEMAND_MAX_STRIDE)
    return fail(VIMG_E_INVALID, "demand: stride must be 0 or 2..%u, not %u", VIMG_DEMAND_MAX_STRIDE, a->stride);
  if (a->stride == 0 ? a->phase != 0 : a->phase >= a->stride * a->stride) {
    if (a->stride == 0) return fail(VIMG_E_INVALID, "demand: phase must be 0 at stride 0, not %u", a->phase);
    return fail(VIMG_E_INVALID, "demand: phase must be 0..%u at stride %u, not %u", a->stride * a->stride - 1, a->stride, a->phase);
  }
  if (const int rc = check_float("min_history", a->min_history, 0.f, false, false)) return rc;
  if (const int rc = check_float("sigma_normal", a->sigma_normal, 0.f, true, false)) return rc;
  if (const int rc = check_float("sigma_plane", a->sigma_plane, 0.f, true, false)) return rc;
  Constants k{};
  if (const int rc = check_previous(d_prev_history, prev_world_to_pixel, k.r)) return rc;
  if (misaligned(d_out_length, 4)) return fail(VIMG_E_INVALID, "demand: the output lengths must be 4-byte aligned");
  if (misaligned(d_out_counts, 4)) return fail(VIMG_E_INVALID, "demand: the output counts must be 4-byte aligned");
  // nothing is written where something is read or where something else is written: outputs in the order mask, lengths,
  // counts, each against the history, the guides and the outputs before it
  const uint64_t n = uint64_t(w) * h, frame = 12 * n, hist = uint64_t(VIMG_DEMAND_HISTORY_PER_PIXEL) * n;
  const Range reads[] = {{d_prev_history, hist, "the previous history"}, {f->normal, frame, "the normal frame"},
                         {f->position, frame, "the position frame"}, {f->depth, frame, "the depth frame"}};
  const Range outs[] = {{d_out_mask, n, "mask"}, {d_out_length, 4 * n, "output lengths"}, {d_out_counts, 4 * COUNTS, "output counts"}};
  for (int o = 0; o < 3; ++o) {
    if (!outs[o].p) continue;
    if (const Range* r = first_overlap(outs[o].p, outs[o].bytes, reads))
      return fail(VIMG_E_INVALID, "demand: the %s overlap%s %s", outs[o].name, o == 0 ? "s" : "", r->name);
    if (const Range* e = first_overlap(outs[o].p, outs[o].bytes, std::span(outs).first(o)))
      return fail(VIMG_E_INVALID, "demand: the %s overlap the %s", outs[o].name, e->name);
  }

  if (a->stride) {
    k.stride = a->stride;
    k.cx = a->phase % a->stride;
    k.cy = (a->phase / a->stride + a->phase % a->stride) % a->stride;
  }
  k.min_history = a->min_history;
  k.r.sigma_normal = a->sigma_normal;
  k.r.sigma_plane = a->sigma_plane;
  hipStream_t s = static_cast<hipStream_t>(stream);

  clear_stale_error();
  if (d_out_counts) {
    const hipError_t e = hipMemsetAsync(d_out_counts, 0, 4 * COUNTS, s);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(VIMG_E_DEVICE, "demand: clear launch failed: %s", hipGetErrorString(e));
    }
  }
  demand_mask_kernel<<<pixel_grid(w, h), pixel_block(), 0, s>>>(
      w, h, static_cast<const float*>(f->normal), static_cast<const float*>(f->position), static_cast<const float*>(f->depth),
      static_cast<const float4*>(d_prev_history), k, static_cast<uint8_t*>(d_out_mask), static_cast<float*>(d_out_length),
      static_cast<uint32_t*>(d_out_counts));
  return launched();
}

const char* vimg_demand_last_error(void) { return g_error; }

}  // extern "C"
