// libvimg_exposure.so: the histogram auto-exposure of include/vimg_exposure.h.
//
// Three kernels around 1040 bytes of state in the caller's device memory:
//   meter     a capped grid of 256-lane workgroups walks the frame in a grid-stride loop, one lane per pixel and three
//             dword loads per lane as despeckle_pack_kernel reads a pixel.  A workgroup counts into its own uint32[256]
//             in LDS with LDS atomicAdd, and ends by adding its non-zero bins - lane b has bin b - to the state's
//             histogram with global atomicAdd: at most VIMG_EXPOSURE_MAX_WORKGROUPS x 256 of them whatever the frame.
//   resolve   ONE workgroup of 256 lanes, lane b has bin b: it takes its count and leaves a zero, an LDS scan gives the
//             rank of the bin's first pixel and T, a second one in 64 bits gives S, and lane 0 does the scalar arithmetic
//             of the contract and writes the four scalars with ordinary stores.
//   apply     one lane per pixel (frames/frame_lib.h's launch shape): out = c * E', E' read from the state.
// The exposure never visits the host: the three are enqueued back to back and the stream orders them.
//
// The arithmetic is the header's contract, operation for operation: built with -ffp-contract=off and without fast-math,
// so + - * / round once each; the clamps are the contract's comparisons, never fmaxf / fminf; counts are integers, so the
// order in which the atomics arrive changes nothing.
#include "vimg_exposure.h"

#define FRAME_LIB "exposure"
#include "../frames/frame_lib.h"
#include "../frames/guides.h"

namespace vimg_exposure {

using namespace vimg_frames;

constexpr int BINS = int(VIMG_EXPOSURE_BINS);
constexpr int FIRST = 888;      // bits(2^-16) >> 20: the exponent field 111 and three mantissa bits of 0

// the state as the kernels see it: VIMG_EXPOSURE_STATE_BYTES
struct State {
  uint32_t hist[BINS];
  float exposure;
  uint32_t frames;
  float metered;
  uint32_t counted;
};
static_assert(sizeof(State) == VIMG_EXPOSURE_STATE_BYTES && offsetof(State, exposure) == 1024 && offsetof(State, frames) == 1028 &&
                  offsetof(State, metered) == 1032 && offsetof(State, counted) == 1036,
              "the state's layout is the header's");

__device__ inline float edge(int b) { return __uint_as_float(uint32_t(b + FIRST) << 20); }

__global__ __launch_bounds__(BINS) void exposure_meter_kernel(uint64_t n, const float* __restrict__ color,
                                                              const float* __restrict__ depth, uint32_t* __restrict__ hist) {
  __shared__ uint32_t local[BINS];
  local[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t stride = uint64_t(gridDim.x) * BINS;
  for (uint64_t p = uint64_t(blockIdx.x) * BINS + threadIdx.x; p < n; p += stride) {
    const uint64_t t = 3 * p;
    const float L = lum(color[t], color[t + 1], color[t + 2]);
    bool counted = L > 0.f && L < __builtin_huge_valf();
    if (depth) counted = counted && depth[t] > 0.f;
    if (counted) {
      int k = int(__float_as_uint(L) >> 20) - FIRST;
      k = k < 0 ? 0 : k > BINS - 1 ? BINS - 1 : k;
      atomicAdd(&local[k], 1u);
    }
  }
  __syncthreads();
  const uint32_t c = local[threadIdx.x];
  if (c) atomicAdd(&hist[threadIdx.x], c);
}

// inclusive scan of one value per lane over the workgroup's 256 lanes, in place in `s` (Hillis-Steele: eight steps)
template <class T>
__device__ inline T scan256(T* s, T v) {
  const int b = int(threadIdx.x);
  s[b] = v;
  __syncthreads();
#pragma unroll
  for (int d = 1; d < BINS; d *= 2) {
    const T add = b >= d ? s[b - d] : T(0);
    __syncthreads();
    v += add;
    s[b] = v;
    __syncthreads();
  }
  return v;
}

__global__ __launch_bounds__(BINS) void exposure_resolve_kernel(State* __restrict__ state, uint32_t low_permille, uint32_t high_permille,
                                                                float key, float min_exposure, float max_exposure, float rate_brighten,
                                                                float rate_darken) {
  __shared__ uint32_t ranks[BINS];
  __shared__ uint64_t sums[BINS];
  const int b = int(threadIdx.x);
  const uint32_t c = state->hist[b];
  state->hist[b] = 0;
  const uint32_t end = scan256(ranks, c);          // the rank after the bin's last pixel; at most 2^30, the largest frame
  const uint64_t T = ranks[BINS - 1];
  const uint64_t lo = T * low_permille / 1000, hi = T * high_permille / 1000;
  // the bin's ranks [first, end) within [lo, hi)
  const uint64_t first = end - c, from = first > lo ? first : lo, to = end < hi ? end : hi;
  const uint64_t inside = to > from ? to - from : 0;
  scan256(sums, uint64_t(b) * inside);
  if (b != 0) return;
  state->counted = uint32_t(T);
  if (T == 0 || hi == lo) return;
  const uint64_t S = sums[BINS - 1];
  const float m = float(S) / float(hi - lo);
  const int i = int(m);                            // m >= 0: the cast is the floor
  const float f = m - float(i);
  const float e0 = edge(i), e1 = edge(i + 1);
  const float metered = e0 + f * (e1 - e0);
  float target = key / metered;
  target = target < min_exposure ? min_exposure : target;
  target = target > max_exposure ? max_exposure : target;
  const uint32_t frames = state->frames;
  float E = target;
  if (frames != 0) {
    const float was = state->exposure;
    const float rate = target < was ? rate_darken : rate_brighten;
    E = was + (target - was) * rate;
  }
  state->exposure = E;
  state->metered = metered;
  state->frames = frames + 1;
}

// `color` and `out` may be the same buffer: neither is __restrict__, and a lane touches its own pixel of them alone
__global__ __launch_bounds__(WAVE_X * ROWS) void exposure_apply_kernel(uint32_t w, uint32_t h, const float* color,
                                                                       const State* __restrict__ state, float* out) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const float E = state->frames == 0 ? 1.f : state->exposure;
  const size_t t = 3 * (size_t(y) * w + size_t(x));
  const float r = color[t], g = color[t + 1], b = color[t + 2];
  out[t] = r * E;
  out[t + 1] = g * E;
  out[t + 2] = b * E;
}

}  // namespace vimg_exposure

using namespace vimg_exposure;

extern "C" {

void vimg_exposure_defaults(VimgExposureParams* params) {
  if (!params) return;
  params->struct_size = sizeof(VimgExposureParams);
  params->low_permille = 500;      // the header's "Defaults"
  params->high_permille = 950;
  params->key = 0.18f;
  params->min_exposure = 1.f / 64.f;
  params->max_exposure = 64.f;
  params->rate_brighten = 0.25f;
  params->rate_darken = 0.5f;
}

int vimg_exposure_adapt(const VimgExposureFrames* f, const VimgExposureParams* a, void* d_state, void* d_out_rgb, void* stream) {
  if (const int rc = check_structs(f, a, "params", VIMG_EXPOSURE_MAX_EXTENT)) return rc;
  if (const int rc = check_present({{f->color, "color"}})) return rc;
  const uint32_t w = f->width, h = f->height;
  if (!d_state) return fail(VIMG_E_INVALID, "exposure: null state");
  if (misaligned(d_state, 16)) return fail(VIMG_E_INVALID, "exposure: the state must be 16-byte aligned");
  if (a->low_permille >= a->high_permille || a->high_permille > 1000)
    return fail(VIMG_E_INVALID, "exposure: the permilles must be 0 <= low < high <= 1000, not %u and %u", a->low_permille, a->high_permille);
  if (const int rc = check_float("key", a->key, 0.f, true, false)) return rc;
  if (const int rc = check_float("min_exposure", a->min_exposure, 0.f, true, false)) return rc;
  if (const int rc = check_float("max_exposure", a->max_exposure, 0.f, true, false)) return rc;
  if (a->min_exposure > a->max_exposure)
    return fail(VIMG_E_INVALID, "exposure: min_exposure %g is above max_exposure %g", double(a->min_exposure), double(a->max_exposure));
  const float rates[2] = {a->rate_brighten, a->rate_darken};
  const char* rate_names[2] = {"rate_brighten", "rate_darken"};
  for (int i = 0; i < 2; ++i) {
    if (const int rc = check_float(rate_names[i], rates[i], 0.f, true, false)) return rc;
    if (rates[i] > 1.f) return fail(VIMG_E_INVALID, "exposure: %s must be at most 1, not %g", rate_names[i], double(rates[i]));
  }
  // a lane of apply touches its own pixel alone, so the colour frame itself may be the output; nothing else may be
  // written where something is read
  const uint64_t frame = uint64_t(12) * w * h;
  const Range reads[] = {{f->color, frame, "color frame"}, {f->depth, frame, "depth frame"}, {d_state, VIMG_EXPOSURE_STATE_BYTES, "state"}};
  if (d_out_rgb)
    if (const Range* r = first_overlap(d_out_rgb, frame, std::span(reads).subspan(d_out_rgb == f->color ? 1 : 0)))
      return fail(VIMG_E_INVALID, "exposure: the output overlaps the %s%s", r->name, r == reads ? " without being it" : "");
  if (const Range* r = first_overlap(d_state, VIMG_EXPOSURE_STATE_BYTES, std::span(reads).first(2)))
    return fail(VIMG_E_INVALID, "exposure: the state overlaps the %s", r->name);

  const uint64_t n = uint64_t(w) * h;
  const uint64_t wanted = (n + BINS - 1) / BINS;
  const uint32_t groups = uint32_t(wanted < VIMG_EXPOSURE_MAX_WORKGROUPS ? wanted : VIMG_EXPOSURE_MAX_WORKGROUPS);
  hipStream_t s = static_cast<hipStream_t>(stream);
  State* state = static_cast<State*>(d_state);
  const float* color = static_cast<const float*>(f->color);

  clear_stale_error();
  exposure_meter_kernel<<<dim3(groups), dim3(BINS), 0, s>>>(n, color, static_cast<const float*>(f->depth), state->hist);
  if (const int rc = launched("meter")) return rc;
  exposure_resolve_kernel<<<dim3(1), dim3(BINS), 0, s>>>(state, a->low_permille, a->high_permille, a->key, a->min_exposure, a->max_exposure,
                                                         a->rate_brighten, a->rate_darken);
  if (const int rc = launched("resolve")) return rc;
  if (!d_out_rgb) return VIMG_OK;
  exposure_apply_kernel<<<pixel_grid(w, h), pixel_block(), 0, s>>>(w, h, color, state, static_cast<float*>(d_out_rgb));
  return launched("apply");
}

const char* vimg_exposure_last_error(void) { return g_error; }

}  // extern "C"
