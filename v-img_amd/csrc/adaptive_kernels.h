// Adaptive sampling beside the render kernels (vimg_hip_progressive_render_masked, _state, _error, _select;
// DESIGN.md 4.14): the item list of one count class, the per-pixel statistics, and the pictures read from the
// accumulator's records.  Nothing here samples: the render kernels add the samples, these kernels decide where
// and keep the books.
//
// A pixel's record (32 B, two v4u; twice per accumulator):  {rng lo, rng hi, N, K} {sum.x, sum.y, sum.z, M2}
//   N  samples the pixel has had           K  increments it has taken part in
//   M2 sum of squared deviations of the increments' batch means of luminance, sample-weighted (float32)
// The render kernels write {rng, 0, 0}{sum, 0}; adapt_carry_kernel fills N, K and M2 in afterwards.
#pragma once
#include "device_math.h"
#include "device_scene.h"

namespace vimg {

#define VHD static __host__ __device__ __forceinline__

// ---- the statistic, stated once: plain float32 +, -, *, /, sqrt, no contraction (-ffp-contract=off), in the
// order written.  include/vimg_hip.h states the same expressions for callers.
VHD float adapt_lum(float x, float y, float z) { return x * 0.212671f + y * 0.715160f + z * 0.072169f; }   // lum3 of post_kernels.h
// M2 after an increment of n samples that took the sums from s0 (N samples; ignored when N == 0) to s1
VHD float adapt_m2(float m2, uint32_t N, uint32_t n, const float s0[3], const float s1[3]) {
  const float b = adapt_lum(s1[0] - s0[0], s1[1] - s0[1], s1[2] - s0[2]) / static_cast<float>(n);
  const float m_old = N ? adapt_lum(s0[0], s0[1], s0[2]) / static_cast<float>(N) : 0.0f;
  const float m_new = adapt_lum(s1[0], s1[1], s1[2]) / static_cast<float>(N + n);
  return m2 + static_cast<float>(n) * (b - m_old) * (b - m_new);
}
// estimated relative standard error of the pixel's mean luminance
VHD float adapt_err(uint32_t N, uint32_t K, float m2, const float s[3]) {
  if (K < 2u) return __builtin_huge_valf();
  const float m = adapt_lum(s[0], s[1], s[2]) / static_cast<float>(N);
  const float var = (m2 < 0.0f ? 0.0f : m2) / static_cast<float>(K - 1u) / static_cast<float>(N);
  return __builtin_sqrtf(var) / (__builtin_fabsf(m) + 1e-3f);
}
#undef VHD

// The work items of an accumulator and where each one's pixel lies in the caller's buffers (the order of
// d_out_rgb: the image for tile_world == 1, the compact tile-major buffer of a shard otherwise).
struct AdaptGeom {
  uint32_t items;                 // 64 per tile of the shard
  uint32_t tile_rank, tile_world, tiles_x, tiles_y, W, H;
};
// false for the off-image slots of ragged tiles; `o` = the pixel's index in the caller's order
VD bool adapt_pixel(const AdaptGeom& G, uint32_t item, uint32_t& o) {
  const uint32_t tile = (item >> 6) * G.tile_world + G.tile_rank;
  const uint32_t within = item & 63u;
  const uint32_t tx = tile / G.tiles_y, ty = tile - tx * G.tiles_y;
  const uint32_t px = tx * 8u + (within & 7u), py = ty * 8u + (within >> 3);
  const bool valid = (tx < G.tiles_x) && (px < G.W) && (py < G.H);
  o = (G.tile_world == 1u) ? (valid ? px + (G.H - 1u - py) * G.W : 0u) : item;
  return valid;
}
VD bool adapt_selected(const AdaptGeom& G, const uint8_t* __restrict__ mask, uint32_t item) {
  uint32_t o;
  if (item >= G.items || !adapt_pixel(G, item, o)) return false;
  return mask ? mask[o] != 0 : true;
}

// control words of one call, in the accumulator's scratch
enum : uint32_t { ACTL_CLASS = 0, ACTL_LEN = 1, ACTL_NEXT = 2, ACTL_MAXSEL = 3, ACTL_ACTIVE = 4, ACTL_WORDS = 8 };
constexpr uint32_t ADAPT_BLOCK = 1024;   // items per workgroup of the list kernels (16 waves)

VD uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(v, off); v = o < v ? o : v; }
  return v;
}
VD uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(v, off); v = o > v ? o : v; }
  return v;
}

// Start of a call: the smallest and the largest count among the selected pixels (one atomic per wave).
__global__ void __launch_bounds__(ADAPT_BLOCK)
adapt_first_class_kernel(const AdaptGeom G, const uint8_t* __restrict__ mask, const v4u* __restrict__ rec,
                         uint32_t* __restrict__ ctl) {
  const uint32_t item = blockIdx.x * ADAPT_BLOCK + threadIdx.x;
  const bool sel = adapt_selected(G, mask, item);
  const uint32_t n = sel ? rec[size_t(item) * 2u].z : 0u;
  const uint32_t lo = wave_min_u32(sel ? n : 0xffffffffu), hi = wave_max_u32(n);
  if ((threadIdx.x & 63u) == 0u && lo != 0xffffffffu) {
    atomicMin(&ctl[ACTL_NEXT], lo);
    atomicMax(&ctl[ACTL_MAXSEL], hi);
  }
}
__global__ void adapt_ctl_init_kernel(uint32_t* __restrict__ ctl) {
  if (threadIdx.x < ACTL_WORDS) ctl[threadIdx.x] = threadIdx.x == ACTL_NEXT ? 0xffffffffu : 0u;
}
// Start of a round: the class found by the round before becomes the current one.
__global__ void adapt_round_kernel(uint32_t* __restrict__ ctl) {
  if (threadIdx.x == 0) {
    ctl[ACTL_CLASS] = ctl[ACTL_NEXT];
    ctl[ACTL_NEXT] = 0xffffffffu;
    ctl[ACTL_LEN] = 0u;
  }
}

// The item list of the class ctl[ACTL_CLASS] - the selected items whose count is that class, ascending - in three
// steps: members per workgroup (and the smallest selected count above the class, the next round's), an
// exclusive scan of those numbers by one workgroup, and the scatter, each member at its workgroup's offset +
// the members of the waves before its own + its rank in its wave's ballot.  No atomic orders anything: the same
// mask and counts give the same list.
template <bool SCATTER>
__global__ void __launch_bounds__(ADAPT_BLOCK)
adapt_list_kernel(const AdaptGeom G, const uint8_t* __restrict__ mask, const v4u* __restrict__ rec,
                  uint32_t* __restrict__ ctl, uint32_t* __restrict__ block_counts, uint32_t* __restrict__ item_list) {
  __shared__ uint32_t wave_n[ADAPT_BLOCK / 64];
  const uint32_t item = blockIdx.x * ADAPT_BLOCK + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t cls = ctl[ACTL_CLASS];
  const bool sel = adapt_selected(G, mask, item);
  const uint32_t n = sel ? rec[size_t(item) * 2u].z : 0u;
  const unsigned long long members = __ballot(sel && n == cls);
  if (lane == 0) wave_n[wave] = static_cast<uint32_t>(__popcll(members));
  if constexpr (!SCATTER) {
    const uint32_t above = wave_min_u32((sel && n > cls) ? n : 0xffffffffu);
    if (lane == 0 && above != 0xffffffffu) atomicMin(&ctl[ACTL_NEXT], above);
  }
  __syncthreads();
  if constexpr (!SCATTER) {
    if (threadIdx.x == 0) {
      uint32_t total = 0;
      for (uint32_t w = 0; w < ADAPT_BLOCK / 64; ++w) total += wave_n[w];
      block_counts[blockIdx.x] = total;
    }
  } else {
    if (sel && n == cls) {
      uint32_t at = block_counts[blockIdx.x];   // (exclusive offsets after the scan)
      for (uint32_t w = 0; w < wave; ++w) at += wave_n[w];
      at += static_cast<uint32_t>(__popcll(members & ((1ull << lane) - 1ull)));
      if (at < G.items) item_list[at] = item;   // (never more members than items: the bound only guards the buffer)
    }
  }
}
// counts -> exclusive offsets in place, the total to ctl[ACTL_LEN]; one workgroup
__global__ void __launch_bounds__(ADAPT_BLOCK)
adapt_scan_kernel(uint32_t* __restrict__ block_counts, uint32_t n_blocks, uint32_t* __restrict__ ctl) {
  __shared__ uint32_t wave_tot[ADAPT_BLOCK / 64];
  __shared__ uint32_t carry_s;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0u;
  __syncthreads();
  for (uint32_t base = 0; base < n_blocks; base += ADAPT_BLOCK) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < n_blocks ? block_counts[i] : 0u;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(inc, off);
      if (lane >= uint32_t(off)) inc += o;
    }
    if (lane == 63u) wave_tot[wave] = inc;
    __syncthreads();
    uint32_t before = carry_s;
    for (uint32_t w = 0; w < wave; ++w) before += wave_tot[w];
    if (i < n_blocks) block_counts[i] = before + inc - v;
    __syncthreads();
    if (threadIdx.x == ADAPT_BLOCK - 1u) carry_s = before + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) ctl[ACTL_LEN] = carry_s;
}

// After the launches of a call: a selected item's new record gets its count, its increments and its M2 from the
// old record and the sums the launch left; every other item's record is copied forward.  One pass, 16-byte
// loads and stores.
__global__ void __launch_bounds__(256)
adapt_carry_kernel(const AdaptGeom G, const uint8_t* __restrict__ mask, const v4u* __restrict__ old_rec,
                   v4u* __restrict__ new_rec, uint32_t samples) {
  const uint32_t item = blockIdx.x * 256u + threadIdx.x;
  if (item >= G.items) return;
  const v4u o0 = old_rec[size_t(item) * 2u], o1 = old_rec[size_t(item) * 2u + 1u];
  if (!adapt_selected(G, mask, item)) {
    new_rec[size_t(item) * 2u] = o0;
    new_rec[size_t(item) * 2u + 1u] = o1;
    return;
  }
  const v4u n0 = new_rec[size_t(item) * 2u], n1 = new_rec[size_t(item) * 2u + 1u];
  const uint32_t N = o0.z;   // (a record at N == 0 is all zeros: vimg_hip_progressive_create and _reset wipe them)
  const float s0[3] = {__uint_as_float(o1.x), __uint_as_float(o1.y), __uint_as_float(o1.z)};
  const float s1[3] = {__uint_as_float(n1.x), __uint_as_float(n1.y), __uint_as_float(n1.z)};
  const float m2 = adapt_m2(__uint_as_float(o1.w), N, samples, s0, s1);
  new_rec[size_t(item) * 2u] = v4u{n0.x, n0.y, N + samples, o0.w + 1u};
  new_rec[size_t(item) * 2u + 1u] = v4u{n1.x, n1.y, n1.z, __float_as_uint(m2)};
}

// The pictures of the current records, each optional: the means (sum / float(N), the render kernels' division;
// 0 0 0 at N == 0), the error, and the mask of vimg_hip_progressive_select with its number of ones (one atomic
// per wave).  Off-image slots of a shard's ragged tiles: means untouched (as the render kernels leave them),
// error 0, mask 0.
__global__ void __launch_bounds__(256)
adapt_resolve_kernel(const AdaptGeom G, const v4u* __restrict__ rec, float* __restrict__ out_rgb,
                     float* __restrict__ err_out, uint8_t* __restrict__ mask_out, float target, uint32_t max_samples,
                     uint32_t* __restrict__ ctl) {
  const uint32_t item = blockIdx.x * 256u + threadIdx.x;
  uint32_t o = 0;
  const bool in_range = item < G.items;
  const bool valid = in_range && adapt_pixel(G, item, o);
  bool active = false;
  if (valid) {
    const v4u r0 = rec[size_t(item) * 2u], r1 = rec[size_t(item) * 2u + 1u];
    const uint32_t N = r0.z, K = r0.w;
    const f3 sum{__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z)};
    if (out_rgb) {
      const f3 mean = N ? sum / static_cast<float>(N) : f3{0.f, 0.f, 0.f};
      out_rgb[size_t(o) * 3u + 0u] = mean.x;
      out_rgb[size_t(o) * 3u + 1u] = mean.y;
      out_rgb[size_t(o) * 3u + 2u] = mean.z;
    }
    if (err_out || mask_out) {
      const float s[3] = {sum.x, sum.y, sum.z};
      const float e = adapt_err(N, K, __uint_as_float(r1.w), s);
      if (err_out) err_out[o] = e;
      active = (e > target && N < max_samples) || K < 2u;
      if (mask_out) mask_out[o] = active ? 1 : 0;
    }
  } else if (in_range && G.tile_world != 1u) {
    if (err_out) err_out[o] = 0.f;
    if (mask_out) mask_out[o] = 0;
  }
  if (mask_out) {
    const unsigned long long ones = __ballot(active);
    if ((threadIdx.x & 63u) == 0u && ones != 0ull) atomicAdd(&ctl[ACTL_ACTIVE], static_cast<uint32_t>(__popcll(ones)));
  }
}

// vimg_hip_progressive_state: the records' fields in the caller's pixel order, each optional
__global__ void __launch_bounds__(256)
adapt_state_kernel(const AdaptGeom G, const v4u* __restrict__ rec, float* __restrict__ sum_rgb,
                   uint32_t* __restrict__ count, uint32_t* __restrict__ batches, float* __restrict__ m2) {
  const uint32_t item = blockIdx.x * 256u + threadIdx.x;
  if (item >= G.items) return;
  uint32_t o;
  const bool valid = adapt_pixel(G, item, o);
  if (!valid && G.tile_world == 1u) return;   // no pixel, no place in the image
  const v4u r0 = rec[size_t(item) * 2u], r1 = rec[size_t(item) * 2u + 1u];
  if (sum_rgb) {
    sum_rgb[size_t(o) * 3u + 0u] = valid ? __uint_as_float(r1.x) : 0.f;
    sum_rgb[size_t(o) * 3u + 1u] = valid ? __uint_as_float(r1.y) : 0.f;
    sum_rgb[size_t(o) * 3u + 2u] = valid ? __uint_as_float(r1.z) : 0.f;
  }
  if (count) count[o] = valid ? r0.z : 0u;
  if (batches) batches[o] = valid ? r0.w : 0u;
  if (m2) m2[o] = valid ? __uint_as_float(r1.w) : 0.f;
}

}  // namespace vimg
