// The first-hit feature integrators (include/vimg_scene.h: VIMG_INTEGRATOR_ALBEDO .. _COVERAGE):
// what a denoiser or compositor wants beside the noisy image, as frames of the render's own shapes.
//
// A kernel of its own, so that nothing of render_kernel or render_cu_kernel moves.  Its sample loop is the normal
// integrators' (reference src/integrators/normals.cpp, restated in render_kernel's camera-ray block): the
// pixel's PCG stream seeded with the image index, the jitter random_x_y_r2(px + py + sample_base + k), rand2
// drawn before rand1, generate_ray, ONE traverse<false> over [1e-4, inf), make_hit_info.  The camera rays are
// therefore those of s_normal, and of vimg_hip_camera_rays + vimg_hip_trace_rays given the same samples: the hit
// record is made with make_hit_info<true>, as the queries make it, so uv exists on every material.
//
// Shape: the lane-bound kernel's.  256 threads, the lane launch's LDS layout (stage_lds: the top of the tree,
// then a stack per lane), a persistent grid whose waves claim 64 work items at a time from the launch's counter
// (one 8x8 tile of an ordinary launch, so a wave's rays start coherent), one lane per pixel, the samples of a
// pixel in order in that lane - the float32 sum is in sample order by construction - and one division at the
// end.  RenderArgs is read as render_kernel reads it: item_list / item_count, single_x / single_y, sample_base /
// prog_in / prog_out, the tile arithmetic; depth and the scheduler options are not read.
#pragma once
#include "render_kernels.h"

namespace vimg {

// The value of one sample that hit something.  Albedo (include/vimg_hip.h has the rule per material): the base
// colour texture of Lambertian and Principled through col_at_ray_hit, with the primary ray's direction and the
// cone the MIS integrator's first vertex evaluates its textures with - the camera's cone {0, cone_spread} carried
// to the hit by propagate_reflect_cone (render_kernel: nee_cone, which is also the cone of the sampled direction
// where the vertex does not refract).
template <bool TEX>
VD f3 feature_value(const DScene& g, uint32_t integrator, const Hit& hit, f3 ray_o, f3 ray_d, float t) {
  switch (integrator) {
    case VIMG_INTEGRATOR_NORMAL: return hit.ns;
    case VIMG_INTEGRATOR_DEPTH: return f3{t, t, t};
    case VIMG_INTEGRATOR_POSITION: return hit.p;
    case VIMG_INTEGRATOR_UV: return f3{hit.uv.x, hit.uv.y, 0.f};
    case VIMG_INTEGRATOR_COVERAGE: return f3{1.f, 1.f, 1.f};
    default: break;
  }
  gptr<VimgMaterial> m = g.materials + hit.mat;
  const uint32_t type = m->type;
  if (type == VIMG_MAT_DIELECTRIC) return f3{1.f, 1.f, 1.f};
  if (type == VIMG_MAT_DIFFUSE_LIGHT) return load3(m->emit);
  RayCone cone{0.f, g.cone_spread};
  if constexpr (TEX) {
    const float hit_dist = length(ray_o - hit.p);
    const float ssa = spread_angle_from_curvature(hit.curvature, cone.cone_width, ray_d, hit.ns);
    cone = propagate_reflect_cone(cone, ssa * 2.f, hit_dist);
  }
  return col_at_ray_hit<TEX>(g, m->tex, ray_d, cone, hit);
}

template <bool TEX>
__global__ void __launch_bounds__(256)
feature_kernel(const DScene g, const RenderArgs A, float* __restrict__ out, DeviceStats* __restrict__ stats,
               unsigned int* __restrict__ work_counter) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const Lds L = stage_lds(g, A, (VIMG_LDS unsigned char*)lds_raw);
  const uint32_t lane = threadIdx.x & 63;
  const bool full_stats = A.full_stats != 0;
  const uint32_t W = static_cast<uint32_t>(g.res_x), H = static_cast<uint32_t>(g.res_y);
  const bool single = A.single_x >= 0;
  const uint32_t total_items = single ? 1u : (A.item_list ? A.item_count : A.num_local_tiles * 64u);
  Counters cnt{0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t nan_samples = 0;

  for (;;) {
    // ---- a wave's claim: 64 consecutive entries of the launch's work list
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(work_counter, 64u);
    base = __shfl(base, 0);
    if (base >= total_items) break;
    uint32_t item = base + lane;
    bool valid = item < total_items;
    uint32_t px = 0, py = 0;
    if (valid) {
      if (A.item_list) item = A.item_list[item];   // a masked launch: the claim names an entry of its list
      if (single) {
        px = static_cast<uint32_t>(A.single_x), py = static_cast<uint32_t>(A.single_y);
      } else {
        // 8x8 tiles in the reference's x-major work_list order; shard r of n owns tiles t with t % n == r
        const uint32_t tile = (item >> 6) * A.tile_world + A.tile_rank;
        const uint32_t within = item & 63u;
        const uint32_t tx = tile / A.tiles_y, ty = tile - tx * A.tiles_y;
        px = tx * 8 + (within & 7u);
        py = ty * 8 + (within >> 3);
        valid = (tx < A.tiles_x) && (px < W) && (py < H);
      }
    }
    if (valid) {   // (no wave-wide operation inside: traverse's votes are among the lanes that call it)
      Rng rng{0};
      f3 acc{0.f, 0.f, 0.f};
      if (A.sample_base == 0u) {
        pcg_seed(rng, uint64_t(px) + uint64_t(H - 1 - py) * W);
      } else {   // a progressive launch after the first: the pixel goes on from its record
        const v4u r0 = A.prog_in[size_t(item) * 2u], r1 = A.prog_in[size_t(item) * 2u + 1u];
        rng.s = uint64_t(r0.x) | (uint64_t(r0.y) << 32);
        acc = f3{__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z)};
      }
#pragma unroll 1
      for (uint32_t smp = 0; smp < A.samples; ++smp) {
        const f2 off = random_x_y_r2(px + py + A.sample_base + smp);
        const float rand2 = rand_float(rng);   // (the reference's call evaluates its arguments right to left)
        const float rand1 = rand_float(rng);
        f3 ray_o, ray_d;
        generate_ray(g, static_cast<float>(px) + off.x, static_cast<float>(py) + off.y, rand1, rand2, ray_o, ray_d);
        TravRay tr{ray_o, ray_d, 0.0001f, VIMG_INF};
        HitRec rec;
        cnt.closest++;
        f3 result{0.f, 0.f, 0.f};
        if (traverse<false>(g, L, tr, rec, cnt, full_stats)) {
          Hit hit;
          make_hit_info<true>(g, rec, tr, hit);
          result = feature_value<TEX>(g, A.integrator, hit, ray_o, ray_d, tr.max_t);
        }
        if (is_nan(result.x) || is_nan(result.y) || is_nan(result.z)) nan_samples++;
        acc = acc + result;
      }
      const f3 px_col = acc / A.spp_div;
      if (A.prog_out) {   // progressive launch: the pixel rests in its record until the next increment
        A.prog_out[size_t(item) * 2u] = v4u{static_cast<uint32_t>(rng.s), static_cast<uint32_t>(rng.s >> 32), 0u, 0u};
        A.prog_out[size_t(item) * 2u + 1u] = v4u{__float_as_uint(acc.x), __float_as_uint(acc.y), __float_as_uint(acc.z), 0u};
      }
      const size_t o = single ? 0 : (A.tile_world == 1 ? (size_t(px) + size_t(H - 1 - py) * W) * 3 : size_t(item) * 3);
      out[o + 0] = px_col.x;
      out[o + 1] = px_col.y;
      out[o + 2] = px_col.z;
    }
  }

  // ---- flush event counts: one atomic per wave and counter
  if (stats) {
    auto wave_sum = [&](uint32_t v) {
      unsigned long long s = v;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
      return s;
    };
    const unsigned long long c0 = wave_sum(cnt.closest), c2 = wave_sum(cnt.internal), c3 = wave_sum(cnt.leaf),
                             c4 = wave_sum(cnt.prim), c5 = wave_sum(nan_samples), c6 = wave_sum(cnt.sphere);
    if (lane == 0) {
      atomicAdd(&stats->closest, c0);
      if (full_stats) {
        atomicAdd(&stats->internal, c2);
        atomicAdd(&stats->leaf, c3);
        atomicAdd(&stats->prim, c4);
        atomicAdd(&stats->sphere, c6);
      }
      if (c5) atomicAdd(&stats->nan_samples, c5);
    }
  }
}

}  // namespace vimg
