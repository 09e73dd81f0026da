// Ray queries on a resident scene (vimg_hip_trace_rays, vimg_hip_occluded, vimg_hip_camera_rays):
// the render's own walk and hit record on rays the caller gives.
//
//   ray_query_kernel<QUERY_CLOSEST>       traverse<false>: t, primitive, barycentrics of vertices 2 and 3
//   ray_query_kernel<QUERY_CLOSEST_INFO>  the same + the make_hit_info<true> record (what PROBE_CLOSEST_HIT returns)
//   ray_query_kernel<QUERY_OCCLUDED>      traverse<true>: the render's shadow test, one byte per ray
//   camera_rays_kernel                    generate_ray per sample, one lane each (not a hot path)
//
// The query kernels call traverse / make_hit_info of render_kernels.h unchanged, so a ray's answer is the
// render's bits.  Launch shape: a persistent grid (as many 256-thread workgroups as the CU holds at the LDS
// size of lane_layout); each workgroup stages the top of the tree into LDS once and
// its waves then take whole 64-ray chunks, chunk = global wave + k * waves of the grid.  A lane loads its
// ray as two 16-byte loads and stores its hit as one (plus three for the record).  The same kernel on a
// grid of one workgroup per 256 rays is the probe's launch; which of the two runs is the policy of
// launch_query below (VIMG_HIP_QUERY_BLOCKS=0 / 1 forces one, tools only).
#include <hip/hip_runtime.h>

#include "hip_internal.h"
#include "ray_query.h"
#include "render_kernels.h"

namespace vimg {

namespace {

constexpr uint32_t kNoHit = 0xffffffffu;   // VIMG_NO_HIT

template <int KIND>
__global__ void __launch_bounds__(256)
ray_query_kernel(const DScene g, const RenderArgs A, const v4f* __restrict__ rays, uint32_t n,
                 v4f* __restrict__ hits, v4f* __restrict__ info, uint8_t* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const Lds L = stage_lds(g, A, (VIMG_LDS unsigned char*)lds_raw);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * (blockDim.x >> 6);
  const uint32_t chunks = uint32_t((uint64_t(n) + 63u) >> 6);   // (n + 63 wraps in 32 bits near 2^32)
  // chunk indices are wave-uniform: every lane of a wave runs the same trips (traverse's wave votes)
  for (uint32_t c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); c < chunks; c += waves) {
    const uint32_t i = (c << 6) + lane;
    if (i >= n) continue;   // the tail chunk's lanes beyond n
    const v4f r0 = rays[2 * size_t(i)], r1 = rays[2 * size_t(i) + 1];
    TravRay tr{f3{r0.x, r0.y, r0.z}, f3{r1.x, r1.y, r1.z}, r0.w, r1.w};
    // an empty range or a NaN in it: a miss without a walk
    const bool live = tr.min_t <= tr.max_t;
    Counters cnt{0, 0, 0, 0, 0, 0, 0, 0};
    HitRec rec;
    if (KIND == QUERY_OCCLUDED) {
      const bool occ = live && traverse<true>(g, L, tr, rec, cnt, false);
      flags[i] = occ ? uint8_t(1) : uint8_t(0);
      continue;
    }
    const bool hit = live && traverse<false>(g, L, tr, rec, cnt, false);
    // tri_hit_info's weights: u = e0 * inv_det (vertex 1), v = e1 * inv_det, w = e2 * inv_det
    const bool tri = hit && rec.kind == 0u;
    hits[i] = v4f{hit ? tr.max_t : VIMG_INF, __uint_as_float(hit ? rec.prim : kNoHit),
                  tri ? rec.e1 * rec.inv_det : 0.f, tri ? rec.e2 * rec.inv_det : 0.f};
    if (KIND == QUERY_CLOSEST_INFO) {
      v4f q0{0.f, 0.f, 0.f, 0.f}, q1 = q0, q2 = q0;
      if (hit) {
        Hit h;
        make_hit_info<true>(g, rec, tr, h);
        q0 = v4f{h.p.x, h.p.y, h.p.z, h.ns.x};
        q1 = v4f{h.ns.y, h.ns.z, h.ng.x, h.ng.y};
        q2 = v4f{h.ng.z, h.uv.x, h.uv.y, __uint_as_float(h.mat)};
      }
      info[3 * size_t(i)] = q0;
      info[3 * size_t(i) + 1] = q1;
      info[3 * size_t(i) + 2] = q2;
    }
  }
}

// TLCam::generate_ray as PROBE_CAMERA_RAY evaluates it: sample {x, y, lens_u, lens_v} -> {org, 1e-4}{dir, inf}
__global__ void __launch_bounds__(256)
camera_rays_kernel(const DScene g, const v4f* __restrict__ samples, uint32_t n, v4f* __restrict__ rays) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const v4f s = samples[i];
  f3 o, d;
  generate_ray(g, s.x, s.y, s.z, s.w, o, d);
  rays[2 * size_t(i)] = v4f{o.x, o.y, o.z, 0.0001f};
  rays[2 * size_t(i) + 1] = v4f{d.x, d.y, d.z, VIMG_INF};
}

}  // namespace

const void* ray_query_kernel(int kind) {
  if (kind == QUERY_CLOSEST_INFO) return reinterpret_cast<const void*>(ray_query_kernel<QUERY_CLOSEST_INFO>);
  if (kind == QUERY_OCCLUDED) return reinterpret_cast<const void*>(ray_query_kernel<QUERY_OCCLUDED>);
  return reinterpret_cast<const void*>(ray_query_kernel<QUERY_CLOSEST>);
}

hipError_t enqueue_ray_query(const DScene& d, const RenderArgs& A, int kind, uint32_t grid, uint32_t lds_bytes,
                             const void* rays, uint32_t n, void* hits, void* info, uint8_t* flags, hipStream_t st) {
  const v4f* r = static_cast<const v4f*>(rays);
  v4f* h = static_cast<v4f*>(hits);
  v4f* q = static_cast<v4f*>(info);
  if (kind == QUERY_CLOSEST_INFO)
    hipLaunchKernelGGL(ray_query_kernel<QUERY_CLOSEST_INFO>, dim3(grid), dim3(256), lds_bytes, st, d, A, r, n, h, q, flags);
  else if (kind == QUERY_OCCLUDED)
    hipLaunchKernelGGL(ray_query_kernel<QUERY_OCCLUDED>, dim3(grid), dim3(256), lds_bytes, st, d, A, r, n, h, q, flags);
  else
    hipLaunchKernelGGL(ray_query_kernel<QUERY_CLOSEST>, dim3(grid), dim3(256), lds_bytes, st, d, A, r, n, h, q, flags);
  return hipGetLastError();
}

hipError_t enqueue_camera_rays(const DScene& d, const void* samples, uint32_t n, void* rays, hipStream_t st) {
  const uint32_t grid = uint32_t((uint64_t(n) + 255u) / 256u);
  hipLaunchKernelGGL(camera_rays_kernel, dim3(grid), dim3(256), 0, st, d, static_cast<const v4f*>(samples), n,
                     static_cast<v4f*>(rays));
  return hipGetLastError();
}

}  // namespace vimg

// ---- the entry points.  The argument checks never read the scene, so they answer
// the same on a machine without a GPU; the calls then only enqueue, and read nothing of the scene's render scratch.
using namespace vimg;

namespace {

bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

int check_query(const char* what, const VimgDeviceScene* s, uint64_t n, const void* in, const char* in_name,
                const void* out, const char* out_name, bool out_aligned) {
  const std::string w(what);
  if (!s) return fail(VIMG_E_INVALID, w + ": null scene");
  if (n >= (1ull << 32)) return fail(VIMG_E_INVALID, w + ": n must be below 2^32");
  if (n == 0) return VIMG_OK;
  if (!in) return fail(VIMG_E_INVALID, w + ": null " + in_name);
  if (!out) return fail(VIMG_E_INVALID, w + ": null " + out_name);
  if (misaligned16(in)) return fail(VIMG_E_INVALID, w + ": " + in_name + " is not 16-byte aligned");
  if (out_aligned && misaligned16(out)) return fail(VIMG_E_INVALID, w + ": " + out_name + " is not 16-byte aligned");
  return VIMG_OK;
}

// The probe's LDS layout (stacks for max_depth + 2 entries, then the top of the tree) and, per query build, the
// workgroups a CU holds at that size.
int ensure_query(VimgDeviceScene* s) {
  if (s->query_ready) return VIMG_OK;
  VimgRenderParams p{VIMG_INTEGRATOR_MIS, 1, 1, 0, 1};
  const LaunchCfg c = lane_layout(facts_of(s), p);
  s->query_args = c.args;
  s->query_lds = c.lds_bytes;
  for (int k = QUERY_CLOSEST; k <= QUERY_OCCLUDED; ++k) {
    if (c.lds_bytes > 48u * 1024u)
      HIP_TRY(hipFuncSetAttribute(ray_query_kernel(k), hipFuncAttributeMaxDynamicSharedMemorySize, int(c.lds_bytes)));
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ray_query_kernel(k), 256, c.lds_bytes) != hipSuccess || per_cu < 1)
      per_cu = 1;
    s->query_per_cu[k] = uint32_t(per_cu);
  }
  s->query_ready = true;
  return VIMG_OK;
}

int launch_query(VimgDeviceScene* s, int kind, const void* rays, uint32_t n, void* hits, void* info, uint8_t* flags,
                 void* stream) {
  if (int rc = ensure_query(s)) return rc;
  hipStream_t st = stream_of(stream);
  const uint64_t chunks = (uint64_t(n) + 63u) / 64u;
  uint64_t grid = (chunks + 3u) / 4u;   // one workgroup per 256 rays
  // Policy: the persistent grid when the top of the tree is staged and the rest read from global memory (config 5
  // stand-in, 16 M rays: 1.03-1.34x); one workgroup per 256 rays when the whole tree sits in LDS or none of it does
  // (config 2: the persistent grid 0.85-0.98x on 11 of 12 rows, the caterpillar's stacks-only layout 0.92-0.96x at
  // 16 M rays) - there
  // the dispatcher's refill of finished workgroups balances chunks of unequal cost better than the persistent grid's
  // fixed share per wave, and the re-staging is cheap
  const bool persistent = s->query_launch == 1 ||
                          (s->query_launch == -1 && s->query_args.lds_nodes > 0 && s->query_args.lds_nodes < s->d.num_nodes);
  if (persistent) grid = std::min<uint64_t>(grid, uint64_t(s->num_cus) * s->query_per_cu[kind]);
  HIP_TRY(enqueue_ray_query(s->d, s->query_args, kind, uint32_t(grid), s->query_lds, rays, n, hits, info, flags, st));
  return VIMG_OK;
}

}  // namespace

extern "C" {

int vimg_hip_trace_rays(VimgDeviceScene* s, const void* d_rays, uint64_t n, void* d_hits, void* d_info, void* stream) {
  if (int rc = check_query("trace_rays", s, n, d_rays, "rays", d_hits, "hits", true)) return rc;
  if (n == 0) return VIMG_OK;
  if (d_info && misaligned16(d_info)) return fail(VIMG_E_INVALID, "trace_rays: info is not 16-byte aligned");
  return launch_query(s, d_info ? QUERY_CLOSEST_INFO : QUERY_CLOSEST, d_rays, uint32_t(n), d_hits, d_info, nullptr, stream);
}

int vimg_hip_occluded(VimgDeviceScene* s, const void* d_rays, uint64_t n, uint8_t* d_flags, void* stream) {
  if (int rc = check_query("occluded", s, n, d_rays, "rays", d_flags, "flags", false)) return rc;
  if (n == 0) return VIMG_OK;
  return launch_query(s, QUERY_OCCLUDED, d_rays, uint32_t(n), nullptr, nullptr, d_flags, stream);
}

int vimg_hip_camera_rays(VimgDeviceScene* s, const void* d_samples, uint64_t n, void* d_rays, void* stream) {
  if (int rc = check_query("camera_rays", s, n, d_samples, "samples", d_rays, "rays", true)) return rc;
  if (n == 0) return VIMG_OK;
  hipStream_t st = stream_of(stream);
  HIP_TRY(enqueue_camera_rays(s->d, d_samples, uint32_t(n), d_rays, st));
  return VIMG_OK;
}

}  // extern "C"
