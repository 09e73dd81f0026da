// What the kernels that weigh a tap by the first-hit guides share (libvimg_filter.so, libvimg_varfilter.so,
// libvimg_infill.so): the albedo floor, the Rec. 709 luminance and the edge-stopping score of the
// normal and plane terms.  Internal, like frame_lib.h: shared source in an anonymous namespace, never a dynamic symbol.
#pragma once
#include <hip/hip_runtime.h>

namespace vimg_frames {
namespace {

__device__ inline float floored(float a, float floor) { return a > floor ? a : floor; }
__device__ inline float lum(float x, float y, float z) { return (x * 0.212671f + y * 0.715160f) + z * 0.072169f; }

// s_n + s_p of the tap q for the pixel p (normal np, position pp, plane_den = (sigma_plane z_p)^2); sigma_normal and
// plane_den are divided by, as the contracts say: no reciprocals
__device__ inline float guide_score(const float4& np, const float4& pp, const float4& nq, const float4& pq, float sigma_normal,
                                    float plane_den) {
  const float dn = 1.f - ((np.x * nq.x + np.y * nq.y) + np.z * nq.z);
  const float s_n = dn < 0.f ? 0.f : dn / sigma_normal;
  const float ex = pq.x - pp.x, ey = pq.y - pp.y, ez = pq.z - pp.z;
  const float d = (np.x * ex + np.y * ey) + np.z * ez;
  const float s_p = (d * d) / plane_den;
  return s_n + s_p;
}

}  // namespace
}  // namespace vimg_frames
