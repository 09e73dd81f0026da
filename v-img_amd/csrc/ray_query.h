// Ray queries on a resident scene (vimg_hip_trace_rays, _occluded, _camera_rays): kernels, launch policy
// and entry points live in ray_query.hip; these are its seams (the probe shares the kernels' launch).
#pragma once
#include <hip/hip_runtime.h>

#include "device_scene.h"

namespace vimg {

enum RayQueryKind { QUERY_CLOSEST = 0, QUERY_CLOSEST_INFO = 1, QUERY_OCCLUDED = 2 };

// The kernel of one query kind (for hipOccupancyMaxActiveBlocksPerMultiprocessor and hipFuncSetAttribute).
const void* ray_query_kernel(int kind);

// Enqueues one query launch of `grid` 256-thread workgroups with `lds_bytes` of LDS laid out by `A`
// (launch_plan.h: lane_layout): rays 32 B each, hits 16 B, info 48 B (or nullptr), flags 1 B.
hipError_t enqueue_ray_query(const DScene& d, const RenderArgs& A, int kind, uint32_t grid, uint32_t lds_bytes,
                             const void* rays, uint32_t n, void* hits, void* info, uint8_t* flags, hipStream_t st);

// One lane per sample {x, y, lens_u, lens_v}: the camera's ray as a 32-byte VimgRay record.
hipError_t enqueue_camera_rays(const DScene& d, const void* samples, uint32_t n, void* rays, hipStream_t st);

}  // namespace vimg
