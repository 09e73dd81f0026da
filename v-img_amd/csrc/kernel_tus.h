// The render kernels are instantiated in translation units of their own (k_*.hip: compiled in
// parallel); launch_policy.hip gets them through these getters.  Every build of render_cu_kernel is one of
// CU_WAVES (cu_layout.h: 16) waves per workgroup, four per SIMD.
#pragma once
#include "device_scene.h"

namespace vimg {

struct CuKArgs;
using RenderKernel = void (*)(const DScene, const RenderArgs, float*, DeviceStats*, unsigned int*);
using CuKernel = void (*)(const CuKArgs);

RenderKernel vimg_lane_kernel(bool tex, int wps);             // render_kernel<TEX, WPS>
RenderKernel vimg_feature_kernel(bool tex);                   // feature_kernel<TEX>: integrators ALBEDO .. COVERAGE
CuKernel vimg_cu_kernel(bool tex, bool deep);                 // render_cu_kernel<TEX, DEEP, CU_WAVES, 4, false, 0>
CuKernel vimg_cu_kernel_early(bool tex, bool deep);           // ... <..., false, 1>: rays queued as soon as they are known
CuKernel vimg_cu_kernel_diag(bool tex, bool deep);            // ... <..., true, 2>: statistics launches
// the PLAIN builds (plain_build.h: launch-constant options compiled in) of the two untextured builds for trees in LDS
CuKernel vimg_cu_kernel_plain();                              // render_cu_kernel<false, false, CU_WAVES, 4, false, 0, PLAIN_FOLD>
CuKernel vimg_cu_kernel_plain_early();                        // ... <..., false, 1, PLAIN_FOLD>
// ... and the same two for scenes that hold a material of class 3 (PLAIN_FOLD_OTHER: the fourth vertex ring stays)
CuKernel vimg_cu_kernel_plain_other();
CuKernel vimg_cu_kernel_plain_other_early();

}  // namespace vimg
