// feature_kernel<TEX>: the first-hit feature integrators (albedo, normal, depth, position, uv, coverage)
#include "kernel_tus.h"
#include "feature_kernel.h"

namespace vimg {
RenderKernel vimg_feature_kernel(bool tex) { return tex ? feature_kernel<true> : feature_kernel<false>; }
}  // namespace vimg
