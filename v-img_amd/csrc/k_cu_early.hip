// render_cu_kernel, the build whose vertex stages queue their rays as soon as they are known (EARLY): frames
// short of pixels and trees in global memory (launch_plan.hip:make_launch_cu)
#include "kernel_tus.h"
#include "render_cu_kernel.h"

namespace vimg {
CuKernel vimg_cu_kernel_early(bool tex, bool deep) {
  if (tex) return deep ? render_cu_kernel<true, true, CU_WAVES, 4, false, 1> : render_cu_kernel<true, false, CU_WAVES, 4, false, 1>;
  return deep ? render_cu_kernel<false, true, CU_WAVES, 4, false, 1> : render_cu_kernel<false, false, CU_WAVES, 4, false, 1>;
}
}  // namespace vimg
