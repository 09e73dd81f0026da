// render_cu_kernel, the PLAIN build whole untextured frames on trees in LDS are timed on: the general build of
// k_cu.hip with the launch-constant options of plain_build.h compiled in (launch_policy.hip picks it when, and
// only when, the launch satisfies every one of them)
#include "kernel_tus.h"
#include "render_cu_kernel.h"

namespace vimg {
CuKernel vimg_cu_kernel_plain() { return render_cu_kernel<false, false, CU_WAVES, 4, false, 0, PLAIN_FOLD>; }
}  // namespace vimg
