// render_cu_kernel, the PLAIN build of k_cu_plain_early.hip for a scene that holds a material of class 3 (plain_build.h:
// PLAIN_FOLD_OTHER = PLAIN_FOLD without PF_NO_OTHER)
#include "kernel_tus.h"
#include "render_cu_kernel.h"

namespace vimg {
CuKernel vimg_cu_kernel_plain_other_early() { return render_cu_kernel<false, false, CU_WAVES, 4, false, 1, PLAIN_FOLD_OTHER>; }
}  // namespace vimg
