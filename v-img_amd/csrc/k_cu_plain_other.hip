// render_cu_kernel, the PLAIN build of k_cu_plain.hip for a scene that holds a material of class 3 (plain_build.h:
// PLAIN_FOLD_OTHER = PLAIN_FOLD without PF_NO_OTHER): the fourth vertex ring and the "any material" vertex stage are in it
#include "kernel_tus.h"
#include "render_cu_kernel.h"

namespace vimg {
CuKernel vimg_cu_kernel_plain_other() { return render_cu_kernel<false, false, CU_WAVES, 4, false, 0, PLAIN_FOLD_OTHER>; }
}  // namespace vimg
