// render_cu_kernel, the PLAIN build of thin shards of untextured frames on trees in LDS: k_cu_early.hip's
// build (rays queued as soon as they are known) with the launch-constant options of plain_build.h compiled in
#include "kernel_tus.h"
#include "render_cu_kernel.h"

namespace vimg {
CuKernel vimg_cu_kernel_plain_early() { return render_cu_kernel<false, false, CU_WAVES, 4, false, 1, PLAIN_FOLD>; }
}  // namespace vimg
