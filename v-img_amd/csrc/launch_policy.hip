// The HIP side of the launch policy.  The plan of a launch is launch_plan.hip's, which knows a scene by a few facts
// and asks the runtime nothing; here those facts are taken from the device scene (facts_of, the one place), a
// lane-shaped launch gets the one occupancy query that sizes its persistent grid, and a plan is mapped to the kernel
// that runs it.
#include "hip_internal.h"
#include "plain_build.h"

namespace vimg {

LaunchFacts facts_of(const VimgDeviceScene* s) {
  LaunchFacts f{};
  f.res_x = s->d.res_x, f.res_y = s->d.res_y;
  f.num_nodes = s->d.num_nodes, f.max_depth = s->d.max_depth;
  f.num_cus = s->num_cus;
  f.num_leaf_prims = s->num_leaf_prims;
  f.num_tris = s->num_tris, f.num_spheres = s->num_spheres, f.num_meshes = s->num_meshes;
  f.num_materials = uint32_t(s->materials.size());
  f.textured = s->textured, f.too_wide = s->too_wide, f.force_general = s->force_general;
  f.no_lds_tables = s->no_lds_tables, f.has_other = s->has_other;
  f.waves_per_simd = s->waves_per_simd;
  f.opt = s->opt;
  return f;
}

// the kernel the policy sizes a lane-shaped launch for, which is the one that runs
static const void* lane_kernel_of(const VimgDeviceScene* s, const LaunchCfg& c) {
  if (c.feature) return reinterpret_cast<const void*>(vimg_feature_kernel(s->textured));
  return reinterpret_cast<const void*>(vimg_lane_kernel(s->textured, c.wps));
}

const void* launched_kernel_of(const VimgDeviceScene* s, const LaunchCfg& c, bool stats) {
  if (c.sched != VIMG_SCHED_CU) return lane_kernel_of(s, c);
  const bool early = (c.args.cu_flex & 32u) != 0u;
  const uint32_t plain = plain_fold_of(facts_of(s), c, stats);   // the fold of the PLAIN build that serves the launch; 0 = none does
  CuKernel k;
  if (plain == PLAIN_FOLD) k = early ? vimg_cu_kernel_plain_early() : vimg_cu_kernel_plain();
  else if (plain != 0u) k = early ? vimg_cu_kernel_plain_other_early() : vimg_cu_kernel_plain_other();
  else k = stats ? vimg_cu_kernel_diag(s->textured, c.deep)
                 : (early ? vimg_cu_kernel_early(s->textured, c.deep) : vimg_cu_kernel(s->textured, c.deep));
  return reinterpret_cast<const void*>(k);
}

LaunchCfg make_launch(const VimgDeviceScene* s, const VimgRenderParams* p, int sx, int sy) {
  const LaunchFacts f = facts_of(s);
  const LaunchCfg c = plan_launch(f, *p, sx, sy, 1);
  if (c.error || c.sched == VIMG_SCHED_CU) return c;
  // a lane-shaped launch: ONE occupancy query, of the kernel that will run, sizes the persistent grid
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lane_kernel_of(s, c), 256, c.lds_bytes) != hipSuccess || per_cu <= 1) return c;
  return plan_launch(f, *p, sx, sy, per_cu);
}

}  // namespace vimg

using namespace vimg;

extern "C" {

const char* vimg_hip_launch_kernel(const VimgDeviceScene* s, const VimgRenderParams* p) {
  if (!s || !p) return "";
  return launch_kernel_name(facts_of(s), *p);
}

const char* vimg_hip_scene_kernel(const VimgDeviceScene* s) {
  // the scheduler is chosen per launch: report the one of a whole frame
  const VimgRenderParams whole{VIMG_INTEGRATOR_MIS, 64, 1, 0, 1};
  return vimg_hip_launch_kernel(s, &whole);
}

}  // extern "C"
