// The launch planner (launch_plan.hip): from a few facts of the resident scene, the render parameters and the options,
// the complete plan of one launch - kernel family, grid, LDS layout (cu_layout.h), scheduler parameters, scratch.  It
// asks the runtime nothing and touches no device: tests/test_launch_plan.py drives it from a host program.
// launch_policy.hip fills the facts from a VimgDeviceScene, adds the one occupancy query (of a lane-shaped launch) and
// maps a plan to the kernel that runs it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/vimg_hip.h"
#include "device_scene.h"

#pragma GCC visibility push(hidden)
namespace vimg {

// what the planner knows of a scene (launch_policy.hip: facts_of)
struct LaunchFacts {
  int32_t res_x, res_y;
  uint32_t num_nodes, max_depth;   // internal nodes of the tree, its depth
  uint32_t num_cus;
  uint32_t num_leaf_prims;
  uint32_t num_tris, num_spheres, num_meshes, num_materials;   // the rows of the tables a launch may stage in LDS
  bool textured, too_wide, force_general, no_lds_tables, has_other;   // as VimgDeviceScene has them
  int waves_per_simd;              // LANE register budget by policy (scene size)
  VimgHipOptions opt;              // the caller's options (VIMG_OPT_AUTO where the policy decides)
};

struct LaunchCfg {
  const char* error;   // nullptr, or why no launch can be made of the scene's options (make_launch_cu): VIMG_E_INVALID
  RenderArgs args;
  uint32_t grid, lds_bytes;
  uint32_t table_bytes;   // CU scheduler: the part of lds_bytes that holds the shading tables and the permuted leaf copies (the end of the layout)
  int sched;     // VIMG_SCHED_CU (a workgroup of CU_WAVES waves, cu_layout.h) or VIMG_SCHED_LANE (of four)
  int wps;       // register-budget build (waves per SIMD of __launch_bounds__)
  bool deep;     // CU scheduler: build whose box loop yields to waiting leaves (tree beyond the LDS node cache)
  bool feature;  // feature_kernel (integrators ALBEDO .. COVERAGE) in the lane launch's shape: sched is VIMG_SCHED_LANE
  size_t cold_bytes;   // scene-owned scratch of the launch: cold slot records of every workgroup (0: none) ...
  size_t ovf_bytes;    // ... and the stack entries beyond stack_lds (0: the stacks fit)
};

inline uint32_t tiles_of(int n) { return (static_cast<uint32_t>(n) + 7u) / 8u; }
// the first-hit feature integrators (feature_kernel.h): one kernel of their own, whatever the scheduler option says
inline bool is_feature_integrator(uint32_t i) { return i >= VIMG_INTEGRATOR_ALBEDO && i <= VIMG_INTEGRATOR_COVERAGE; }
inline uint32_t opt_or(int32_t v, uint32_t dflt) { return v == VIMG_OPT_AUTO ? dflt : static_cast<uint32_t>(v); }

uint32_t local_tiles(const LaunchFacts& f, const VimgRenderParams& p);   // tiles of the frame the shard owns
// The plan of a launch; (sx, sy): that pixel alone when >= 0.  A lane-shaped launch (the lane-bound kernel by name or for
// a frame too wide, feature_kernel) has a persistent grid of `lane_per_cu` workgroups per compute unit, which its
// kernel's occupancy decides: the caller's number.  The CU scheduler's workgroup is a whole compute unit
LaunchCfg plan_launch(const LaunchFacts& f, const VimgRenderParams& p, int sx, int sy, int lane_per_cu);
// the lane launch's arguments and LDS layout (stacks, then the top of the tree) without a grid: all that probes, the
// heatmap and the ray queries take of it
LaunchCfg lane_layout(const LaunchFacts& f, const VimgRenderParams& p);
// the fold of the PLAIN build (plain_build.h) that serves the launch as its arguments stand, 0 = none does
uint32_t plain_fold_of(const LaunchFacts& f, const LaunchCfg& c, bool stats);
// takes the shading tables out of a launch that will not run a PLAIN build (call once its arguments are complete)
void drop_unread_tables(const LaunchFacts& f, LaunchCfg& c, bool stats);
// what vimg_hip_launch_kernel answers for a whole frame with these parameters
const char* launch_kernel_name(const LaunchFacts& f, const VimgRenderParams& p);

}  // namespace vimg
#pragma GCC visibility pop
