// What the host units of libvimg_hip.so share (none of it is exported: include/vimg_hip.h is the ABI).
//   vimg_hip.hip       init / options / last_error, the render entry points, enqueue_render
//   scene_upload.hip   validation, baking and upload of a scene, its changes, its release
//   launch_plan.hip    the plan of one launch (render_cu_kernel, the lane-bound render_kernel, feature_kernel) from a
//                      few facts of the scene: host arithmetic only, no runtime call (launch_plan.h; cu_layout.h is the
//                      workgroup's LDS, shared with the kernel)
//   launch_policy.hip  its HIP side: the facts of a device scene, the lane launch's occupancy query, plan -> kernel
//   ray_query.hip      ray queries        precompute.hip   texture pre-pass and post-processing
//   scene_rebuild.hip  a new tree for a resident scene, its cost       bvh_build.hip    the GPU builders and their cores
//   scene_relight.hip  new materials, texture contents, emitters and background of a resident scene
//   device_mem.h       fail / HIP_TRY, and DevBuf / DevEvent: the one owner type of device memory, and of events
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vimg_hip.h"
#include "device_mem.h"
#include "device_scene.h"
#include "kernel_tus.h"
#include "launch_plan.h"

#pragma GCC visibility push(hidden)
struct VimgDeviceScene {
  vimg::DScene d{};            // the kernels' view: raw pointers into the buffers below
  // the tables a rebuild replaces, under their own names; the others, fixed at upload, in upload order
  vimg::DevBuf nodes, leaf_prims;
  vimg::DevBuf chain_leaf;     // per chain record {first slot, count} of its whole leaf (uint32_t pairs; empty: no chains)
  std::vector<vimg::DevBuf> tables;
  size_t total_bytes = 0;      // of nodes, leaf_prims and tables (vimg_hip_scene_bytes)
  bool textured = false;       // needs the TEX=true kernels (cones, image textures, env map)
  VimgHipOptions opt{};        // the caller's options (VIMG_OPT_AUTO where the policy decides)
  int waves_per_simd = 2;      // LANE register budget by policy (scene size)
  bool too_wide = false;       // resolution beyond the 16-bit pixel coordinates of the slot records
  bool force_general = false;  // VIMG_HIP_PLAIN=0 at upload: never a PLAIN build of render_cu_kernel (tests, A/B runs)
  bool no_lds_tables = false;  // VIMG_HIP_LDS_TABLES=0 at upload: no launch stages the shading tables in LDS (tests, A/B runs)
  bool has_other = false;      // a material of class 3 is in the table (scene_bake.h: table_holds_other; upload and every material edit)
  uint32_t num_cus = 0;
  uint32_t num_leaf_prims = 0;   // records in d.leaf_prims (= primitives of the scene)
  // scratch owned by the scene; the last four grow to what a launch asks for and never shrink
  vimg::DevBuf stats;            // one DeviceStats
  vimg::DevBuf counter;          // unsigned int[2]: the work counter, the error word of the last launch
  vimg::DevBuf root_box;         // 6 floats the refit leaves the root's box in
  vimg::DevBuf frame;            // host renders: the frame before it is copied out
  vimg::DevBuf pool_cold;        // CU scheduler: cold slot records of every workgroup
  vimg::DevBuf stack_ovf;        // CU scheduler, deep trees: the stack entries beyond the LDS part, per walking wave
  vimg::DevBuf pool_state;       // CU scheduler: per-pixel record between sample segments
  uint32_t pool_epoch = 0;       // bumped per launch: tags of earlier launches never match
  // geometry updates (vimg_hip_scene_update_geometry): what the upload knew of the tables and the tree
  uint64_t generation = 0;       // bumped by every change of the resident scene; accumulators remember theirs
  uint32_t num_vertices = 0, num_tris = 0, num_spheres = 0;
  uint32_t num_meshes = 0;       // (with the counts above and the host copies below: the rows of the tables a launch may stage in LDS)
  std::vector<std::pair<uint32_t, uint32_t>> normal_rows;   // (first vertex, count) of the meshes with normals, merged
  uint32_t n_internal = 0;       // DNode records of the tree; the n_chain chain records follow them
  uint32_t n_chain = 0;
  std::vector<uint32_t> level_begin;        // breadth-first levels of the internal nodes: [level_begin[k], level_begin[k+1])
  // material updates (scene_relight.hip): host copies of the small tables an update is checked against, and the
  // places in `tables` of the buffers it writes or swaps
  std::vector<VimgMaterial> materials;
  std::vector<VimgTexture> textures;
  std::vector<VimgLight> lights;
  uint32_t num_rg_textures = 0;
  uint64_t num_texels = 0, num_cdf = 0;
  size_t lights_table = 0, dlights_table = 0, dmaterials_table = 0;
  // ray queries (vimg_hip_trace_rays, _occluded): the LDS layout and the blocks per CU of each query build, worked
  // out at the first query and again after vimg_hip_scene_rebuild_bvh (which resets query_ready: both depend on
  // max_depth and num_nodes; nothing else changes the tree's shape, and the options never change after upload)
  int query_launch = -1;        // VIMG_HIP_QUERY_BLOCKS (tools/ only): 0 = one workgroup per 256 rays (the probe's launch),
                                // 1 = the persistent grid, unset = the policy of launch_query
  bool query_ready = false;
  vimg::RenderArgs query_args{};
  uint32_t query_lds = 0;
  uint32_t query_per_cu[3] = {0, 0, 0};
};

// A frame rendered in increments (vimg_hip_progressive_*): its scene, its parameters and the pixel records.
struct VimgProgressive {
  VimgDeviceScene* scene = nullptr;
  VimgRenderParams params{};      // samples field unused
  uint64_t items = 0;             // work items of a launch (64 per tile of the shard)
  vimg::DevBuf rec[2];            // 32 B per item each; rec[cur] holds the state after `samples`
  int cur = 0;
  uint32_t samples = 0;           // samples per pixel so far: every pixel's count while `uniform`, else the largest
  vimg::DevBuf scratch;           // the means of increments asked for without an output buffer
  uint64_t generation = 0;        // the scene's generation its records were made in
  // adaptive sampling (progressive_adaptive.hip): the records also keep each pixel's count, increments and M2
  bool uniform = true;            // every pixel stands at `samples` (no masked call since the last reset left some behind)
  uint64_t valid_items = 0;       // items that are pixels (ragged tiles have slots off the image)
  uint64_t launches = 0;          // render launches of the successful calls since the last reset
  vimg::DevBuf item_list;         // the work items of one count class, `items` words
  vimg::DevBuf block_counts;      // members per workgroup of the list kernels, then their offsets
  vimg::DevBuf ctl;               // control words of a call (adaptive_kernels.h: ACTL_*)
};

namespace vimg {

extern hipStream_t g_stream;   // vimg_hip.hip (vimg_hip_init)
extern int g_device;
// the stream argument of the ABI: NULL = the library's own stream
inline hipStream_t stream_of(void* stream) { return stream ? static_cast<hipStream_t>(stream) : g_stream; }

// ---- bvh_build.hip: the cores of vimg_hip_build_ploc / _lbvh.  They take the primitive bounds (n x {min.xyz,
// max.xyz}) on the device and leave the tree in the reference's layout (include/bvh.h:22-57) there too: nodes
// [num_nodes] of VimgBVHNode, bb [(2 num_nodes + 2) x 3] floats, obj_indices [n] of uint32_t.  Blocking, on the
// null stream; VIMG_PLOC_* and VIMG_HIP_DIAG as for the exported builders.
struct DeviceTree {
  DevBuf nodes, bb, obj_indices;
  uint32_t num_nodes = 0, max_depth = 0;
  std::vector<uint32_t> level_internal;   // nodes with children on every level that has some, root level first
};
int build_tree_device(uint32_t builder /* VIMG_BUILDER_* */, uint32_t n, const float* d_bounds6, DeviceTree* out);

// ---- scene_upload.hip: the upload's checks of the material and the emitter table, shared with the material update
int validate_materials(const VimgMaterial* materials, uint32_t num_materials, const VimgTexture* textures, uint32_t num_textures,
                       uint32_t num_rg_textures);
int validate_lights(const VimgLight* lights, uint32_t num_lights, uint32_t num_prims);
// whether the tables need the TEX kernels, and Background::is_emissive
bool tables_textured(const VimgMaterial* materials, uint32_t num_materials, const VimgTexture* textures, const VimgBackground& bg);
bool background_is_emissive(const VimgBackground& bg);

// ---- scene_relight.hip: the fields of a VimgGeometryUpdate behind `spheres`.  check_ finds every
// argument error and touches nothing; prepare_ allocates what the call needs (new emitter buffers, the CDF kernels'
// temporaries) before anything is enqueued; enqueue_ puts copies and kernels on `st`; commit_, after the stream has
// been synchronised, swaps the new buffers in and takes the host copies.
struct RelightPlan {
  bool any = false;                  // the update carries one of the new fields
  DevBuf new_lights, new_dlights;    // set_lights: built beside the scene's
  DevBuf new_dmaterials;             // materials or textures: the baked material records, built beside the scene's
  DevBuf sin_elev, lum, row_int, row_tot;   // env-map CDFs: the kernels' temporaries
  std::vector<float> sin_table;
};
int check_relight(const VimgDeviceScene* s, const VimgGeometryUpdate* u);
int prepare_relight(const VimgDeviceScene* s, const VimgGeometryUpdate* u, RelightPlan* plan);
int enqueue_relight(VimgDeviceScene* s, const VimgGeometryUpdate* u, RelightPlan* plan, hipStream_t st);
void commit_relight(VimgDeviceScene* s, const VimgGeometryUpdate* u, RelightPlan* plan);
// one DMaterial per material into `out`, from the materials and texture records resident in `d` (the upload's bake
// and the re-bake of an edit: one kernel, material_terms.h's statements)
int enqueue_material_bake(const DScene& d, uint32_t num_materials, DMaterial* out, hipStream_t st);

// ---- precompute.hip: the launches of the texture pre-pass on device buffers.  level_offset: in texels from
// `texels`, level 0 filled; the CDFs go where row_cdf (h + 1 floats) and col_cdfs (h x (w + 1)) point
struct EnvCdfScratch {
  float* sin_elev;   // h floats: env_sin_table(h), uploaded
  float* lum;        // w * h
  float* row_int;    // h
  float* row_tot;    // 1
};
void enqueue_mip_levels(float* texels, const uint64_t* level_offset, uint32_t levels, uint32_t w, uint32_t h, uint32_t wrap_u,
                        uint32_t wrap_v, hipStream_t st);
std::vector<float> env_sin_table(uint32_t h);
void enqueue_env_cdfs(const float* img, uint32_t w, uint32_t h, const EnvCdfScratch& t, float* row_cdf, float* col_cdfs, hipStream_t st);

// ---- vimg_hip.hip: the one path every render takes, shared with progressive_adaptive.hip
// A progressive launch: p->samples more samples for pixels that have had `base`, their records read from `in`
// (when base > 0) and written to `out`; item_list, when given, names the work items of the launch (a masked
// increment's count class); keep_stats adds the launch's events to the scene's instead of starting them at 0.
struct ProgLaunch {
  uint32_t base;
  const void* in;
  void* out;
  const uint32_t* item_list = nullptr;
  uint32_t item_count = 0;
  bool keep_stats = false;
};
int check_params(const VimgDeviceScene* s, const VimgRenderParams* p);
int check_render(const VimgDeviceScene* s, const VimgRenderParams* p, const void* d_out);   // check_params, and an output to write
// One render for enqueue_render: into d_out on `st` (counter / queue resets, then the kernel).  stats: the statistics
// build, counting into the scene's DeviceStats; (sx, sy): that pixel alone; ev0 / ev1: recorded right around the kernel.
struct RenderLaunch {
  float* d_out;
  hipStream_t st;
  bool stats = false;
  int sx = -1, sy = -1;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  const ProgLaunch* prog = nullptr;
};
int enqueue_render(VimgDeviceScene* s, const VimgRenderParams* p, const RenderLaunch& r);
int check_kernel_error(VimgDeviceScene* s);    // reads (and clears) the scene's error word
uint64_t fetch_shard_pixels(const VimgDeviceScene* s, const VimgRenderParams* p);   // pixels the shard owns
int fetch_stats(VimgDeviceScene* s, const VimgRenderParams* p, VimgRenderStats* out);   // (paths = pixels x p->samples)

// ---- launch_policy.hip
LaunchFacts facts_of(const VimgDeviceScene* s);   // what the planner (launch_plan.h) knows of the scene: filled here and nowhere else
// the plan of a launch: plan_launch, with the grid of a lane-shaped launch sized by its kernel's occupancy
LaunchCfg make_launch(const VimgDeviceScene* s, const VimgRenderParams* p, int sx, int sy);
// the build that runs a plan (render_cu_kernel: the statistics build for `stats`, the early-ray build for cu_flex
// bit 5, a PLAIN build where plain_fold_of names one)
const void* launched_kernel_of(const VimgDeviceScene* s, const LaunchCfg& c, bool stats);

}  // namespace vimg
#pragma GCC visibility pop
