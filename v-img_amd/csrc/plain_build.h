// The PLAIN builds of render_cu_kernel: launch-constant options of the persistent loop compiled in.
//
// Every option below is wave-uniform and fixed for a whole launch, yet the general build reads it from
// RenderArgs on the hot path (a scalar load, a compare and a branch around code the launch never runs).  A
// PLAIN build (k_cu_plain.hip, k_cu_plain_early.hip) takes the options named in its mask as constants; the
// stage bodies read each one through ONE helper (render_cu_kernel.h: opt_*), so there is one text of every
// stage.  The list of what is folded and the host's test that a launch satisfies it stand side by side here:
// the policy (launch_policy.hip) runs a PLAIN build when, and only when, plain_build_serves() says yes.
//
// To leave an option at run time: take its bit out of PLAIN_FOLD (one line); the helper then reads the
// argument again and the predicate stops asking for it.
//
// This header is plain C++ (no HIP): tests compile the predicate on its own.
#pragma once
#include <cstdint>

namespace vimg {

enum : uint32_t {
  PF_INTEGRATOR = 1u,   // integrator == MIS: no material / normal integrator branches in the vertex stages and the hand-over
  PF_CLASSES = 2u,      // pool_classes == 3: classes as the leaf records name them, batches specialised by class
  PF_LEAF_LDS = 4u,     // lds_leaf != 0: the leaf loop reads its primitives from LDS only
  PF_SINGLE = 8u,       // no trace_pixel: single_x < 0
  PF_ITEMS = 16u,       // no item list (masked progressive increments bring one)
  PF_FLEX = 32u,        // cu_flex at the policy's default: walking waves may shade (bit 1), no wave priorities (bits 2 and 4),
                        // split batches on (bit 16 clear); bit 32 (early rays) is the EARLY template parameter already
  // The launch-constant shading tables, read from the workgroup's copies in LDS (render_kernels.h: LdsTables, tb_*),
  // one bit per group; a group is staged whole or not at all (launch_policy.hip), as the leaf records are
  PF_TAB_HIT = 64u,     // hit records: prims, tri_shade, spheres, material_flags, meshes
  PF_TAB_MAT = 128u,    // materials: materials, dmaterials.  NOT folded by default (it costs the PLAIN
                        // kernels their 128th register; a sweep bit, like every other, through -DVIMG_PLAIN_FOLD)
  PF_TABLES = PF_TAB_HIT | PF_TAB_MAT,   // (the emitter tables stay in global memory: DESIGN.md 4.4)
  // The leaf records once more per major axis of a ray (kz == 0, kz == 1; the leaf table itself is kz == 2), their
  // triangles' vertices permuted as the watertight test permutes them: a lane reads the copy of its ray's axis and
  // the test permutes nothing.  A scene without triangles needs no copy
  PF_LEAF_PERM = 256u,
  // The resident scene holds no material of class 3 ("other": what is neither an emitter nor Lambertian nor Principled,
  // scene_bake.h: bake_material_class), so no slot ever goes to the fourth vertex ring: the hand-over, the main loop's
  // look and the dispatch drop that ring, and the "any material" vertex stage is not instantiated.  The only bit that
  // describes the SCENE: a scene that does hold such a material runs the build without it (PLAIN_FOLD_OTHER).  It needs
  // the integrator and the classes folded (another integrator, fewer classes route differently): opt_no_other
  PF_NO_OTHER = 512u,
};
// What the PLAIN builds fold (DESIGN.md 4.4 has the times of the candidates)
#ifdef VIMG_PLAIN_FOLD   // (sweeps: -DVIMG_PLAIN_FOLD=<mask> on the units that include this header)
constexpr uint32_t PLAIN_FOLD = VIMG_PLAIN_FOLD;
#else
constexpr uint32_t PLAIN_FOLD = PF_INTEGRATOR | PF_CLASSES | PF_LEAF_LDS | PF_SINGLE | PF_ITEMS | PF_FLEX | PF_TAB_HIT | PF_LEAF_PERM | PF_NO_OTHER;
#endif
// ... and what the PLAIN builds of a scene with a material of class 3 fold (k_cu_plain_other*.hip): the same without the bit
constexpr uint32_t PLAIN_FOLD_OTHER = PLAIN_FOLD & ~PF_NO_OTHER;

// what the predicate needs to know of a launch (plain_launch_of below fills it)
struct PlainLaunch {
  bool cu_sched;        // render_cu_kernel (not the lane-bound kernel)
  bool textured, deep;  // the TEX / DEEP builds have no PLAIN counterpart
  int cu_waves;         // 16
  bool stats;           // a statistics launch runs the DIAG build
  bool force_general;   // VIMG_HIP_PLAIN=0 at upload
  uint32_t integrator, pool_classes, lds_leaf, cu_flex;
  int single_x;
  bool has_item_list;
  bool has_other = false;   // the resident scene holds a material of class 3 (known at upload, again after a material edit)
};
constexpr uint32_t PLAIN_INTEGRATOR_MIS = 3u;   // (VIMG_INTEGRATOR_MIS; render_cu_kernel.h asserts they agree)
constexpr uint32_t PLAIN_FLEX_DEFAULT = 1u;     // cu_flex without the early bit

// true when a build that folds `fold` computes exactly what the general build computes for this launch
constexpr bool plain_build_serves(const PlainLaunch& l, uint32_t fold = PLAIN_FOLD) {
  if (l.force_general || !l.cu_sched || l.textured || l.deep || l.cu_waves != 16 || l.stats) return false;
  if ((fold & PF_INTEGRATOR) && l.integrator != PLAIN_INTEGRATOR_MIS) return false;
  if ((fold & PF_CLASSES) && l.pool_classes != 3u) return false;
  if ((fold & PF_LEAF_LDS) && l.lds_leaf == 0u) return false;
  if ((fold & PF_SINGLE) && l.single_x >= 0) return false;
  if ((fold & PF_ITEMS) && l.has_item_list) return false;
  if ((fold & PF_FLEX) && (l.cu_flex & ~32u) != PLAIN_FLEX_DEFAULT) return false;
  if ((fold & PF_NO_OTHER) && l.has_other) return false;
  return true;
}
// The fold of the PLAIN build that serves the launch: PLAIN_FOLD, else PLAIN_FOLD_OTHER (the scene holds class 3); 0 = none
constexpr uint32_t plain_fold_serving(const PlainLaunch& l) {
  return plain_build_serves(l, PLAIN_FOLD) ? PLAIN_FOLD : (plain_build_serves(l, PLAIN_FOLD_OTHER) ? PLAIN_FOLD_OTHER : 0u);
}

// The table groups are one more folded constant, with a predicate of their own beside the one above: `staged` is
// the launch's RenderArgs::lds_tables (the groups the policy found room for).  A build that reads a group from LDS
// serves only launches that staged it; a launch whose tables do not fit runs the general build.
constexpr bool plain_tables_serve(uint32_t staged, uint32_t fold = PLAIN_FOLD) {
  return (staged & fold & PF_TABLES) == (fold & PF_TABLES);
}

// The permuted leaf copies likewise: `ready` is the launch's RenderArgs::leaf_perm (the policy staged the two copies,
// or the scene has no triangle and needs none).  A build that reads a lane's leaves from the copy of its ray's axis
// serves only launches where that copy is there; a launch whose copies do not fit runs the general build.
constexpr bool plain_leaf_perm_serves(uint32_t ready, uint32_t fold = PLAIN_FOLD) {
  return !(fold & PF_LEAF_PERM) || ready != 0u;
}

// The description of a launch from what the policy knows of it: the kernel family and the build class, whether
// statistics were asked for, the override, and the launch's arguments (RenderArgs; a template so that this header
// stays plain C++ and the mapping can be tested without the device headers).
template <class Args>
constexpr PlainLaunch plain_launch_of(bool cu_sched, bool textured, bool deep, int cu_waves, bool stats, bool force_general,
                                      const Args& a, bool has_other = false) {
  return PlainLaunch{cu_sched, textured, deep, cu_waves, stats || a.full_stats != 0u, force_general,
                     a.integrator, a.pool_classes, a.lds_leaf, a.cu_flex, a.single_x, a.item_list != nullptr, has_other};
}

}  // namespace vimg
