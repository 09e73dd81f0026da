// Geometry update of a resident scene (vimg_hip_scene_update_geometry): the records the
// upload bakes from the positions are baked again from new ones, with the upload's float expressions,
// and the tree keeps its topology while its boxes are recomputed bottom-up.
//
//   scene_update_tris     one thread per triangle: DTriShade positions, face normal n, tri_area_pdf
//   scene_update_spheres  one thread per sphere: centre and radius of d.spheres (the material stays)
//   scene_update_leaves   one thread per leaf slot: a, b, c0 and the degenerate flag of DLeafPrim
//   scene_update_lights   one thread per emitter: the triangle / sphere fields of DLight
//   scene_refit_chains    one thread per chain record (leaves over 127 primitives): the leaf's box twice
//   scene_refit_level     one thread per internal node of one breadth-first level, deepest level first
//   scene_refit_root      one thread: the root's box for DScene::root_min / root_max
//
// Boxes are folded with the host's selects (b < a ? b : a, a < b ? b : a; host/hmath.hpp) in the host
// builders' order: a triangle's box is vmin(v0, vmin(v1, v2)), a leaf's the fold over its primitives in
// obj_indices order from the first, an internal child's grow(left, right).  The levels need no
// synchronisation between workgroups: a launch only reads records the launches before it wrote.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "scene_bake.h"
#include "scene_boxes.h"
#include "scene_update.h"

namespace vimg {

namespace {

constexpr uint32_t kRefMask = (1u << 25) - 1u;

// the scene's tables as plain (flat) pointers: records are copied whole, and written (off the hot path)
template <typename T>
VD T* flat(gptr<T> p) {
  return (T*)p;
}

// prim_bounds (host/bvh_build.cpp) of one leaf slot
VD Box3 slot_box(const DScene& d, uint32_t j) {
  const DLeafPrim lp = flat(d.leaf_prims)[j];
  if (lp.kind == 1u) return sphere_box(mk3(lp.a.x, lp.a.y, lp.a.z), lp.a.w);
  return tri_box(mk3(lp.a.x, lp.a.y, lp.a.z), mk3(lp.a.w, lp.b.x, lp.b.y), mk3(lp.b.z, lp.b.w, lp.c0));
}

VD Box3 leaf_box(const DScene& d, uint32_t first, uint32_t count) {
  Box3 b = slot_box(d, first);
  for (uint32_t i = 1; i < count; ++i) b = grow(b, slot_box(d, first + i));
  return b;
}

// the box a child reference stands for: a leaf's fold, or the union of a node's two children (a chain
// record carries its whole leaf on both sides, and grow(b, b) is b bit for bit)
VD Box3 ref_box(const DScene& d, uint32_t ref) {
  const uint32_t count = ref >> 25, idx = ref & kRefMask;
  if (count) return leaf_box(d, idx, count);
  const DNode n = flat(d.nodes)[idx];
  const Box3 l{mk3(n.a.x, n.a.y, n.a.z), mk3(n.a.w, n.b.x, n.b.y)};
  const Box3 r{mk3(n.b.z, n.b.w, n.c.x), mk3(n.c.y, n.c.z, n.c.w)};
  return grow(l, r);
}

VD void store_boxes(const DScene& d, uint32_t i, Box3 l, Box3 r) {
  const float lmin[3] = {l.lo.x, l.lo.y, l.lo.z}, lmax[3] = {l.hi.x, l.hi.y, l.hi.z};
  const float rmin[3] = {r.lo.x, r.lo.y, r.lo.z}, rmax[3] = {r.hi.x, r.hi.y, r.hi.z};
  pack_boxes(flat(d.nodes)[i], lmin, lmax, rmin, rmax);
}

}  // namespace

__global__ void scene_update_tris(const DScene d, const float* vertices, uint32_t num_tris) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= num_tris) return;
  DTriShade* ts = flat(d.tri_shade) + t;
  const uint32_t ids[3] = {ts->i0, ts->i1, ts->i2};
  float v[9];
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a) v[k * 3 + a] = vertices[size_t(ids[k]) * 3 + a];
  float n[3], area_pdf;
  bake_tri_normal_pdf(v, n, &area_pdf);
  for (int k = 0; k < 9; ++k) ts->p[k] = v[k];
  for (int a = 0; a < 3; ++a) ts->n[a] = n[a];
  flat(d.tri_area_pdf)[t] = area_pdf;
}

__global__ void scene_update_spheres(const DScene d, const float* centre_radius, uint32_t num_spheres) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_spheres) return;
  VimgSphere* sp = flat(d.spheres) + i;
  for (int a = 0; a < 3; ++a) sp->center[a] = centre_radius[size_t(i) * 4 + a];
  sp->radius = centre_radius[size_t(i) * 4 + 3];
}

__global__ void scene_update_leaves(const DScene d, uint32_t num_slots) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= num_slots) return;
  DLeafPrim* lp = flat(d.leaf_prims) + j;
  const VimgPrim p = flat(d.prims)[lp->prim];
  if (p.type == VIMG_PRIM_TRIANGLE) {
    bake_leaf_tri(flat(d.tri_shade)[p.index].p, *lp);
  } else {
    bake_leaf_sphere(flat(d.spheres)[p.index], *lp);
  }
}

__global__ void scene_update_lights(const DScene d) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.num_lights) return;
  const VimgLight l = flat(d.lights)[i];
  if (l.type == VIMG_LIGHT_BACKGROUND) return;
  const VimgPrim p = flat(d.prims)[l.prim];
  DLight* L = flat(d.dlights) + i;
  if (p.type == VIMG_PRIM_TRIANGLE) {
    bake_light_tri(flat(d.tri_shade)[p.index], flat(d.tri_area_pdf)[p.index], *L);
  } else {
    bake_light_sphere(flat(d.spheres)[p.index], *L);
  }
}

__global__ void scene_refit_chains(const DScene d, const uint32_t* chain_leaf, uint32_t first_record, uint32_t n_chain) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_chain) return;
  const Box3 b = leaf_box(d, chain_leaf[2 * k], chain_leaf[2 * k + 1]);
  store_boxes(d, first_record + k, b, b);
}

__global__ void scene_refit_level(const DScene d, uint32_t begin, uint32_t end) {
  const uint32_t i = begin + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= end) return;
  const uint32_t lref = flat(d.nodes)[i].left_ref, rref = flat(d.nodes)[i].right_ref;
  store_boxes(d, i, ref_box(d, lref), ref_box(d, rref));
}

__global__ void scene_refit_root(const DScene d, float* root_box) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const Box3 b = ref_box(d, d.root_ref);
  root_box[0] = b.lo.x, root_box[1] = b.lo.y, root_box[2] = b.lo.z;
  root_box[3] = b.hi.x, root_box[4] = b.hi.y, root_box[5] = b.hi.z;
}

hipError_t enqueue_scene_update(const DScene& d, const SceneUpdate& u, hipStream_t st) {
  constexpr uint32_t kBlock = 256;
  auto blocks = [](uint32_t n) { return dim3((n + kBlock - 1) / kBlock); };
  if (u.vertices && u.num_tris)
    hipLaunchKernelGGL(scene_update_tris, blocks(u.num_tris), dim3(kBlock), 0, st, d, u.vertices, u.num_tris);
  if (u.spheres && u.num_spheres)
    hipLaunchKernelGGL(scene_update_spheres, blocks(u.num_spheres), dim3(kBlock), 0, st, d, u.spheres, u.num_spheres);
  // the slots read the triangle records and spheres written above, the lights too, the refit the slots
  hipLaunchKernelGGL(scene_update_leaves, blocks(u.num_slots), dim3(kBlock), 0, st, d, u.num_slots);
  if (d.num_lights) hipLaunchKernelGGL(scene_update_lights, blocks(d.num_lights), dim3(kBlock), 0, st, d);
  if (u.n_chain)
    hipLaunchKernelGGL(scene_refit_chains, blocks(u.n_chain), dim3(kBlock), 0, st, d, u.chain_leaf, u.n_internal, u.n_chain);
  for (uint32_t k = u.num_levels; k-- > 0;) {
    const uint32_t begin = u.level_begin[k], end = u.level_begin[k + 1];
    hipLaunchKernelGGL(scene_refit_level, blocks(end - begin), dim3(kBlock), 0, st, d, begin, end);
  }
  hipLaunchKernelGGL(scene_refit_root, dim3(1), dim3(64), 0, st, d, u.root_box);
  return hipGetLastError();
}

}  // namespace vimg
