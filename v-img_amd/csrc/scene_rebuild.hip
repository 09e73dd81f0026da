// A new tree for a resident scene (vimg_hip_scene_rebuild_bvh) and the cost of the one it has
// (vimg_hip_scene_bvh_cost); DESIGN.md 4.13.  Everything a launch reads of a tree - the DNode records, the
// leaf slots in obj_indices order, root_ref and the root's box, num_nodes, max_depth - is made here by kernels
// from data that is already resident, so that the scene afterwards is byte for byte the upload of the host
// scene with the same positions and a vimg_host_build_bvh_with(vimg_hip_build_ploc / _lbvh) tree:
//
//   scene_rebuild_bounds    one lane per primitive: prim_bounds (host/bvh_build.cpp) from DTriShade.p / d.spheres
//   (bvh_build.hip)         the builder's core on those bounds: the tree in the reference's layout, on the device
//   scene_rebuild_classify  one lane per node of that layout: "has children" (and "leaf over 127"), for the scan
//   scene_rebuild_nodes     one lane per node with children: its DNode at its breadth-first rank - what
//                           renumber_bvh, leaf_ref and pack_boxes (scene_upload.hip) do on the host
//   scene_rebuild_cls       one lane per old leaf slot: the material class of its primitive, by primitive
//   scene_rebuild_slots     one lane per new leaf slot: bake_leaves (scene_upload.hip) in the new obj_indices order
//   scene_bvh_cost_partial  one lane per DNode: area x weight of its two children, summed per workgroup
//   scene_bvh_cost_final    one workgroup: the partial sums in index order, the root's term, the division
//
// The reference layout is breadth-first with siblings adjacent (emit_reference_layout), so the exclusive count
// of nodes with children before a node IS the index renumber_bvh gives it, and a level's nodes are one index
// range; tests/test_scene_rebuild.py compares with the upload instead of assuming so.  No kernel waits for
// another workgroup and none uses an atomic: the scan gives every record its place.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "hip_internal.h"
#include "scene_bake.h"
#include "scene_boxes.h"

namespace vimg {

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kRefMask = (1u << 25) - 1u;

template <typename T>
VD T* flat(gptr<T> p) {
  return (T*)p;
}

dim3 blocks_for(uint32_t n) { return dim3((n + kBlock - 1) / kBlock); }

}  // namespace

__global__ void __launch_bounds__(kBlock) scene_rebuild_bounds(const DScene d, uint32_t num_prims, float* __restrict__ bounds6) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_prims) return;
  const VimgPrim p = flat(d.prims)[i];
  Box3 b;
  if (p.type == VIMG_PRIM_TRIANGLE) {
    const DTriShade ts = flat(d.tri_shade)[p.index];
    b = tri_box(mk3(ts.p[0], ts.p[1], ts.p[2]), mk3(ts.p[3], ts.p[4], ts.p[5]), mk3(ts.p[6], ts.p[7], ts.p[8]));
  } else {
    const VimgSphere sp = flat(d.spheres)[p.index];
    b = sphere_box(mk3(sp.center[0], sp.center[1], sp.center[2]), sp.radius);
  }
  float* o = bounds6 + size_t(i) * 6;
  o[0] = b.lo.x, o[1] = b.lo.y, o[2] = b.lo.z, o[3] = b.hi.x, o[4] = b.hi.y, o[5] = b.hi.z;
}

// low word: the node has children; high word: a leaf the 7-bit count of a child reference cannot hold
__global__ void __launch_bounds__(kBlock)
scene_rebuild_classify(const VimgBVHNode* __restrict__ nodes, uint32_t num_nodes, unsigned long long* __restrict__ packed) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_nodes) return;
  const uint32_t count = nodes[i].obj_count;
  packed[i] = count == 0u ? 1ull : (count > 127u ? (1ull << 32) : 0ull);
}

__global__ void __launch_bounds__(kBlock)
scene_rebuild_nodes(const VimgBVHNode* __restrict__ nodes, const float* __restrict__ bb, const unsigned long long* __restrict__ scanned,
                    uint32_t num_nodes, uint32_t n_internal, DNode* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_nodes) return;
  const VimgBVHNode node = nodes[i];
  if (node.obj_count != 0u) return;
  const uint32_t first = node.first_index, rank = static_cast<uint32_t>(scanned[i]);
  if (first == 0u || first >= num_nodes - 1u || rank >= n_internal) return;   // (no builder's layout: nothing is indexed outside the arrays)
  uint32_t refs[2];
  for (uint32_t k = 0; k < 2u; ++k) {
    const VimgBVHNode c = nodes[first + k];
    refs[k] = c.obj_count == 0u ? static_cast<uint32_t>(scanned[first + k]) : ((c.obj_count << 25) | (c.first_index & kRefMask));
  }
  const float* box = bb + (size_t(first) * 2 + 2) * 3;   // {Lmin, Rmin, Lmax, Rmax}
  DNode dn{};
  pack_boxes(dn, box, box + 6, box + 3, box + 9);
  dn.left_ref = refs[0], dn.right_ref = refs[1];
  out[rank] = dn;
}

__global__ void __launch_bounds__(kBlock) scene_rebuild_cls(const DScene d, uint32_t num_slots, uint32_t* __restrict__ cls_of_prim) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= num_slots) return;
  const v4u tail = reinterpret_cast<const v4u*>(flat(d.leaf_prims) + j)[2];   // {c0, prim, kind, cls}
  if (tail.y < num_slots) cls_of_prim[tail.y] = tail.w;
}

__global__ void __launch_bounds__(kBlock)
scene_rebuild_slots(const DScene d, const uint32_t* __restrict__ obj_indices, const uint32_t* __restrict__ cls_of_prim, uint32_t num_slots,
                    DLeafPrim* __restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= num_slots) return;
  const uint32_t prim = obj_indices[j];
  if (prim >= num_slots) return;
  const VimgPrim p = flat(d.prims)[prim];
  DLeafPrim lp{};
  lp.prim = prim;
  lp.cls = cls_of_prim[prim];
  if (p.type == VIMG_PRIM_TRIANGLE) {
    bake_leaf_tri(flat(d.tri_shade)[p.index].p, lp);
  } else {
    bake_leaf_sphere(flat(d.spheres)[p.index], lp);
    lp.kind = 1u;
  }
  out[j] = lp;
}

namespace {

VD double box_area(float lx, float ly, float lz, float hx, float hy, float hz) {
  const double dx = static_cast<double>(hx - lx), dy = static_cast<double>(hy - ly), dz = static_cast<double>(hz - lz);
  return dx * dy + dx * dz + dy * dz;
}

// what a child reference stands for in the sum: 0.5 for a node with children, the primitive count for a leaf - a
// chained leaf (uploaded trees: a reference to a record behind the tree's own) once, with its whole count
VD double ref_weight(uint32_t ref, uint32_t n_internal, const uint32_t* chain_leaf) {
  const uint32_t count = ref >> 25, idx = ref & kRefMask;
  if (count) return static_cast<double>(count);
  return idx >= n_internal ? static_cast<double>(chain_leaf[2u * (idx - n_internal) + 1u]) : 0.5;
}

// the workgroup's 256 values in a fixed order; the sum in sh[0]
VD void block_sum(double* sh, double v) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t o = kBlock / 2u; o; o >>= 1) {
    if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
}

}  // namespace

__global__ void __launch_bounds__(kBlock)
scene_bvh_cost_partial(const DScene d, uint32_t n_internal, const uint32_t* __restrict__ chain_leaf, double* __restrict__ partial) {
  __shared__ double sh[kBlock];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  double v = 0.0;
  if (i < n_internal) {
    const DNode n = flat(d.nodes)[i];
    v = box_area(n.a.x, n.a.y, n.a.z, n.a.w, n.b.x, n.b.y) * ref_weight(n.left_ref, n_internal, chain_leaf) +
        box_area(n.b.z, n.b.w, n.c.x, n.c.y, n.c.z, n.c.w) * ref_weight(n.right_ref, n_internal, chain_leaf);
  }
  block_sum(sh, v);
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

__global__ void __launch_bounds__(kBlock)
scene_bvh_cost_final(const DScene d, uint32_t n_internal, const uint32_t* __restrict__ chain_leaf, const double* __restrict__ partial,
                     uint32_t num_partial, double* __restrict__ cost) {
  __shared__ double sh[kBlock];
  double v = 0.0;
  for (uint32_t k = threadIdx.x; k < num_partial; k += kBlock) v += partial[k];
  block_sum(sh, v);
  if (threadIdx.x != 0) return;
  const double root = box_area(d.root_min[0], d.root_min[1], d.root_min[2], d.root_max[0], d.root_max[1], d.root_max[2]);
  *cost = (sh[0] + root * ref_weight(d.root_ref, n_internal, chain_leaf)) / root;
}

}  // namespace vimg

using namespace vimg;

extern "C" {

int vimg_hip_scene_rebuild_bvh(VimgDeviceScene* s, const VimgRebuildOptions* opts, void* stream) {
  if (!s) return fail(VIMG_E_INVALID, "rebuild_bvh: null scene");
  uint32_t builder = VIMG_BUILDER_PLOC;
  if (opts) {
    if (opts->struct_size < sizeof(VimgRebuildOptions)) return fail(VIMG_E_INVALID, "rebuild_bvh: struct_size too small");
    builder = opts->builder;
  }
  if (builder != VIMG_BUILDER_PLOC && builder != VIMG_BUILDER_LBVH) return fail(VIMG_E_INVALID, "rebuild_bvh: unknown builder");
  if (g_device < 0) return fail(VIMG_E_DEVICE, "rebuild_bvh: no device");
  hipStream_t st = stream_of(stream);
  const uint32_t n = s->num_leaf_prims;

  // 1. primitive bounds, after whatever the stream still holds; the builders run on the null stream
  DevBuf d_bounds;
  if (int rc = d_bounds.alloc(size_t(n) * 6 * sizeof(float))) return rc;
  hipLaunchKernelGGL(scene_rebuild_bounds, blocks_for(n), dim3(kBlock), 0, st, s->d, n, d_bounds.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));

  // 2. the tree, in the reference's layout, on the device
  DeviceTree tree;
  if (int rc = build_tree_device(builder, n, d_bounds.as<float>(), &tree)) return rc;   // (the builder's own message stands)
  if (tree.max_depth + 2 > 96) return fail(VIMG_E_INVALID, "rebuild_bvh: BVH deeper than the 94-level stack bound");
  const uint32_t num_nodes = tree.num_nodes;

  // 3. the device layout: every node with children at the count of such nodes before it
  DevBuf d_packed, d_scanned, d_scan_tmp, d_nodes, d_cls, d_slots;
  if (int rc = d_packed.alloc(size_t(num_nodes) * 8)) return rc;
  if (int rc = d_scanned.alloc(size_t(num_nodes) * 8)) return rc;
  size_t scan_bytes = 0;
  HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, d_packed.as<unsigned long long>(), d_scanned.as<unsigned long long>(), 0ull,
                                  num_nodes, rocprim::plus<unsigned long long>(), st));
  if (int rc = d_scan_tmp.alloc(std::max<size_t>(scan_bytes, 16))) return rc;
  hipLaunchKernelGGL(scene_rebuild_classify, blocks_for(num_nodes), dim3(kBlock), 0, st, tree.nodes.as<VimgBVHNode>(), num_nodes,
                     d_packed.as<unsigned long long>());
  HIP_TRY(rocprim::exclusive_scan(d_scan_tmp.p, scan_bytes, d_packed.as<unsigned long long>(), d_scanned.as<unsigned long long>(), 0ull,
                                  num_nodes, rocprim::plus<unsigned long long>(), st));
  unsigned long long last[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&last[0], d_scanned.as<unsigned long long>() + (num_nodes - 1u), 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&last[1], d_packed.as<unsigned long long>() + (num_nodes - 1u), 8, hipMemcpyDeviceToHost, st));
  VimgBVHNode root{};
  float root_rows[9];   // bb rows 0 and 2: the root's box
  HIP_TRY(hipMemcpyAsync(&root, tree.nodes.p, sizeof(root), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(root_rows, tree.bb.p, sizeof(root_rows), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const unsigned long long totals = last[0] + last[1];
  const uint32_t n_internal = static_cast<uint32_t>(totals & 0xffffffffull);
  if (totals >> 32) return fail(VIMG_E_UNSUPPORTED, "rebuild_bvh: a leaf of more than 127 primitives (chain records are not rebuilt)");
  std::vector<uint32_t> level_begin;
  uint32_t begin = 0;
  for (uint32_t c : tree.level_internal) level_begin.push_back(begin), begin += c;
  level_begin.push_back(begin);
  if (begin != n_internal || n_internal >= (1u << 25) || (root.obj_count == 0u) != (n_internal != 0u))
    return fail(VIMG_E_DEVICE, "rebuild_bvh: the builder's levels and its nodes disagree");
  const size_t node_bytes = std::max<size_t>(n_internal, 1) * sizeof(DNode);
  if (int rc = d_nodes.alloc(node_bytes)) return rc;
  if (n_internal)
    hipLaunchKernelGGL(scene_rebuild_nodes, blocks_for(num_nodes), dim3(kBlock), 0, st, tree.nodes.as<VimgBVHNode>(), tree.bb.as<float>(),
                       d_scanned.as<unsigned long long>(), num_nodes, n_internal, d_nodes.as<DNode>());

  // 4. the leaf slots in the new order (DTriShade, spheres, prims: by primitive, untouched)
  if (int rc = d_cls.alloc(size_t(n) * 4)) return rc;
  if (int rc = d_slots.alloc(size_t(n) * sizeof(DLeafPrim))) return rc;
  hipLaunchKernelGGL(scene_rebuild_cls, blocks_for(n), dim3(kBlock), 0, st, s->d, n, d_cls.as<uint32_t>());
  hipLaunchKernelGGL(scene_rebuild_slots, blocks_for(n), dim3(kBlock), 0, st, s->d, tree.obj_indices.as<uint32_t>(), d_cls.as<uint32_t>(), n,
                     d_slots.as<DLeafPrim>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));

  // 5. every step succeeded: swap, and drop what was derived from the old tree's shape
  // (a move frees what the scene held: the old records, the old slots, the chain-leaf table of an uploaded tree)
  DScene& d = s->d;
  s->total_bytes = s->total_bytes - s->nodes.bytes + node_bytes;
  s->nodes = std::move(d_nodes);
  s->leaf_prims = std::move(d_slots);
  s->chain_leaf = DevBuf{};
  d.nodes = (decltype(d.nodes))s->nodes.p;
  d.leaf_prims = (decltype(d.leaf_prims))s->leaf_prims.p;
  s->waves_per_simd = (s->total_bytes > (32u << 20)) ? 3 : 2;   // (the policy of the upload, on the bytes an upload would count)
  d.num_nodes = n_internal;
  d.max_depth = tree.max_depth;
  d.root_ref = root.obj_count == 0u ? 0u : ((root.obj_count << 25) | root.first_index);
  for (int a = 0; a < 3; ++a) d.root_min[a] = root_rows[a], d.root_max[a] = root_rows[6 + a];
  s->n_internal = n_internal;
  s->n_chain = 0;
  s->level_begin = std::move(level_begin);
  s->query_ready = false;   // the query LDS layout and blocks per CU depend on max_depth and num_nodes
  ++s->generation;
  return VIMG_OK;
}

int vimg_hip_scene_bvh_cost(VimgDeviceScene* s, void* stream, double* cost) {
  if (!s || !cost) return fail(VIMG_E_INVALID, "bvh_cost: null scene or result");
  if (g_device < 0) return fail(VIMG_E_DEVICE, "bvh_cost: no device");
  hipStream_t st = stream_of(stream);
  const uint32_t num_partial = (s->n_internal + kBlock - 1) / kBlock;
  DevBuf d_sums;   // the partial sums, then the result
  if (int rc = d_sums.alloc((size_t(num_partial) + 1) * sizeof(double))) return rc;
  if (num_partial)
    hipLaunchKernelGGL(scene_bvh_cost_partial, dim3(num_partial), dim3(kBlock), 0, st, s->d, s->n_internal, s->chain_leaf.as<const uint32_t>(),
                       d_sums.as<double>());
  hipLaunchKernelGGL(scene_bvh_cost_final, dim3(1), dim3(kBlock), 0, st, s->d, s->n_internal, s->chain_leaf.as<const uint32_t>(), d_sums.as<double>(),
                     num_partial, d_sums.as<double>() + num_partial);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(cost, d_sums.as<double>() + num_partial, sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return VIMG_OK;
}

}  // extern "C"
