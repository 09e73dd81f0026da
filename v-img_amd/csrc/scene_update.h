// Re-bake and refit of a resident scene (vimg_hip_scene_update_geometry): the kernels live in
// scene_update.hip, the ABI unit launches them through this one call.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "device_scene.h"

namespace vimg {

// What the upload recorded for a later refit, and the new positions of one update.
struct SceneUpdate {
  const float* vertices;        // num_vertices x 3 (device), or nullptr: DTriShade positions stay
  const float* spheres;         // num_spheres x 4 (device), or nullptr: d.spheres stays
  uint32_t num_tris, num_spheres;
  uint32_t num_slots;           // leaf slots (= primitives)
  uint32_t n_internal;          // the tree's own DNode records; chain records follow them
  uint32_t n_chain;             // chain records of leaves over 127 primitives
  const uint32_t* chain_leaf;   // per chain record {first slot, count} of its whole leaf (device)
  const uint32_t* level_begin;  // host: breadth-first levels of the internal nodes, level k = [level_begin[k], level_begin[k+1])
  uint32_t num_levels;
  float* root_box;              // device, 6 floats: root min xyz, max xyz
};

// Enqueues on `st`, in order: the triangle pass (positions, face normal, area pdf) when
// u.vertices is given, the sphere pass when u.spheres is given, the leaf-slot pass, the light
// pass, the chain records, one refit launch per level (deepest first), and the root box.
hipError_t enqueue_scene_update(const DScene& d, const SceneUpdate& u, hipStream_t st);

}  // namespace vimg
