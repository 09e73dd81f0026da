// Device-resident scene layout (gfx950).  Built once by vimg_hip_scene_upload from the VimgScene
// tables; every render reads only these arrays.
//
// Layout rules (DESIGN.md "Data layout in HBM"):
//  * everything a lane fetches in one step is one 16-byte-aligned record read with dwordx4 loads;
//    records that are always consumed together share a 64-byte line (BVH node = its own header +
//    both child boxes; leaf primitive = everything the intersection test needs);
//  * records are stored in the order traversal consumes them (leaf primitives in obj_indices
//    order, so a leaf's primitives are consecutive);
//  * the index chasing of the reference (obj_indices -> prims -> mesh -> indices -> vertices,
//    include/bvh.h:152, include/geometry/triangle.h:75-79) is resolved at upload time.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vimg_scene.h"
#include "material_record.h"

namespace vimg {

// Explicit address spaces: pointers that live inside a by-value kernel argument are otherwise
// generic and every access becomes a flat_* instruction (which also ties up the LDS counter).
#define VIMG_GLOBAL __attribute__((address_space(1)))
#define VIMG_LDS __attribute__((address_space(3)))
template <typename T>
using gptr = const VIMG_GLOBAL T*;
// builtin vector types (unlike HIP's float4 class) can be loaded from any address space
typedef float v4f __attribute__((ext_vector_type(4)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// One INTERNAL BVH node, 64 B: the boxes of both children exactly as BB_mins_maxes[2c+2 .. 2c+5]
// holds them (reference include/bvh.h:171-188) and a reference to each child.  A child
// reference packs "primitive count << 25 | index": count == 0 -> index of another DNode,
// count > 0 -> a leaf whose primitives are leaf_prims[index .. index+count).  Leaves therefore
// need no node record and no load of their own.
struct __attribute__((aligned(16))) DNode {
  v4f a;         // Lmin.x Lmin.y Lmin.z Lmax.x
  v4f b;         // Lmax.y Lmax.z Rmin.x Rmin.y
  v4f c;         // Rmin.z Rmax.x Rmax.y Rmax.z
  uint32_t left_ref, right_ref, pad0, pad1;
};
static_assert(sizeof(DNode) == 64, "DNode must be one 64-byte line");

// One leaf slot (position j of obj_indices), 48 B: all an intersection test reads.
//  kind 0 triangle : v = p0 p1 p2          kind 2 degenerate triangle (never hit,
//  kind 1 sphere   : v = centre, radius         include/geometry/triangle.h:86-92)
struct __attribute__((aligned(16))) DLeafPrim {
  v4f a, b;
  float c0;
  uint32_t prim;   // index into the reference's list_objects order
  uint32_t kind;
  uint32_t cls;    // material class of the primitive: 0 emitter, 1 Lambertian, 2 Principled, 3 other
};
static_assert(sizeof(DLeafPrim) == 48, "DLeafPrim must be 48 bytes");

// Per-triangle shading record, 64 B (positions again so hit_info needs no second indirection).
// `n` is normalize(cross(p1-p0, p2-p0)) — a function of the vertices only, evaluated once at
// upload with the float expression the reference evaluates per hit (src/geometry/triangle.cpp:25).
struct __attribute__((aligned(16))) DTriShade {
  float p[9];
  uint32_t mesh;
  uint32_t i0, i1, i2;   // global vertex ids (normals / uv lookup)
  float n[3];
};
static_assert(sizeof(DTriShade) == 64, "DTriShade must be 64 bytes");

// One emitter of GroupOfEmitters::list_of_emitters, 80 B: everything its sample() reads, in one fetch
// instead of the chase light -> primitive -> triangle / sphere -> mesh -> material (five dependent loads
// in front of every next-event estimate).
//  kind 0 background        kind 1 triangle without vertex normals: a b c = p0 p1 p2 n (the baked face normal)
//  kind 3 sphere: a = centre, radius      kind 2 triangle with vertex normals: sampled through the tables (index)
//  d = the material's emission (zero when it is no DiffuseLight), w = the triangle's area pdf
struct __attribute__((aligned(16))) DLight {
  v4f a, b, c, d;
  uint32_t kind, index, pad0, pad1;
};
static_assert(sizeof(DLight) == 80, "DLight must be 80 bytes");

struct DScene {
  // camera (TLCam members, reference src/tl_camera.cpp:6-23) — derived values computed on the host
  float cam_to_world[16];
  float p_size0, p_size1;
  float cone_spread;        // raycone_for_primary_ray(...) is a per-render constant
  float aperture_radius, focal_dist;
  int32_t res_x, res_y;

  // BVH
  float root_min[3], root_max[3];
  uint32_t num_nodes, max_depth;   // num_nodes = internal nodes
  uint32_t root_ref;               // packed reference of the root (a leaf for 1-node trees)
  gptr<DNode> nodes;
  gptr<DLeafPrim> leaf_prims;

  // primitives / shading data
  gptr<VimgPrim> prims;
  gptr<DTriShade> tri_shade;
  gptr<float> tri_area_pdf;   // 1 / (|cross(e2, e1)| / 2) per triangle (triangle.cpp:229-231,246)
  gptr<VimgMesh> meshes;
  gptr<float> normals;
  gptr<float> uvs;
  gptr<VimgSphere> spheres;
  gptr<VimgMaterial> materials;
  gptr<uint32_t> material_flags;   // MATF_* per material
  gptr<DMaterial> dmaterials;      // the same table, baked: 304 B per material (material_record.h, material_terms.h)
  gptr<VimgTexture> textures;
  gptr<float> texels;
  gptr<VimgTextureRG> rg_textures;
  gptr<float> rg_texels;
  gptr<VimgLight> lights;
  gptr<DLight> dlights;       // the same list, baked
  uint32_t num_lights;
  gptr<float> cdf_pool;
  VimgBackground background;
  uint32_t background_emissive;
};

// The launch-constant shading tables a small scene's launch serves from LDS (render_cu_kernel.h), in staging order.
// A row in LDS is the table's record, copied word for word; a VimgSphere (20 B) is padded to 32 B so that no row
// straddles a 16-byte boundary it need not.
enum : uint32_t {
  TAB_PRIMS = 0, TAB_TRI_SHADE, TAB_SPHERES, TAB_MATERIAL_FLAGS, TAB_MESHES,   // hit records
  TAB_MATERIALS, TAB_DMATERIALS,                                               // materials
  TAB_COUNT
};
struct __attribute__((aligned(16))) LSphere {   // VimgSphere's members under their names, one 32-byte row
  float center[3];
  float radius;
  uint32_t material;
  uint32_t pad[3];
};
static_assert(sizeof(LSphere) == 32, "LSphere must be 32 bytes");
// bytes of a table's row in LDS
__host__ __device__ constexpr uint32_t tab_row_bytes(uint32_t t) {
  return t == TAB_PRIMS ? uint32_t(sizeof(VimgPrim)) : t == TAB_TRI_SHADE ? uint32_t(sizeof(DTriShade)) :
         t == TAB_SPHERES ? uint32_t(sizeof(LSphere)) : t == TAB_MATERIAL_FLAGS ? 4u :
         t == TAB_MESHES ? uint32_t(sizeof(VimgMesh)) : t == TAB_MATERIALS ? uint32_t(sizeof(VimgMaterial)) :
         uint32_t(sizeof(DMaterial));
}

enum : uint32_t {
  MATF_NEEDS_UV = 1u,      // colour texture is not constant (checker / image) or RG / normal map
  MATF_NEEDS_FRAME = 2u,   // Principled: reads HitInfo::n_frame
};

struct RenderArgs {
  uint32_t integrator, samples, depth;
  uint32_t tile_rank, tile_world;
  uint32_t tiles_x, tiles_y;        // ceil(W/8), ceil(H/8)
  uint32_t num_local_tiles;
  uint32_t full_stats;
  uint32_t stack_entries;           // per-lane LDS stack depth (max_depth + 2)
  uint32_t lds_nodes;               // number of top-of-tree nodes staged into LDS
  // (the pool_* and stack_* fields below are read by the CU scheduler only; the lane-bound kernel's launches leave them 0)
  uint32_t stack_lds;               // deep trees: stack entries kept in LDS (== stack_entries: all of them);
                                    // the LDS stack then has stack_lds + 1 rows (the last one takes the writes above)
  VIMG_GLOBAL uint32_t* stack_ovf;  // the entries beyond, per walking wave of the grid [entry - stack_lds][lane] (scene-owned scratch)
  VIMG_GLOBAL v4u* pool_cold;       // cold slot records, one region per workgroup (scene-owned scratch)
  uint32_t lds_leaf;                // number of leaf records copied to LDS (all or 0)
  VIMG_GLOBAL v4u* pool_state;      // per work item {rng lo, rng hi, epoch + segments done, -}{acc.xyz, -}
  uint32_t pool_segments;           // segments a pixel's samples are split into (>= 1)
  uint32_t pool_seg_len;            // samples per segment
  uint32_t pool_epoch;              // tag base of this launch (stale records of earlier launches never match)
  uint32_t pool_slots;              // path slots per workgroup (0 = lane-bound kernel)
  uint32_t pool_refill;             // finished rays of a walking wave that trigger hand-over and refill
  uint32_t pool_vbatch;             // queued slots of one class that start a vertex batch
  uint32_t pool_boxmin;             // leave the box loop when fewer lanes than this still descend (0 = never)
  uint32_t pool_starve;             // smallest partial vertex batch a wave takes at once
  uint32_t pool_gbreak;             // unused (a retired scheduler's; kept for the layout)
  uint32_t pool_classes;            // vertex queues: 1 = one, 2 = Principled apart, 3 = + Lambertian apart
  uint32_t cu_walkers;              // CU scheduler: waves [0, cu_walkers) own traversal stacks and walk; the others only shade
  uint32_t cu_flex;                 // CU scheduler: bit 0 = a walking wave that holds no ray may run a vertex batch
  uint32_t cu_lowwater;             // CU scheduler: partial vertex batches only while fewer rays than this wait in the walk ring
  uint32_t cu_patience;             // CU scheduler: looks in vain after which a wave takes a partial batch of any size
  uint32_t cu_join;                 // CU scheduler: queued rays at which a walking wave that holds none starts to walk (fewer: after cu_patience looks)
  uint32_t cu_sleep;                // CU scheduler: s_sleep argument of a wave that found nothing to do
  uint32_t cu_watchdog;             // CU scheduler: a wave idle for longer than this (2^20 ticks of the 100 MHz clock) while slots are live gives up
  uint32_t cu_magic_v, cu_shift_v;  // CU scheduler: n / pool_slots == mulhi(n, magic) >> shift (n < 2^31)
  uint32_t cu_magic_w, cu_shift_w;  // ... n / (2 * pool_slots)
  int32_t single_x, single_y;       // trace_pixel mode when >= 0
  // progressive rendering (vimg_hip_progressive_render): the launch adds `samples` to pixels that already had
  // `sample_base`; segment 0 of a pixel starts from its record in prog_in when sample_base > 0, and the pixel's
  // last sample writes its record to prog_out.  Ordinary launches: 0, float(samples), nullptr, nullptr
  uint32_t sample_base;             // samples per pixel before this launch (the R2 jitter index is absolute)
  float spp_div;                    // static_cast<float>(sample_base + samples): the divisor of the mean
  const VIMG_GLOBAL v4u* prog_in;   // per work item {rng lo, rng hi, -, -}{acc.xyz, -}, in the launch's item order
  VIMG_GLOBAL v4u* prog_out;        // the same records after this launch (another buffer: a failed launch leaves prog_in as it was)
  // masked progressive launches (vimg_hip_progressive_render_masked, progressive_adaptive.hip): the work items of
  // the launch are item_list[0 .. item_count), ascending; a claim's index is looked up there and everything
  // else (pixel, records, output offset) goes by the item found.  Other launches: nullptr, 0
  const VIMG_GLOBAL uint32_t* item_list;
  uint32_t item_count;
  // CU scheduler: the launch-constant shading tables each workgroup copies to LDS behind its leaf records when the
  // launch starts (render_cu_kernel.h: stage_tables).  lds_tables: the groups staged (plain_build.h: PF_TAB_*), each
  // whole or not at all, 0 = none; tab_off / tab_rows: of every table of a staged group, its byte offset from the
  // start of the workgroup's dynamic LDS (a multiple of 16) and its rows
  uint32_t lds_tables;
  uint32_t tab_off[TAB_COUNT], tab_rows[TAB_COUNT];
  // CU scheduler: the leaf records once more for the rays of major axis kz == 0 and kz == 1, triangles' vertices
  // permuted as the watertight test permutes them, staged behind the tables when the launch starts (render_cu_kernel.h:
  // stage_leaf_perm; the leaf table itself serves kz == 2).  leaf_perm: 1 = a build that folds PF_LEAF_PERM may run
  // (both copies staged, or a scene without triangles, which needs none).  Copy k starts leaf_perm_off + k *
  // leaf_perm_stride bytes behind the start of the leaf table; a scene without triangles has 0 and 0: every "copy"
  // is the leaf table, and nothing more is laid out
  uint32_t leaf_perm, leaf_perm_off, leaf_perm_stride;
};

struct DeviceStats {
  unsigned long long closest, shadow, internal, leaf, prim, sphere, nan_samples;
  unsigned long long trip_descend, trip_prim, iterations;   // wave-level loop trips (diagnostic)
  // render_cu_kernel, statistics launches: per stage cycles [0..5], batches [6..9], waves [10] and the batches' slots [11..14];
  // shadow rays whose light sample adds exactly zero, which a late build does not queue [15];
  // the walk's passes, rounds, sessions and refills [16..22]; looks for work and the ring counts seen [23..27]
  unsigned long long prof[28];
  unsigned long long wait_cyc[5], wait_n[5];   // render_cu_kernel, statistics launches: cycles slots waited in the rings (vertex 0-3, walk), and how many
  unsigned long long px_done[3];    // render_cu_kernel, statistics launches: when pixels finished (10 ns ticks since their workgroup started): sum, count, latest
  unsigned long long px_hops[3];    // ... vertex-stage visits per pixel (whole segments only): sum, largest, and (finish time << 24 | hops) of the last pixel
  unsigned long long ray_cyc[2];    // ... cycles rays spent in a walking lane (pop to hand-over): sum, count
  unsigned long long pv_cyc[7];     // ... Principled batches: cycles in state loads, hit record + path logic, light sample, BSDF sample, evaluations, stores + hand-over; batches
  unsigned long long walk_cyc[4];   // render_cu_kernel, statistics launches: cycles of the walk sessions in refill + set-up, box loop, leaf rounds, hand-over
};

}  // namespace vimg
