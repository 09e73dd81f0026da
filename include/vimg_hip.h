/*
 * vimg_hip.h — C ABI of libvimg_hip.so, the MI355X (gfx950) implementation of v-img's hot path.
 *
 * The reference has no FFI; its narrowest seam is the template call
 *   std::vector<glm::vec3> scene_integrator(render_data, bvh, prims, lights, integrator)
 *   (reference include/integrators.h:36-153, called from src/main.cpp:219-248)
 * and its single-pixel twin trace_pixel (include/integrators.h:181-220, src/main.cpp:257-298).
 * The entry points below replace exactly those two calls; INTEGRATION.md shows the binding a
 * maintainer adds on the reference side.  Plain pointers and sizes only.
 *
 * Conventions: every function returns 0 on success and a negative VIMG_E_* code on failure;
 * vimg_hip_last_error() returns the message for the calling thread's last failure.  Nothing
 * throws across the ABI.  One device context per process (one process per GPU).
 */
#ifndef VIMG_HIP_H
#define VIMG_HIP_H

#include "vimg_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  VIMG_OK = 0,
  VIMG_E_INVALID = -1,     /* bad argument / inconsistent scene tables */
  VIMG_E_DEVICE = -2,      /* HIP runtime error (no device, allocation, launch) */
  VIMG_E_UNSUPPORTED = -3  /* feature outside what the path reproduces */
};

typedef struct VimgDeviceScene VimgDeviceScene;   /* opaque: device-resident scene */

/* Selects the GPU for this process (hipSetDevice) and creates the render stream. */
int vimg_hip_init(int device_ordinal);

/* Number of visible HIP devices, or a negative error code. */
int vimg_hip_device_count(void);

/* How a scene's frames are scheduled on the GPU.  Every field: VIMG_OPT_AUTO (-1) = the library's
 * policy (stated per field); the schedulers execute the same per-path arithmetic and give
 * the same bits.  The reference has no counterpart (its scheduler is the tile loop of
 * include/integrators.h:57-101); these are the knobs of OUR replacement of that loop, at the
 * boundary instead of in the environment.  (For tools/ only, VIMG_HIP_* environment variables
 * still override single fields at upload: scheduler VIMG_HIP_SCHED=cu|lane, the others as named in
 * scene_upload.hip:options_from_env.) */
#define VIMG_OPT_AUTO (-1)
enum {
  VIMG_SCHED_LANE = 1,   /* render_kernel: one path per lane, persistent waves */
  /* 2-5: retired.  The schedulers of rounds 1 and 2 were removed from the library; the values keep their
   * places for older callers, and an upload that names one answers VIMG_E_UNSUPPORTED */
  VIMG_SCHED_POOL = 2,
  VIMG_SCHED_STAGE = 3,
  VIMG_SCHED_POOL4 = 4,
  VIMG_SCHED_POOL4G = 5,
  VIMG_SCHED_CU = 6      /* render_cu_kernel: one pool per compute unit, walking and shading waves, lock-free rings in LDS, both rays of a vertex walked at once */
};
typedef struct VimgHipOptions {
  uint32_t struct_size;       /* sizeof(VimgHipOptions): lets the library accept older callers */
  int32_t scheduler;          /* AUTO (launch_policy.hip:make_launch): CU for every launch; LANE for frames wider than 65 535 pixels */
  int32_t waves_per_simd;     /* LANE: register budget, 2 or 3.  AUTO: 3 for scenes > 32 MiB else 2.  (CU is built for 4) */
  int32_t lds_budget_kb;      /* LANE: LDS per workgroup for the top of the tree and the stacks, AUTO 40.  CU: LDS for the top of the tree alone, AUTO 4.5; a value no launch fits beside is VIMG_E_INVALID at the render */
  int32_t pool_slots;         /* CU: path slots per compute unit.  AUTO: what the CU's LDS holds, <= 1280 on trees in LDS, pixels / 2.7 on launches of 1 to 2.7 pools' worth of pixels, never more than pixels per CU + 8 */
  int32_t pool_segments;      /* CU: segments a pixel's samples are cut into.  AUTO: ~176 / pool generations of the launch, <= 64 and <= samples / 4; 1 on launches of ten generations or more */
  int32_t pool_refill;        /* CU: finished rays of a walking wave that trigger hand-over and refill.  AUTO 16; on trees in global memory 2 */
  int32_t pool_vbatch;        /* CU: queued slots of one class that start a vertex batch, 1..64.  AUTO 64 */
  int32_t pool_classes;       /* CU: vertex queues by material, 1..3.  AUTO 3 */
  int32_t pool_starve;        /* CU: smallest partial vertex batch a wave takes at once.  AUTO 16 */
  int32_t pool_boxmin;        /* CU, trees in global memory: leave the box loop below this many descending lanes.  AUTO 16; 8 on launches whose pixels all own a slot */
  int32_t lds_leaf;           /* CU: 0 = never copy the leaf records to LDS.  AUTO: when they fit 4 KiB */
  int32_t stage_slots;        /* accepted and ignored (read by a retired scheduler only) */
  int32_t stage_seg_len;      /* accepted and ignored */
  int32_t stage_wchunk;       /* accepted and ignored */
  int32_t stage_walk_quota;   /* accepted and ignored */
  int32_t pool4_rays;         /* accepted and ignored */
  int32_t lds_stack;          /* CU: entries of a lane's traversal stack kept in LDS, the rest in global memory.  AUTO 32 (fewer where the LDS asks for it); a value no launch fits is VIMG_E_INVALID at the render */
  int32_t pool_gbreak;        /* accepted and ignored */
  int32_t cu_waves;           /* CU: reserved; one 16-wave workgroup is a whole compute unit (12 waves at 168 registers measured slower) */
  int32_t cu_walkers;         /* CU: waves of the 16 that walk (the rest only shade).  AUTO: 8 on trees in LDS, 10 on trees in global memory, all 16 when every pixel of the launch owns a slot (tree in LDS) */
  int32_t cu_flex;            /* CU: bit 0: a walking wave that holds no ray may run a vertex batch; bit 4 (16): no split batches (the two BSDF evaluations of a vertex on the two halves of the wave when a batch has <= 32 slots); bit 5 (32): EARLY rays - a vertex stage queues its shadow ray right after the light sample and its path ray right after the BSDF sample and finishes (evaluations, stores) beside their walks; bits 1, 2: shading / walking at wave priority 1 (measurements).  AUTO 1, + 32 on launches of fewer than three pools' worth of pixels and on trees in global memory */
  int32_t cu_lowwater;        /* CU: partial vertex batches run only while fewer rays than this wait in the walk ring.  AUTO 64 */
  int32_t cu_patience;        /* CU: looks in vain after which a wave takes a partial batch of any size.  AUTO 4 */
  int32_t cu_join;            /* CU: queued rays at which a walking wave that holds no ray starts to walk (fewer: after cu_patience looks).  AUTO 1 */
  int32_t cu_sleep;           /* CU: s_sleep argument (64 cycles each) of a wave that found nothing to do.  AUTO 4 */
} VimgHipOptions;
/* Fills every field with VIMG_OPT_AUTO (and struct_size). */
void vimg_hip_options_default(VimgHipOptions* opts);

/* Validates the tables of `scene` (index ranges, BVH child ranges, stack bound), bakes them
 * into the device layout described in DESIGN.md and copies them to HBM.  The host arrays may
 * be freed afterwards.  Replaces nothing in the reference (its scene is already in RAM); it is
 * the "load once" half of the seam so that the timed render starts with inputs resident.
 * `opts` may be NULL (= all AUTO); vimg_hip_scene_upload(scene, out) is that case. */
int vimg_hip_scene_upload(const VimgScene* scene, VimgDeviceScene** out);
int vimg_hip_scene_upload_opts(const VimgScene* scene, const VimgHipOptions* opts, VimgDeviceScene** out);
int vimg_hip_scene_free(VimgDeviceScene* scene);

/* Changing a resident scene without a new upload: the same primitive set, texture sizes
 * and resolution; new positions, materials, texture contents, emitters, background and camera (and, below, a new
 * tree).  vimg_hip_scene_update_geometry is the scene's update entry point: one call carries any of the changes.
 *  _update_geometry : new positions, NULL = unchanged.  DEVICE pointers to float32, read on `stream`:
 *      vertices num_vertices x 3 (the whole table, VimgScene order), normals num_vertices x 3 (rows of
 *      meshes without normals are ignored), spheres num_spheres x 4 (centre xyz, radius; the material
 *      stays).  Bakes again everything the upload derives from positions - triangle records, face
 *      normals, area pdfs, leaf records and their degenerate flag, emitters - and refits the tree's boxes
 *      bottom-up in its existing topology, all in kernels with the upload's float expressions and the host
 *      builders' fold order; then blocks until the scene is consistent (the inputs may be reused at once).
 *      A launch afterwards reads exactly what an upload of the host scene with the same positions and a
 *      vimg_host_refit_bvh tree reads.  Values are taken as they come (no finiteness check).
 *    The fields behind `spheres` (since the material update; struct_size tells the library whether the caller
 *    has them) change what the upload takes from the material, texture, light and background tables; NULL / 0 =
 *    unchanged, and a call with all of them zero is the geometry update above.  Applied after the positions, in
 *    the order images, tables, lights; afterwards a launch reads exactly what an upload of the host scene edited
 *    the same way (vimg_host_set_materials, _set_texture_colors, _set_texture_image, _set_background) reads,
 *    vimg_hip_scene_bytes included:
 *      materials  : the whole table, as many records as uploaded; any field may change, the type included.  The
 *                   upload's checks apply.  material_flags, the class of every leaf slot, the emission of every
 *                   emitter (zero when its primitive's material is no DiffuseLight any more: it is still sampled)
 *                   and the TEX / non-TEX kernel family are derived again.
 *      textures   : the whole record table.  A record keeps its type; an IMAGE record keeps everything (its size,
 *                   levels, offsets and wrap modes); CONST may change col_a, CHECKER both colours and cell counts.
 *      lights     : with set_lights != 0 a new emitter list of num_lights entries (0: a scene without emitters,
 *                   which, like an upload without emitters, the mis integrator refuses and the others render);
 *                   prim < num_prims, at most one BACKGROUND entry.  Baked by a kernel from the resident records.
 *      background : keeps type, env_tex and both CDF offsets; col, radiance_scale and the two matrices may change.
 *      images     : new level-0 texels of IMAGE textures, from DEVICE memory; the mip chain is filtered again in
 *                   place, and for the background's env_tex the sampling CDFs too, device to device.
 *  _set_camera : the camera values the upload derives (pixel size, primary-ray cone, lens).  A different
 *      res_x / res_y is VIMG_E_INVALID.
 * Both change the scene's generation, once per successful call: a VimgProgressive whose records were made before
 * refuses its next increment (VIMG_E_INVALID) until vimg_hip_progressive_reset.  Argument errors (NULL, a
 * struct_size that is neither 32 - the layout before the material update - nor at least sizeof(VimgGeometryUpdate),
 * a table the upload would refuse, a record that changes what must stay) return VIMG_E_INVALID before anything is
 * enqueued or written and leave the scene and its generation as they were.  Launches on the scene stay ordered on
 * one stream, as for every launch of a scene. */
typedef struct VimgTextureImage {
  uint32_t texture;         /* index of a resident IMAGE texture */
  uint32_t reserved;
  const void* level0;       /* DEVICE pointer: width * height float32 rgb triples, row 0 = top; 4-byte aligned */
} VimgTextureImage;
typedef struct VimgGeometryUpdate {
  uint32_t struct_size;     /* sizeof(VimgGeometryUpdate), or 32: the first four fields only */
  const void* vertices;     /* num_vertices x 3, or NULL */
  const void* normals;      /* num_vertices x 3, or NULL */
  const void* spheres;      /* num_spheres x 4, or NULL */
  /* since the material update; HOST pointers unless said otherwise; NULL / 0 = unchanged */
  const VimgMaterial* materials;      /* the whole table, num_materials records as uploaded */
  const VimgTexture* textures;        /* the whole record table, num_textures records */
  const VimgLight* lights;            /* a new emitter list of num_lights entries, read when set_lights != 0 */
  uint32_t num_lights, set_lights;    /* (set_lights != 0 with num_lights == 0: a scene without emitters) */
  const VimgBackground* background;
  const VimgTextureImage* images;     /* host array of num_images entries; each level0 is a DEVICE pointer */
  uint32_t num_images, reserved;
} VimgGeometryUpdate;
#define VIMG_GEOMETRY_UPDATE_V1_SIZE 32u
int vimg_hip_scene_update_geometry(VimgDeviceScene* scene, const VimgGeometryUpdate* update, void* stream);
int vimg_hip_scene_set_camera(VimgDeviceScene* scene, const VimgCamera* camera);

/* A new tree for a resident scene: what a refit cannot give after a large deformation.
 *  _rebuild_bvh : builds a BVH over the scene's primitives as they now stand (after any _update_geometry) with
 *      the PLOC builder (opts NULL, or builder VIMG_BUILDER_PLOC) or the LBVH, and bakes the device layout from
 *      it, all in kernels on resident data: primitive bounds from the triangle records and spheres, the builder's
 *      core, node records, leaf slots in the new order.  The host only reads the builders' per-round / per-level
 *      counters.  Afterwards a launch reads exactly the bytes vimg_hip_scene_upload gives for the host scene with
 *      the same positions whose tree vimg_host_build_bvh_with(vimg_hip_build_ploc) (resp. _lbvh) built: image,
 *      event counts, heatmap, trace_pixel and ray queries are that upload's, and so is vimg_hip_scene_bytes.
 *      Blocking; ordered after the work already on `stream` (NULL = the library's).  Changes the scene's
 *      generation like _update_geometry.  The tree is built beside the old one and swapped in when every step
 *      has succeeded: a failed call (VIMG_E_DEVICE, a tree beyond the 94-level stack bound, VIMG_E_UNSUPPORTED
 *      for a leaf over 127 primitives - the builders end theirs at 8) leaves the scene as it was, generation
 *      included.  A NULL scene, a struct_size below sizeof(VimgRebuildOptions) or an unknown builder are
 *      VIMG_E_INVALID, found before anything is enqueued.
 *  _bvh_cost : the surface-area cost of the scene's tree under the reference's model (include/bvh.h:17-20:
 *      traversal 0.5, intersection 1): the sum over nodes of area x (0.5 for a node with children, its primitive
 *      count for a leaf) over the root's area, area = dx dy + dx dz + dy dz of the float32 extents, summed in
 *      float64 in a fixed order (the same scene gives the same bits).  It rises when a refit stretches a tree
 *      over moved geometry and falls back with a rebuild.  Blocking; reads only the tree. */
enum { VIMG_BUILDER_PLOC = 0, VIMG_BUILDER_LBVH = 1 };
typedef struct VimgRebuildOptions {
  uint32_t struct_size;     /* sizeof(VimgRebuildOptions) */
  uint32_t builder;         /* VIMG_BUILDER_* */
} VimgRebuildOptions;
int vimg_hip_scene_rebuild_bvh(VimgDeviceScene* scene, const VimgRebuildOptions* opts, void* stream);
int vimg_hip_scene_bvh_cost(VimgDeviceScene* scene, void* stream, double* cost);

/* Ray queries on a resident scene: the render's own walk on rays the caller gives.
 *  _trace_rays  : closest hit, exactly what the render's walk (traverse<false>: the same slab, triangle and
 *      sphere expressions, the same tie rule) computes for a ray with that [t_min, t_max].  d_hits: n VimgRayHit
 *      - t the hit distance, prim an index into VimgScene.prims, b1 b2 the weights of a triangle's 2nd and 3rd
 *      vertex (e1 * inv_det, e2 * inv_det as tri_hit_info forms them; 0 for spheres).  A miss writes t = +inf,
 *      prim = VIMG_NO_HIT, b1 = b2 = 0.  d_info (may be NULL): n VimgHitInfo, the hit's full record
 *      (make_hit_info<true>, what the parity probe returns): position, shading and geometric normal, uv,
 *      material; zeros for a miss.
 *  _occluded    : the render's shadow test (traverse<true>) over [t_min, t_max]: d_flags[i] = 1 when anything
 *      is hit, else 0.
 *  _camera_rays : the camera's generate_ray (as the render and the image use it; the one _set_camera sets) for
 *      n samples {x, y, lens_u, lens_v} of float32 (pixel coordinates, lens samples in [0, 1)): n VimgRay with
 *      t_min = 0.0001f, t_max = +inf.  Picking = _camera_rays, then _trace_rays.
 * All three only enqueue on `stream` (NULL = the library's stream): no allocation, no host wait.  They read the
 * scene and nothing else (none of its render scratch), so they may sit between renders and progressive
 * increments without changing those results or the scene's generation; a call after _update_geometry returns
 * sees the new geometry.  Buffers are DEVICE pointers, 16-byte aligned (d_flags: any alignment).  n == 0 does
 * nothing; n >= 2^32, a NULL scene, a NULL buffer with n > 0 or a misaligned buffer are VIMG_E_INVALID, found
 * before anything is enqueued (also without a GPU).  A ray with t_min > t_max or a NaN in its range is a miss,
 * not an error. */
typedef struct VimgRay { float org[3]; float t_min; float dir[3]; float t_max; } VimgRay;             /* 32 B */
typedef struct VimgRayHit { float t; uint32_t prim; float b1, b2; } VimgRayHit;                       /* 16 B */
typedef struct VimgHitInfo { float p[3]; float ns[3]; float ng[3]; float uv[2]; uint32_t mat; } VimgHitInfo;   /* 48 B */
#define VIMG_NO_HIT 0xffffffffu
int vimg_hip_trace_rays(VimgDeviceScene* scene, const void* d_rays, uint64_t n, void* d_hits, void* d_info,
                        void* stream);
int vimg_hip_occluded(VimgDeviceScene* scene, const void* d_rays, uint64_t n, uint8_t* d_flags, void* stream);
int vimg_hip_camera_rays(VimgDeviceScene* scene, const void* d_samples, uint64_t n, void* d_rays, void* stream);

/* Number of float triples a shard's compact framebuffer holds
 * (= 64 * number of 8x8 tiles owned by tile_rank). */
int64_t vimg_hip_shard_pixels(const VimgDeviceScene* scene, const VimgRenderParams* params);

/* scene_integrator (reference include/integrators.h:36-153) with any of the four integrators
 * of integrator_func: s_normal, g_normal, material (src/integrators/mat_integrator.cpp), mis.
 *  d_out_rgb : DEVICE pointer.
 *      tile_world == 1: W*H float triples, linear radiance, index x + (H-1-y)*W, i.e. exactly
 *                       the reference's image_accumulated vector (include/integrators.h:113,137).
 *      tile_world  > 1: the shard's compact buffer, vimg_hip_shard_pixels() triples, tile-major
 *                       ([local_tile][ty*8+tx]); assemble with vimg_hip_assemble_shards().
 *  stream    : a hipStream_t cast to void*, or NULL for the library's own stream.
 *  stats     : optional HOST pointer, filled when the call returns.
 * The call enqueues the kernels and waits for them (the reference call is blocking too).
 * Limit of one launch: the rings of a compute unit count the rays it queues in 32 bits - about 2^31 per
 * launch, i.e. the whole 1800x800 frame of disney_spheres up to ~60 000 samples per pixel (the reference's
 * scenes ask for 512-2048); beyond it the launch ends with VIMG_E_DEVICE and says so.  More samples than
 * that: render the frame progressively (below), where the limit holds per increment.
 *
 * The first-hit feature integrators VIMG_INTEGRATOR_ALBEDO .. _COVERAGE (include/vimg_scene.h) render what a
 * denoiser or compositor needs beside the image, through this and every other entry point that takes
 * VimgRenderParams (render_async, render_to_host, trace_pixel, shards, the progressive calls, masked or not).
 * Their samples are the normal integrators': the pixel's PCG stream seeded with the image index, the jitter
 * random_x_y_r2(px + py + k), the lens draws, one closest-hit walk of the camera ray over [1e-4, inf) - the rays
 * of s_normal, and of _camera_rays + _trace_rays given the same samples.  A pixel is the float32 sum of its
 * samples' values in sample order, divided once by float(samples); a miss contributes 0 0 0.  On a hit:
 *   ALBEDO    the material's base colour at the hit:
 *               Lambertian, Principled  their colour texture (VimgMaterial.tex) evaluated as the MIS integrator's
 *                                       first vertex evaluates it: col_at_ray_hit with the primary ray's direction
 *                                       and the cone {width |spread * distance|, angle spread + 2 * surface spread}
 *                                       the camera's cone {0, pixel spread} becomes at the hit (mip level of image
 *                                       textures; constant and checkerboard textures do not read it)
 *               Dielectric              1 1 1
 *               DiffuseLight            its emission colour (VimgMaterial.emit), whichever side is seen
 *   NORMAL    the shading normal as it is (VimgHitInfo.ns: normal-mapped where the material has a map), not (n+1)/2
 *   DEPTH     t t t, the distance along the camera ray (VimgRayHit.t)
 *   POSITION  the hit point (VimgHitInfo.p)
 *   UV        u v 0 (VimgHitInfo.uv: the colour texture's set, barycentrics on a mesh without one)
 *   COVERAGE  1 1 1
 * `depth` is not read, a scene without lights is accepted, and VimgHipOptions.scheduler is not read: these
 * integrators have one kernel (vimg_hip_launch_kernel names it).  Statistics: paths = closest_rays = pixels x
 * samples, shadow_rays = 0, and the traversal counts of an s_normal launch of the same frame. */
int vimg_hip_render(VimgDeviceScene* scene, const VimgRenderParams* params, void* d_out_rgb,
                    void* stream, VimgRenderStats* stats);

/* Progressive rendering: one frame (or shard) of `scene` rendered a few samples at a time.  An accumulator
 * is bound to one scene and one set of parameters: integrator, depth, tile_rank and tile_world are fixed
 * for its life, params->samples is ignored.  It keeps a 32-byte record per pixel of the launch (the RNG
 * state and the float sum - and the pixel's count and statistics, see adaptive sampling below - in the compact
 * tile-major order of shards; twice, so that a failed increment leaves the last good state).
 * Contract: increments n_1 .. n_k give, after each one, exactly the bits vimg_hip_render gives at
 * samples = n_1 + .. + n_i - the same per-pixel PCG stream, the same jitter index, the same division -
 * for every integrator, every shard and every scheduler configuration of this library.
 *  _render  : adds `samples` samples to every pixel and writes the running mean in vimg_hip_render's
 *             layout to d_out_rgb (DEVICE; NULL = advance only).  Blocks like vimg_hip_render and reads
 *             the scene's error word; the accumulator advances only when the launch succeeded.  stats
 *             (HOST, optional) = this increment's events.  VIMG_E_INVALID for samples == 0, a running
 *             total beyond UINT32_MAX (the reference's sample count is 32-bit), another scene than the
 *             accumulator's, NULL arguments.  The 2^31-ray limit of vimg_hip_render holds per increment.
 *  _samples : samples per pixel so far (0 for NULL);  _reset: back to 0 (the next increment seeds again).
 * Accumulators on the same scene are independent (each launch owns the scene's scratch while it runs);
 * free them before their scene. */
typedef struct VimgProgressive VimgProgressive;   /* opaque */
int vimg_hip_progressive_create(VimgDeviceScene* scene, const VimgRenderParams* params, VimgProgressive** out);
int vimg_hip_progressive_render(VimgDeviceScene* scene, VimgProgressive* acc, uint32_t samples,
                                void* d_out_rgb, void* stream, VimgRenderStats* stats);
uint64_t vimg_hip_progressive_samples(const VimgProgressive* acc);
int vimg_hip_progressive_reset(VimgProgressive* acc);
int vimg_hip_progressive_free(VimgProgressive* acc);

/* Adaptive sampling on an accumulator: increments that reach only some pixels, and a per-pixel
 * error to choose them by.  The accumulator keeps, in the three spare words of its 32-byte record, each pixel's
 * count N, the number K of increments it has taken part in, and M2 (below).  Per-pixel buffers are DEVICE pointers
 * in the pixel order of d_out_rgb for the accumulator: the image layout (x + (H-1-y)*W) for tile_world == 1, the
 * compact tile-major layout of the shard otherwise (off-image slots of ragged tiles: never selected, count 0).
 *  _render_masked : adds `samples` samples to exactly the pixels whose d_mask byte (uint8) is non-zero, then
 *      writes EVERY pixel's mean to d_out_rgb (NULL = advance only).  d_mask == NULL selects every pixel; on an
 *      accumulator whose pixels all stand at one count that is vimg_hip_progressive_render itself, the same single
 *      launch over every item (plus the pass that keeps N, K and M2).  Masked and unmasked calls follow each
 *      other in any order.
 *      Contract: after any sequence of calls a pixel whose count is N carries exactly the bits vimg_hip_render
 *      gives that pixel at samples = N - its PCG stream goes on from its record, the jitter index of a sample is
 *      px + py + (N before the call) + its number within the call, the mean is one division sum / float(N) - for
 *      all four integrators, every shard and every scheduler configuration.  A pixel at N == 0 is written 0 0 0.
 *      Cost: the sample base is a constant of a launch, so the selected pixels are rendered one launch per
 *      DISTINCT COUNT among them, in ascending count, each over the compacted list of its pixels and each with
 *      the ~1.6 ms tail of a launch; each class also costs one 16-byte read-back.  The adaptive
 *      loop (select, then a masked increment) only ever has one class.
 *      All or nothing: every launch writes the accumulator's other buffer; buffers, counts, statistics and
 *      _launches advance only when every launch succeeded and the scene's error word is clean, otherwise the
 *      accumulator stays at its last good state.  VIMG_E_INVALID, found before anything is enqueued and with
 *      the accumulator untouched: samples == 0, NULL scene or accumulator, another scene's accumulator, a
 *      scene changed since the records were made (reset first), a selected pixel whose count would pass
 *      UINT32_MAX.  (The last one is decided on the host from the largest count of any pixel; only when THAT
 *      would pass the bound does it depend on which pixels the device mask selects, and the largest selected
 *      count is then read back - two read-only kernels and 4 bytes - before any render launch.)  stats (HOST, optional): the events of this call's launches, summed; paths =
 *      selected pixels x samples.
 *  _samples (above) : every pixel's count while all pixels stand at one; after masked calls the largest count.
 *  _launches : render launches of the successful calls since creation or the last reset.
 *  _state : the records, each buffer optional (NULL): d_sum_rgb 3 float32 per pixel (the running sums), d_count
 *      uint32 N, d_batches uint32 K, d_m2 float32 M2.  Only enqueues on `stream`.
 *  _error : one float32 per pixel, the estimated relative standard error of the pixel's mean luminance (err
 *      below; +inf while K < 2).  Only enqueues.
 *  _select : d_mask (uint8 per pixel) = 1 where (err > target && N < max_samples) || K < 2, else 0; *active_out
 *      (HOST) = the number of ones, one 4-byte read-back after which the call returns.  target must be >= 0.
 * The statistic, in float32 with IEEE +, -, *, /, sqrt and no fused multiply-add, evaluated in the order written
 * (a numpy float32 restatement gives the same bits).  Y(v) = v.x * 0.212671f + v.y * 0.715160f + v.z * 0.072169f,
 * the luminance of the post chain's Reinhard operator.  An increment of n samples takes a selected pixel's sums
 * from S to S', its count from N to N' = N + n:
 *      b     = Y(S' - S) / float(n)                    (the increment's batch mean; S' - S per component)
 *      m_old = N ? Y(S) / float(N) : 0                 m_new = Y(S') / float(N')
 *      M2'   = M2 + float(n) * (b - m_old) * (b - m_new)       ((float(n) * (b - m_old)) * (b - m_new))
 *      K'    = K + 1
 *      err   = K < 2 ? +inf : sqrt((M2 < 0 ? 0 : M2) / float(K - 1) / float(N)) / (fabs(Y(S) / float(N)) + 1e-3f)
 * vimg_hip_progressive_reset clears N, K and M2 with the sums; it waits for the device first, so read-outs that
 * were only enqueued (_state, _error) are finished before the records are wiped. */
int vimg_hip_progressive_render_masked(VimgDeviceScene* scene, VimgProgressive* acc, uint32_t samples,
                                       const uint8_t* d_mask, void* d_out_rgb, void* stream, VimgRenderStats* stats);
uint64_t vimg_hip_progressive_launches(const VimgProgressive* acc);
int vimg_hip_progressive_state(VimgProgressive* acc, void* d_sum_rgb, void* d_count, void* d_batches, void* d_m2,
                               void* stream);
int vimg_hip_progressive_error(VimgProgressive* acc, void* d_err, void* stream);
int vimg_hip_progressive_select(VimgProgressive* acc, float target, uint32_t max_samples, uint8_t* d_mask,
                                void* stream, uint32_t* active_out);

/* Same as vimg_hip_render but only enqueues (no host wait, no stats); used by bench.py to time
 * back-to-back launches with HIP events on `stream`.  A scene renders one frame at a time: its
 * work counter and the scheduler's scratch (path-slot records, per-pixel records) are owned by the
 * scene, so launches on the same scene must be ordered on one stream.  A kernel-side failure (the
 * scheduler's watchdog) is reported by the next blocking call on the scene or by vimg_hip_check, not by this one. */
int vimg_hip_render_async(VimgDeviceScene* scene, const VimgRenderParams* params, void* d_out_rgb,
                          void* stream);

/* The error word of the scene's launches since it was last read: VIMG_OK, or VIMG_E_DEVICE when a
 * kernel's watchdog gave a frame up (the frame is then incomplete).  Blocking calls read it
 * themselves; after vimg_hip_render_async the caller synchronises the stream and then asks here,
 * before it uses, gathers or times the frame.  Reading clears the word. */
int vimg_hip_check(VimgDeviceScene* scene);

/* Convenience: tile_world must be 1; renders into an internal device buffer and copies the
 * W*H*3 floats to out_rgb_host (what a reference maintainer would call from main.cpp). */
int vimg_hip_render_to_host(VimgDeviceScene* scene, const VimgRenderParams* params,
                            float* out_rgb_host, VimgRenderStats* stats);

/* trace_pixel (reference include/integrators.h:181-220): one pixel (x, y), all samples;
 * writes 3 floats to out_rgb_host. */
int vimg_hip_trace_pixel(VimgDeviceScene* scene, const VimgRenderParams* params, int x, int y,
                         float* out_rgb_host);

/* heatmap_img (reference src/integrators/heatmap.cpp:38-147, called from src/main.cpp:255): the
 * BVH traversal-cost picture, turbo(colour) of cost / factor (factor <= 0 -> 20).  Uses
 * params->samples and the tile shard; the output layout is vimg_hip_render's.  d_out_rgb: device
 * pointer.  Blocking. */
int vimg_hip_render_heatmap(VimgDeviceScene* scene, const VimgRenderParams* params, float factor,
                            void* d_out_rgb, void* stream);

/* De-interleaves `world` gathered compact shard buffers (concatenated in rank order, each
 * padded to `shard_stride_pixels` triples) into the reference image layout.  d_shards and
 * d_out_rgb are DEVICE pointers. */
int vimg_hip_assemble_shards(const VimgDeviceScene* scene, uint32_t world,
                             int64_t shard_stride_pixels, const void* d_shards, void* d_out_rgb,
                             void* stream);

/* Times `steps` back-to-back renders with hipEvents recorded on the launch stream.
 * ms_per_launch[i] (host, `steps` floats) = duration of launch i.  Used for roofline.achieved. */
int vimg_hip_time_renders(VimgDeviceScene* scene, const VimgRenderParams* params, void* d_out_rgb,
                          int steps, float* ms_per_launch);

/* Post chain of reference src/main.cpp:304-356 on the GPU: tonemapper 0 clamp (simple_clamp),
 * 1 AgX (src/tonemap/agx.cpp), 2 Reinhard on the image's largest luminance
 * (src/tonemap/reinhard.cpp), 3 ACES (src/tonemap/aces.cpp); then sRGB_gamma_correction
 * (include/color_utils.h:45-68) and the 8-bit quantisation with NaN -> magenta.
 * d_rgb: DEVICE, w*h float triples; d_rgb8: DEVICE, w*h byte triples.  Saves the 12 B/pixel
 * download when only the picture is wanted.
 * Known limit: Reinhard's largest luminance is reduced into ONE device word of the process, reset and
 * read by each call on its own stream.  Calls with tonemapper 2 that run concurrently on different
 * streams share that word and may read each other's maximum; serialise them. */
int vimg_hip_post_rgb8(const void* d_rgb, int w, int h, int tonemapper, void* d_rgb8,
                       void* stream);

/* Bytes of HBM the uploaded scene occupies. */
int64_t vimg_hip_scene_bytes(const VimgDeviceScene* scene);

/* ---- the pre-step of the path on the GPU --------------------------------
 * Host buffers in and out: these replace the OpenMP loops of the reference's scene set-up
 * (src/image_texture.cpp:60-130,257-275; include/rng/sampling.h:113-135,168-197) while a scene
 * is assembled; their results are byte-identical to libvimg_host's.  vimg_hip_build_mip_chain and
 * vimg_hip_build_env_cdfs have the signatures vimg_host_set_precompute() takes. */

/* Texels of all levels of the reference's chain for a w x h image (level 0 included) and the
 * level count min(ceil(log2(min(w, h))), 15). */
uint64_t vimg_hip_mip_chain_texels(uint32_t w, uint32_t h, uint32_t* num_levels);
/* out_levels: 3 floats per texel, level 0 first, each level (max(w >> l, 1) x max(h >> l, 1))
 * behind the one before; wrap modes VIMG_WRAP_*. */
int vimg_hip_build_mip_chain(uint32_t w, uint32_t h, const float* level0_rgb, uint32_t wrap_u,
                             uint32_t wrap_v, float* out_levels);
/* Env-map importance tables from the w x h lat-long image: row_cdf[h + 1] (marginal over rows)
 * and col_cdfs[h][w + 1] (one conditional per row), as ArraySampling2D builds them. */
int vimg_hip_build_env_cdfs(const float* img_rgb, uint32_t w, uint32_t h, float* row_cdf,
                            float* col_cdfs);
/* out[i] = lut256[in[i]]: convert_sRGB_to_linear on 8-bit data with the caller's table
 * (vimg_host_srgb8_lut evaluates the reference's expression for the 256 inputs). */
int vimg_hip_lut8_to_float(const uint8_t* in, uint64_t n, const float* lut256, float* out);
/* convert_RGB_to_normal: normalize((rgb / 127.5 - 1) * (scale, scale, 1)) per pixel. */
int vimg_hip_rgb8_to_normal(const uint8_t* rgb8, uint64_t n_pixels, float scale, float* out_xyz);

/* ---- GPU BVH builders --------------------------------------------------
 * A linear BVH (Morton order, Karras' radix tree, bottom-up boxes; one primitive per leaf) in the
 * reference's layout (include/bvh.h:22-57).  Not the reference's SAH builders (those stay on the
 * host, vimg_host_build_bvh): for geometry that changes between frames.  The tree AND its layout
 * (breadth-first numbering, sibling-pair boxes, obj_indices, depth) are made by kernels; the host
 * copies the arrays in and out.  Host buffers:
 *   bounds6     : n x {min.xyz, max.xyz} of the primitives, in list_objects order
 *   nodes       : capacity 2n - 1;   bb : capacity (2 (2n - 1) + 3) float triples;
 *   obj_indices : n entries.
 * Has the signature vimg_host_build_bvh_with() takes.  The same input gives the same arrays. */
int vimg_hip_build_lbvh(uint32_t n, const float* bounds6, uint32_t* num_nodes, uint32_t* max_depth,
                        VimgBVHNode* nodes, float* bb, uint32_t* obj_indices);
/* The quality builder: PLOC (parallel locally-ordered clustering over the Morton order, search
 * radius 12), leaves ended by the reference builders' surface-area heuristic (up to 8 primitives,
 * include/bvh.h:17-20), and the top of the tree - the 16 384 subtrees of largest area - rebuilt
 * top-down by binned SAH (the quantity src/bvh/sweep_bvh.cpp:7-49 sweeps), all in kernels: 519 K
 * triangles in 4.5 ms of kernels + 2.7 ms of layout and download; the renderer runs within 3 % of its
 * rate on the host's sweep-SAH tree.  Same buffers, same layout, same hook as
 * vimg_hip_build_lbvh. */
int vimg_hip_build_ploc(uint32_t n, const float* bounds6, uint32_t* num_nodes, uint32_t* max_depth,
                        VimgBVHNode* nodes, float* bb, uint32_t* obj_indices);

/* Name of the render kernel a whole frame of this scene is launched with (textured or not,
 * register budget, scheduler) - what a rocprofv3 kernel trace will show - and the one a launch
 * with these parameters gets (the scheduler is chosen per launch: thin shards may differ). */
const char* vimg_hip_scene_kernel(const VimgDeviceScene* scene);
const char* vimg_hip_launch_kernel(const VimgDeviceScene* scene, const VimgRenderParams* params);

const char* vimg_hip_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
