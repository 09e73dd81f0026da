/*
 * vimg_motion.h — C ABI of libvimg_motion.so: where the surface point a pixel shows WAS before the scene's geometry
 * moved, over frames and tables that are already in device memory (gfx950).  vimg_temporal_accumulate,
 * vimg_moments_accumulate and vimg_wtemporal_accumulate look a pixel up in the history where the LAST camera saw the
 * pixel's CURRENT world position; that is right only while the world stands still.  After
 * vimg_hip_scene_update_geometry a pixel on a moved object must look where its surface point was.  This library
 * writes that previous-world position per pixel - the current position plus the displacement of the pixel-centre hit,
 * interpolated from the old and new vertex tables by the hit's barycentrics, or taken from the old and new sphere -
 * and the accumulate calls, which already take the position frame as an argument, run unchanged on it.
 *
 * An eighth frame library beside libvimg_hip.so: it reads frames and tables and no scene, links the HIP runtime and
 * nothing of the other libraries, whose ABIs stay closed; this header includes vimg_hip.h for the VIMG_E_* codes and
 * the records VimgRay, VimgRayHit (as vimg_hip_camera_rays and vimg_hip_trace_rays write them) and vimg_scene.h's
 * VimgPrim alone.
 *
 * Conventions, as in vimg_temporal.h: a call returns VIMG_OK or a negative VIMG_E_* code,
 * vimg_motion_last_error() returns the message of the calling thread's last failure.  A call only ENQUEUES on
 * `stream` (NULL = HIP's null stream): the library has no stream of its own, allocates nothing and waits for
 * nothing; buffers belong to the caller and must stay alive until the stream has passed the call.  Argument errors
 * (VIMG_E_INVALID) are found before anything is enqueued and give the same answer on a machine without a GPU.
 */
#ifndef VIMG_MOTION_H
#define VIMG_MOTION_H

#include <stdint.h>

#include "vimg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIMG_MOTION_MAX_EXTENT 32768u /* largest width and height */

/* what d_out_code holds per pixel */
enum { VIMG_MOTION_STATIC = 0, VIMG_MOTION_TRIANGLE = 1, VIMG_MOTION_SPHERE = 2, VIMG_MOTION_OUT_OF_RANGE = 3 };

/* The picture: DEVICE pointers, in frame-array order (row 0 = top), tightly packed. */
typedef struct VimgMotionFrames {
  uint32_t struct_size, width, height, reserved;
  const void* position; /* w*h xyz float32 (the `position` feature frame), 4-byte aligned                            */
  const void* hits;     /* w*h VimgRayHit, 16-byte aligned: the closest hit of one pixel-centre ray per pixel        */
  const void* rays;     /* w*h VimgRay, 16-byte aligned: the rays those hits answer; read for sphere hits only, NULL */
                        /* is allowed when num_spheres == 0                                                          */
} VimgMotionFrames;

/* The scene's tables: DEVICE pointers.  old / new: the positions under which the history was made and the current
 * ones; each pair is both given or both NULL, NULL = that table did not move. */
typedef struct VimgMotionGeometry {
  uint32_t struct_size, num_prims, num_tris, num_vertices, num_spheres, reserved;
  const void* prims;        /* num_prims VimgPrim, 8-byte aligned                                                  */
  const void* tri_vertices; /* num_tris x 3 uint32, 4-byte aligned: GLOBAL vertex rows,                            */
                            /* meshes[tri_mesh[t]].first_vertex + tri_indices[3 t + k]                             */
  const void* old_vertices; /* num_vertices x 3 float32, 4-byte aligned                                            */
  const void* new_vertices;
  const void* old_spheres;  /* num_spheres x 4 float32 (centre xyz, radius), 16-byte aligned                       */
  const void* new_spheres;
} VimgMotionGeometry;

/*
 * Writes Q, the previous-world position of the surface point each pixel shows, to `d_out_previous` (w*h xyz float32,
 * 4-byte aligned) and, when `d_out_code` is not NULL, one VIMG_MOTION_* byte per pixel to it.  Neither output may
 * overlap an input or the other output.  One kernel launch on `stream`, one lane per pixel.
 *
 * The contract, which a float32 restatement reproduces BIT FOR BIT (tests/motion_ref.py): everything is float32 with
 * IEEE + - * / and comparisons - no fused multiply-add - evaluated in the order written.  With P the pixel's
 * `position` triple and {t, prim, b1, b2} its hit:
 *
 *   prim == VIMG_NO_HIT:  Q = P, code 0.
 *   An index out of range - prim >= num_prims; for a triangle prims[prim].index >= num_tris or one of its three
 *   vertex rows >= num_vertices; for a sphere prims[prim].index >= num_spheres; a prims[prim].type that is neither -
 *   Q = P, code 3, and NOTHING behind the bad index is read: every gather is bounds-tested in the kernel.
 *   Triangle, rows i0 i1 i2 = tri_vertices[3 index + 0 .. 2]:
 *       e_k = old[i_k] - new[i_k]  per component;   w0 = (1 - b1) - b2;   D = (w0 e0 + b1 e1) + b2 e2
 *     with the vertex tables NULL, D = 0.
 *   Sphere, {c_old, r_old}, {c_new, r_new} = old / new_spheres[index], {org, dir} the pixel's ray:
 *       u = (org + t dir) - c_new  per component;   s = r_old / r_new;   D = (c_old - c_new) + (u s - u)
 *     where !(r_new > 0), D = c_old - c_new; with the sphere tables NULL, D = 0.
 *   D.x == 0 && D.y == 0 && D.z == 0:  Q is P's BITS, code 0 - a select, not an add (-0 + 0 would flip a sign bit).
 *   Otherwise Q = P + D per component, code 1 (triangle) or 2 (sphere).
 *
 * So where nothing moved the accumulate calls get the bytes they get without this library.  A NaN in a table or a
 * hit makes D compare unequal to 0: Q = P + D is NaN there, which the accumulate calls treat as a pixel without
 * history.
 *
 * VIMG_E_INVALID, each with its sentence, in this order: a NULL frames / geometry pointer; a struct_size below the
 * struct's; width or height 0 or above 32768; a NULL position or hits frame; a position frame that is not 4-byte, a
 * hits or rays frame that is not 16-byte aligned; NULL rays with num_spheres > 0; num_prims > 0 with NULL prims,
 * num_tris > 0 with NULL tri_vertices; prims not 8-byte, tri_vertices not 4-byte aligned; one half of the vertex or
 * of the sphere pair; a vertex table that is not 4-byte, a sphere table that is not 16-byte aligned; a NULL or not
 * 4-byte aligned d_out_previous; a d_out_previous, then a d_out_code, that overlaps position, hits, rays, prims,
 * tri_vertices, a vertex or a sphere table; a d_out_code that overlaps d_out_previous.  VIMG_E_DEVICE: a launch the
 * HIP runtime refused.
 */
int vimg_motion_previous_position(const VimgMotionFrames* frames, const VimgMotionGeometry* geometry, void* d_out_previous,
                                  void* d_out_code, void* stream);

const char* vimg_motion_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
