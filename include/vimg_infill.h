/*
 * vimg_infill.h — C ABI of libvimg_infill.so: reconstruction of a sparsely sampled colour frame from the first-hit
 * feature frames beside it, over frames that are already in device memory (gfx950).  A masked progressive increment
 * (vimg_hip_progressive_render_masked) gives radiance to a subset of the pixels - one in four on a stride-2 lattice -
 * while the guides exist for every pixel at full resolution; this library fills the pixels without samples from the
 * sampled ones around them that lie on the same surface.
 *
 * A frame library of its own beside libvimg_filter.so, libvimg_temporal.so, libvimg_varfilter.so and
 * libvimg_moments.so: it reads frames, never a scene, and calls no entry point of another
 * library, whose ABIs stay closed.  It links the HIP runtime and none of the project's libraries; this header includes
 * vimg_hip.h for the VIMG_E_* codes alone.
 *
 * Conventions, as in vimg_filter.h: a call returns VIMG_OK or a negative VIMG_E_* code, vimg_infill_last_error()
 * returns the message of the calling thread's last failure.  A call only ENQUEUES on `stream` (NULL = HIP's null
 * stream): the library has no stream of its own, allocates nothing and waits for nothing; buffers belong to the
 * caller and must stay alive until the stream has passed the call.  Argument errors (VIMG_E_INVALID) are found before
 * anything is enqueued and give the same answer on a machine without a GPU.
 */
#ifndef VIMG_INFILL_H
#define VIMG_INFILL_H

#include <stdint.h>

#include "vimg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIMG_INFILL_MAX_EXTENT 32768u        /* largest width and height */
#define VIMG_INFILL_MAX_RADIUS 4u
#define VIMG_INFILL_WORKSPACE_PER_PIXEL 48u

/* What vimg_infill_reconstruct did for a pixel (d_out_code, one uint8 per pixel). */
#define VIMG_INFILL_SAMPLED 0u     /* the pixel has samples: its colour is copied                                   */
#define VIMG_INFILL_GUIDED 1u      /* filled from sampled taps of its own kind, a live pixel's weighted by the guides */
#define VIMG_INFILL_UNGUIDED 2u    /* no such tap in the window: the tent-weighted mean of every sampled tap        */
#define VIMG_INFILL_HOLE 3u        /* no sampled tap in the window at all: 0 0 0                                    */

/* The frames of one picture: DEVICE pointers, tightly packed rows, 4-byte aligned.  The first nine fields are those
 * of VimgFilterFrames. */
typedef struct VimgInfillFrames {
  uint32_t struct_size, width, height, reserved;
  const void* color;      /* w*h rgb triples, float32; read where count > 0 (the others may hold anything finite or not) */
  const void* normal;     /* w*h xyz  (the `normal` feature frame)                                         */
  const void* position;   /* w*h xyz  (`position`)                                                         */
  const void* depth;      /* w*h triples t t t (`depth`); the first component is read                      */
  const void* albedo;     /* w*h rgb (`albedo`), or NULL: no demodulation                                  */
  const void* count;      /* w*h uint32, one per pixel in the row order of the other frames: the samples the
                           * pixel has had (vimg_hip_progressive_state's count).  A pixel is SAMPLED when its
                           * count is above 0 */
} VimgInfillFrames;

/* Defaults (vimg_infill_defaults): radius 2, sigma_normal 1, sigma_plane 0.005, albedo_floor 1/64 - see "Defaults"
 * below. */
typedef struct VimgInfillParams {
  uint32_t struct_size;
  uint32_t radius;       /* 1..4: taps reach radius pixels each way.  A lattice of stride s leaves no hole from
                          * radius s - 1 on */
  float sigma_normal;    /* > 0, finite: 1 - n_p . n_q at which a tap's weight reaches 0 */
  float sigma_plane;     /* > 0, finite: distance of a tap from p's tangent plane, as a fraction of p's depth, at
                          * which the weight reaches 0 */
  float albedo_floor;    /* > 0, finite: albedo components at or below it demodulate by it instead */
} VimgInfillParams;

/* struct_size and the defaults above. */
void vimg_infill_defaults(VimgInfillParams* params);

/* Bytes of workspace vimg_infill_reconstruct needs for a w x h picture: 48 per pixel - three planes of float4,
 * {C.rgb, sampled}, {n.xyz, z} and {P.xyz, 0} - whatever the arguments (0 x 0 is 0). */
uint64_t vimg_infill_workspace(uint32_t width, uint32_t height);

/*
 * Fills the pixels of `color` that have no samples.  Two kernel launches on `stream`.  d_out_rgb (w*h rgb triples)
 * may be frames->color itself; it must not overlap any other frame, d_out_code or the workspace.  d_out_code: w*h
 * uint8, the VIMG_INFILL_* code of each pixel, or NULL.  d_workspace: 16-byte aligned, at least
 * vimg_infill_workspace(w, h) bytes.
 *
 * The contract, which a float32 restatement reproduces BIT FOR BIT (tests/infill_ref.py): everything is float32 with
 * IEEE + - * / and comparisons - no fused multiply-add, no fmaxf / fminf, no transcendental - evaluated in the order
 * written.
 *
 *   Pack, every pixel.  LIVE when z > 0 (misses and NaN depths are not).  a~ = albedo > floor ? albedo : floor per
 *   component (1 without an albedo frame), as in vimg_filter.h.  C = live ? color / a~ : color: a pixel that is not
 *   live is not demodulated.  Planes {C.rgb, sampled ? 1 : 0}, {n.xyz, z}, {P.xyz, 0}.
 *
 *   Fill, every pixel p.  R = radius, taps q = p + (dx, dy), dy = -R..R outer, dx = -R..R inner, tent weight
 *   k = float((R + 1 - |dx|) (R + 1 - |dy|)), an exact small integer.  A tap outside the image or not sampled has no
 *   part in anything below; p itself is a tap only when it is sampled, and then none is looked at:
 *     sampled p              out = the bits of color (a copy, not C a~), code 0.
 *     unsampled live p       over the sampled LIVE taps, with p's normal, position and depth:
 *                              dn = 1 - ((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z)      s_n = dn < 0 ? 0 : dn / sigma_normal
 *                              e  = P_q - P_p;  d = (n_p.x e.x + n_p.y e.y) + n_p.z e.z   s_p = (d d) / ((sigma_plane z_p) (sigma_plane z_p))
 *                              S  = s_n + s_p                                             w   = S < 1 ? k ((1 - S) (1 - S)) : 0
 *                            (a NaN anywhere in S gives w = 0).  Taps with w > 0 add w to sumw and w C_q to sumc, in
 *                            tap order.  If sumw > 0: C_p = sumc / sumw, code 1.
 *     unsampled p, not live  the same over the sampled taps that are NOT live, with w = k: the background continues.
 *     otherwise              for either kind: every sampled tap inside the image with w = k, C_p = sumc / sumw,
 *                            code 2 - the unguided fallback, the surface has no sampled neighbour in the window.
 *     no sampled tap at all  C_p = 0 0 0, code 3: a hole.
 *   out = live ? C_p a~_p : C_p for an unsampled p.  Because it is multiplied by its OWN full-resolution albedo,
 *   texture detail comes back at full resolution and only irradiance is interpolated.
 *
 * A NaN colour of a sampled pixel stays where it is and reaches the pixels it is a tap of with w > 0: the weights do
 * not look at colour.  On a full lattice of stride s (every s-th pixel of every s-th row sampled, any offset) in a
 * picture of at least s x s, radius >= s - 1 leaves no hole.
 *
 * Known limits: that of vimg_filter.h (coverage-scaled guides at silhouettes, which here mostly end as code 2); and
 * the guides know nothing of shadow edges, highlights and reflections, which are interpolated across - there is no
 * colour term, the pixel to fill has no colour.
 *
 * Defaults.  Measured on the GPU on the frames of vimg_filter.h's "Defaults" - cornell_box_spheres 512 x 512 and
 * disney_spheres 900 x 400, mis at 4 and 16 spp on the stride-2 lattice of phase 0, guides at 4 samples, against mis at
 * 1024 spp, e = mean((x - ref)^2 / (ref^2 + 0.01)), geometric mean of the four (tools/infill_sweep.py, 184 settings in
 * two sweeps; DESIGN.md 4.23 has the tables):
 *   tent-weighted mean without guides, radius 2                     0.19656
 *   radius 2, sigma_normal 0.5, sigma_plane 0.005 (vimg_filter.h's)  0.03773   (0.03585, 0.02100, 0.07618, 0.03535)
 *   radius 2, sigma_normal 1,   sigma_plane 0.005 (the defaults)     0.03651   (0.03576, 0.02096, 0.07317, 0.03241)
 *   radius 1 / 3 / 4 at the defaults' sigmas                         0.04432 / 0.03299 / 0.03313
 *   the same samples on every pixel, no fill                         (0.07495, 0.01837, 0.12749, 0.03158)
 * sigma_normal 1 - the weight reaches 0 where the normals are at right angles - is lower than 0.5 on each of the four
 * frames and halves the share of code 2 (0.79 -> 0.28 % and 0.69 -> 0.35 % of the unsampled pixels); 2 and 4 gain
 * another 2.4 and 0.9 % and were not taken: from 2 on the term no longer excludes anything.  radius stays 2, the
 * smallest window that gives every pixel of a stride-2 lattice at least four taps: at these sample counts a wider
 * window scores better because it averages more noise - on three of the four frames the fill at radius 3 is nearer the
 * reference than the fully sampled frame at the same count - which is the preview filter's work, and Progressive.render_sparse asks for
 * radius = stride.  sigma_plane stays 0.005: 0.001 scores 3 % lower and 0.0002 a further 16 %, but on small pictures it
 * drives pixels into the unguided fallback (cornell_box_spheres 64 x 64: code 2 on 9.4 % of the unsampled pixels at
 * 0.005, 16.7 % at 0.001, 23.5 % at 0.0002).  albedo_floor is vimg_filter.h's.
 *
 * VIMG_E_INVALID, each with its sentence: a NULL frames / params / color / normal / position / depth / count / out /
 * workspace pointer; a struct_size below the struct's; width or height 0 or above 32768; radius outside 1..4; a sigma
 * or the albedo floor <= 0, NaN or infinite; a workspace too small or not 16-byte aligned; an output that overlaps the
 * colour frame without being it, or another frame, the codes or the workspace; codes that overlap the workspace.
 * VIMG_E_DEVICE: a launch the HIP runtime refused.
 */
int vimg_infill_reconstruct(const VimgInfillFrames* frames, const VimgInfillParams* params, void* d_out_rgb,
                            void* d_out_code, void* d_workspace, uint64_t workspace_bytes, void* stream);

const char* vimg_infill_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
