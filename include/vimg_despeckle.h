/*
 * vimg_despeckle.h — C ABI of libvimg_despeckle.so: the clamp of fireflies in a colour frame, before it is filtered,
 * over frames that are already in device memory (gfx950).  A path-traced frame of 1 - 16 samples per pixel carries
 * fireflies: single pixels whose mean is many times that of the same surface around them.  The a-trous filters
 * (vimg_filter.h, vimg_varfilter.h) spread each one into a bright blotch - one sigma_color cannot both filter the
 * noise and reject a 50x outlier - and the temporal accumulation then carries the blotch for max_history frames.  This
 * library scales such a pixel down to a bound taken from the pixels of its own surface around it.
 *
 * A frame library of its own beside libvimg_filter.so ... libvimg_motion.so: it reads frames,
 * never a scene, and calls no entry point of another library, whose ABIs stay closed.  It links the HIP runtime and
 * none of the project's libraries; this header includes vimg_hip.h for the VIMG_E_* codes alone.
 *
 * Conventions, as in vimg_filter.h: a call returns VIMG_OK or a negative VIMG_E_* code, vimg_despeckle_last_error()
 * returns the message of the calling thread's last failure.  A call only ENQUEUES on `stream` (NULL = HIP's null
 * stream): the library has no stream of its own, allocates nothing and waits for nothing; buffers belong to the
 * caller and must stay alive until the stream has passed the call.  Argument errors (VIMG_E_INVALID) are found before
 * anything is enqueued and give the same answer on a machine without a GPU.
 */
#ifndef VIMG_DESPECKLE_H
#define VIMG_DESPECKLE_H

#include <stdint.h>

#include "vimg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIMG_DESPECKLE_MAX_EXTENT 32768u        /* largest width and height */
#define VIMG_DESPECKLE_MAX_RADIUS 3u
#define VIMG_DESPECKLE_MAX_RANK 4u
#define VIMG_DESPECKLE_WORKSPACE_PER_PIXEL 32u

/* What vimg_despeckle_clamp did for a pixel (d_out_code, one uint8 per pixel). */
#define VIMG_DESPECKLE_KEPT 0u       /* at or below its bound: the colour is copied                                  */
#define VIMG_DESPECKLE_CLAMPED 1u    /* above its bound: the colour is scaled down to it                             */
#define VIMG_DESPECKLE_FEW_TAPS 2u   /* fewer than min_taps pixels of its own surface in the window: copied          */
#define VIMG_DESPECKLE_NOT_LIVE 3u   /* a miss (or a NaN depth): copied                                              */

/* The frames of one picture: DEVICE pointers, tightly packed rows, 4-byte aligned.  The nine fields are those of
 * VimgFilterFrames. */
typedef struct VimgDespeckleFrames {
  uint32_t struct_size, width, height, reserved;
  const void* color;      /* w*h rgb triples, float32                                                      */
  const void* normal;     /* w*h xyz  (the `normal` feature frame)                                         */
  const void* position;   /* w*h xyz  (`position`)                                                         */
  const void* depth;      /* w*h triples t t t (`depth`); the first component is read                      */
  const void* albedo;     /* w*h rgb (`albedo`), or NULL: no demodulation                                  */
} VimgDespeckleFrames;

/* Defaults (vimg_despeckle_defaults): radius 1, rank 3, min_taps 4, gain 3, sigma_normal 0.5, sigma_plane 0.005,
 * albedo_floor 1/64 - see "Defaults" below. */
typedef struct VimgDespeckleParams {
  uint32_t struct_size;
  uint32_t radius;       /* 1..3: taps reach radius pixels each way                                                  */
  uint32_t rank;         /* 1..4: the rank-th largest accepted tap enters the bound; rank - 1 brighter ones are
                          * taken for outliers themselves                                                            */
  uint32_t min_taps;     /* rank..(2 radius + 1)^2 - 1: with fewer accepted taps the pixel is left alone             */
  float gain;            /* >= 1, finite: the bound is gain times the larger of the mean and the rank-th largest tap */
  float sigma_normal;    /* > 0, finite: 1 - n_p . n_q at which a tap's score reaches 1 */
  float sigma_plane;     /* > 0, finite: distance of a tap from p's tangent plane, as a fraction of p's depth, at
                          * which the score reaches 1 */
  float albedo_floor;    /* > 0, finite: albedo components at or below it demodulate by it instead */
} VimgDespeckleParams;

/* struct_size and the defaults above. */
void vimg_despeckle_defaults(VimgDespeckleParams* params);

/* Bytes of workspace vimg_despeckle_clamp needs for a w x h picture: 32 per pixel - two planes of float4,
 * {n.xyz, z} and {P.xyz, L} - whatever the arguments (0 x 0 is 0). */
uint64_t vimg_despeckle_workspace(uint32_t width, uint32_t height);

/*
 * Scales the pixels of `color` that stand out of their own surface down to a bound.  Two kernel launches on `stream`.
 * d_out_rgb (w*h rgb triples) may be frames->color itself - in place is the preview's normal use; it must not overlap
 * any other frame, d_out_code or the workspace.  d_out_code: w*h uint8, the VIMG_DESPECKLE_* code of each pixel, or
 * NULL.  d_workspace: 16-byte aligned, at least vimg_despeckle_workspace(w, h) bytes.
 *
 * The contract, which a float32 restatement reproduces BIT FOR BIT (tests/despeckle_ref.py): everything is float32
 * with IEEE + - * / and comparisons - no fused multiply-add, no fmaxf / fminf, no transcendental - evaluated in the
 * order written.
 *
 *   Pack, every pixel.  LIVE when z > 0 (misses and NaN depths are not).  a~ = albedo > floor ? albedo : floor per
 *   component (1 without an albedo frame), as in vimg_filter.h.  C = live ? color / a~ : color.
 *   L = (C.r 0.212671 + C.g 0.715160) + C.b 0.072169, the luminance of vimg_varfilter.h.  Planes {n.xyz, z}, {P.xyz, L}.
 *
 *   Clamp, every pixel p.  R = radius.
 *     p not live           out = the bits of color, code 3.
 *     p live               taps q = p + (dx, dy), dy = -R..R outer, dx = -R..R inner, (0, 0) skipped.  A tap is
 *                          ACCEPTED when it is inside the image, live, S < 1 and L_q >= 0, with vimg_infill.h's
 *                            dn = 1 - ((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z)      s_n = dn < 0 ? 0 : dn / sigma_normal
 *                            e  = P_q - P_p;  d = (n_p.x e.x + n_p.y e.y) + n_p.z e.z   s_p = (d d) / ((sigma_plane z_p) (sigma_plane z_p))
 *                            S  = s_n + s_p
 *                          (a NaN anywhere makes it not accepted).  For the accepted taps, in tap order: m += 1,
 *                          sum = sum + L_q, and L_q is inserted into the descending list t_1..t_rank, which starts
 *                          at -inf: v = L_q; for k = 1..rank: if v > t_k, swap v and t_k.
 *       m < min_taps       out = the bits of color, code 2.
 *       otherwise          mean = sum / float(m);  b = mean > t_rank ? mean : t_rank;  T = gain b.
 *                          If L_p > T and L_p < +inf:  f = T / L_p,  out = (C_p f) a~_p per component (C_p f without
 *                          an albedo frame), code 1.  Otherwise out = the bits of color, code 0.
 *
 * What follows from it.  A kept pixel is a copy, not C a~.  A NaN or infinite colour at p is left where it is (L_p is
 * NaN or +inf, or not above T): the post chain's NaN rule stays visible.  A NaN tap takes no part (L_q >= 0 fails);
 * an infinite tap makes the sum, the mean and so T infinite, whatever the rank, and the pixels around it are not
 * clamped.  Hue is kept: the colour is scaled by one factor.  Misses and pixels with too few taps of their
 * own surface - lone emitters, silhouettes - are never touched, and an emitter's pixels protect each other, because
 * the guides exclude the other surfaces around them.  The mean is in the bound so that a pixel among few and dim
 * accepted taps - t_rank = 0 when fewer than rank of them are above 0 - is not turned black, and so that a
 * converged picture is left alone: the rank-th largest of eight taps alone sits below many a pixel of plain noise.
 *
 * Known limits.  It removes energy: sparse true signal - a caustic a few pixels wide, a glint - is dimmed like a
 * firefly, and the picture's mean falls by what the fireflies carried ("luminance kept" below).  It sees pixel means,
 * not samples: a firefly sample in a pixel of many samples is diluted before it is seen, and one pixel of two cannot
 * be told from a bright pixel.  It inherits vimg_filter.h's coverage-scaled guides at silhouettes: code 2 there.
 *
 * Defaults.  Measured on the GPU on the frames of vimg_filter.h's "Defaults" - cornell_box_spheres 512 x 512 and
 * disney_spheres 900 x 400, mis at 4 and 16 spp, guides at 4 samples, against mis at 1024 spp, e = mean((x - ref)^2 /
 * (ref^2 + 0.01)) - over radius 1..3 x rank 1..4 x gain 1, 1.5, 2, 3, 4 (tools/despeckle_sweep.py, 60 settings; DESIGN.md
 * 4.30 has the tables).  Each clamped frame is filtered by vimg_filter_atrous and by vimg_varfilter_atrous at their
 * defaults; a setting's score is the geometric mean of those eight e, and it is ELIGIBLE when none of the eight is above
 * the same frame's filtered without a clamp and it clamps at most 1 % of the live pixels of each 1024-spp frame.
 *                                      score     e filtered (cornell 4, 16, disney 4, 16 spp)    e variance-guided
 *   no clamp                           0.003170  0.00218  0.00094  0.01089  0.00441              0.00412  0.00121  0.00805  0.00256
 *   radius 1, rank 3, gain 2           0.003051  0.00261  0.00096  0.00901  0.00436              0.00338  0.00116  0.00767  0.00254
 *   radius 1, rank 3, gain 3 (default) 0.002986  0.00209  0.00094  0.01027  0.00440              0.00304  0.00117  0.00777  0.00256
 *   radius 1, rank 4, gain 3           0.002987        radius 1, rank 3 / 4, gain 4   0.002997 / 0.002993
 *   radius 3, rank 2, gain 1 (lowest)  0.002865  not eligible: clamps 1.5 and 2.0 % of the 1024-spp frames
 * 13 of the 60 settings are eligible, all at gain 3 or 4; radius 1, rank 3, gain 3 is the lowest of them.  The gain of 2
 * this library was first written with is not: it makes cornell at 4 spp WORSE after the fixed filter than no clamp
 * (0.00261 against 0.00218; at 16 spp 0.00096 against 0.00094) - at 512 x 512 it clamps 4.9 % of the live pixels and takes
 * 1.3 % of the frame's luminance, a bias the filter cannot average out, where gain 3 clamps 2.1 % and takes 0.6 %.  At
 * the defaults the clamp changes 0.023 and 0.037 % of the live pixels of the two 1024-spp frames and keeps 0.9939,
 * 0.9991, 0.9992 and 1.0000 of the four noisy frames' luminance.  Radius and rank stay: at the eligible gains a wider window scores
 * worse (rank 3, gain 3: 0.00306 at radius 2, 0.00314 at radius 3: the rank-th largest of 24 or 48 taps is a higher
 * bound, and fewer fireflies are caught), and ranks 3 and 4 differ by less than the
 * figures resolve.  min_taps 4 is half the window; the sigmas and the floor are vimg_filter.h's.
 *
 * VIMG_E_INVALID, each with its sentence: a NULL frames / params / color / normal / position / depth / out /
 * workspace pointer; a struct_size below the struct's; width or height 0 or above 32768; a workspace too small or not
 * 16-byte aligned; radius outside 1..3; rank outside 1..4; min_taps outside rank..(2 radius + 1)^2 - 1; gain below 1,
 * NaN or infinite; a sigma or the albedo floor <= 0, NaN or infinite; an output that overlaps the colour frame
 * without being it, or another frame, the codes or the workspace; codes that overlap the workspace.
 * VIMG_E_DEVICE: a launch the HIP runtime refused.
 */
int vimg_despeckle_clamp(const VimgDespeckleFrames* frames, const VimgDespeckleParams* params, void* d_out_rgb,
                         void* d_out_code, void* d_workspace, uint64_t workspace_bytes, void* stream);

const char* vimg_despeckle_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
