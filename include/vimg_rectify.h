/*
 * vimg_rectify.h — C ABI of libvimg_rectify.so: the clamp of a long history of radiance to a short history beside it,
 * over histories that are already in device memory (gfx950).  The temporal accumulation (vimg_temporal.h,
 * vimg_moments.h) keeps up to max_history = 32 frames of RADIANCE, and radiance goes stale whenever the light on a
 * surface changes: an edit, a moved object, view-dependent shading under a moving camera.  vimg_antilag.h cuts the
 * history's LENGTH where a test sees the change; nothing bounds its COLOUR.  This library does: a second, short history
 * (a few frames: vimg_temporal_accumulate with a small max_history on a pair of buffers of its own) is noisy but nearly
 * current, and the long history is clamped, per pixel, to the mean +- k standard deviations of the short one over a
 * small window of the same surface - the "fast history" clamp of real-time path-tracing denoisers.
 *
 * A frame library of its own beside libvimg_filter.so ... libvimg_demand.so: it reads
 * histories and frames, never a scene, and calls no entry point of another library, whose ABIs stay closed.  It links
 * the HIP runtime and none of the project's libraries; this header includes vimg_hip.h for the VIMG_E_* codes alone.
 *
 * Conventions, as in vimg_filter.h: a call returns VIMG_OK or a negative VIMG_E_* code, vimg_rectify_last_error()
 * returns the message of the calling thread's last failure.  A call only ENQUEUES on `stream` (NULL = HIP's null
 * stream): the library has no stream of its own, allocates nothing and waits for nothing; buffers belong to the
 * caller and must stay alive until the stream has passed the call.  Argument errors (VIMG_E_INVALID) are found before
 * anything is enqueued and give the same answer on a machine without a GPU.
 */
#ifndef VIMG_RECTIFY_H
#define VIMG_RECTIFY_H

#include <stdint.h>

#include "vimg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIMG_RECTIFY_MAX_EXTENT 32768u        /* largest width and height */
#define VIMG_RECTIFY_MAX_RADIUS 3u
#define VIMG_RECTIFY_HISTORY_PER_PIXEL 48u     /* the three planes of vimg_temporal.h's history */

/* What vimg_rectify_clamp did for a pixel (d_out_code, one uint8 per pixel). */
#define VIMG_RECTIFY_KEPT 0u       /* every channel inside its bounds: the bits of slow.A stay                       */
#define VIMG_RECTIFY_CLAMPED 1u    /* some channel outside: the colour is moved to the bounds, the length shortened    */
#define VIMG_RECTIFY_FEW_TAPS 2u   /* fewer than min_taps pixels of its own surface with a fast history: untouched     */
#define VIMG_RECTIFY_NOT_LIVE 3u   /* a miss, a NaN depth or a pixel without a slow history: untouched                 */

/* The two histories of one picture and its albedo frame: DEVICE pointers.  A history has vimg_temporal.h's layout -
 * [3][h][w] float4, A = {r, g, b, L}, G0 = {n.x, n.y, n.z, z}, G1 = {P.x, P.y, P.z, 0} - and is 16-byte aligned; the
 * first three planes of a vimg_moments.h history qualify.  This is not the shared eight-field struct of the libraries
 * that read a current picture. */
typedef struct VimgRectifyFrames {
  uint32_t struct_size, width, height, reserved;
  void* slow;             /* the long history: plane A is read AND rewritten, G0 and G1 are read                */
  const void* fast;       /* the short history of the same picture, read only; only its plane A is read         */
  const void* albedo;     /* w*h rgb triples, float32 (`albedo`), 4-byte aligned, or NULL: no demodulation      */
} VimgRectifyFrames;

/* Defaults (vimg_rectify_defaults): radius 1, min_taps 4, k 1, cut 1, sigma_normal 0.5, sigma_plane 0.005,
 * albedo_floor 1/64 - see "Defaults" below. */
typedef struct VimgRectifyParams {
  uint32_t struct_size;
  uint32_t radius;       /* 1..3: taps reach radius pixels each way                                                  */
  uint32_t min_taps;     /* 1..(2 radius + 1)^2: with fewer accepted taps (the centre counts) the pixel is left alone */
  uint32_t reserved;
  float k;               /* >= 0, not NaN, +inf allowed: the bounds are the mean -+ k standard deviations            */
  float cut;             /* 0..1: how far a clamped pixel's length moves from the slow to the fast history's         */
  float sigma_normal;    /* > 0, finite: 1 - n_p . n_q at which a tap's score reaches 1 */
  float sigma_plane;     /* > 0, finite: distance of a tap from p's tangent plane, as a fraction of p's depth, at
                          * which the score reaches 1 */
  float albedo_floor;    /* > 0, finite: albedo components at or below it demodulate by it instead */
} VimgRectifyParams;

/* struct_size and the defaults above. */
void vimg_rectify_defaults(VimgRectifyParams* params);

/* Bytes of workspace vimg_rectify_clamp needs for a w x h picture: 0, whatever the arguments.  There is no pack pass:
 * the one kernel demodulates the fast history as it stages its tile. */
uint64_t vimg_rectify_workspace(uint32_t width, uint32_t height);

/*
 * Clamps plane A of `frames->slow`, IN PLACE, to the statistics of `frames->fast` around each pixel.  One kernel launch
 * on `stream`.  d_out_rgb: w*h rgb triples, float32, 4-byte aligned, which receive the resulting slow.A.rgb of EVERY
 * pixel, or NULL.  d_out_code: w*h uint8, the VIMG_RECTIFY_* code of each pixel, or NULL.  d_workspace,
 * workspace_bytes: not used (vimg_rectify_workspace is 0); the pointer may be NULL.  Nothing overlaps anything: not the
 * two histories, not the albedo frame and the slow history, not an output and a history, the albedo frame or the other
 * output.  The clamp is in place on `slow` by definition.
 *
 * The contract, which a float32 restatement reproduces BIT FOR BIT (tests/rectify_ref.py): everything is float32 with
 * IEEE + - * /, comparisons and the correctly rounded sqrtf - no fused multiply-add, no fmaxf / fminf - evaluated in
 * the order written.  (vimg_hip.h's adaptive statistic has a sqrt in its contract already.)
 *
 *   The guides n, z, P of every pixel are slow's G0 and G1.  a~ = albedo > albedo_floor ? albedo : albedo_floor per
 *   component (1 without an albedo frame), as in vimg_filter.h.  For a pixel q: F_q = fast.A_q.rgb / a~_q per
 *   component, Lf_q = fast.A_q.w.  For the pixel p: Ls = slow.A_p.w, H = slow.A_p.rgb / a~_p.  R = radius.
 *
 *     !(z_p > 0) or !(Ls > 0)   nothing is written to slow, code 3.
 *     otherwise                 taps q = p + (dx, dy), dy = -R..R outer, dx = -R..R inner, THE CENTRE INCLUDED.  A tap
 *                               is ACCEPTED when it is inside the image, z_q > 0, Lf_q > 0 and it is the centre or
 *                               S < 1, with vimg_infill.h's
 *                                 dn = 1 - ((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z)      s_n = dn < 0 ? 0 : dn / sigma_normal
 *                                 e  = P_q - P_p;  d = (n_p.x e.x + n_p.y e.y) + n_p.z e.z   s_p = (d d) / ((sigma_plane z_p) (sigma_plane z_p))
 *                                 S  = s_n + s_p
 *                               (a NaN guide makes a tap other than the centre not accepted).  For the accepted taps,
 *                               in tap order, per channel: m += 1, s1 = s1 + F_q, s2 = s2 + F_q F_q.
 *       m < min_taps            nothing is written to slow, code 2.
 *       otherwise, per channel  mean = s1 / float(m);  v = s2 / float(m) - mean mean;  if (v < 0) v = 0;
 *                               w = k sqrtf(v);  lo = mean - w;  hi = mean + w;
 *                               Hc = H < lo ? lo : H > hi ? hi : H;  the channel MOVED when H < lo or H > hi.
 *         no channel moved      the bits of slow.A_p stay, code 0.
 *         some channel moved    slow.A_p.rgb = Hc a~_p, all three channels (Hc without an albedo frame);
 *                               slow.A_p.w = Ls - cut (Ls - Lf_p) when Lf_p > 0 and Ls > Lf_p, else Ls;  code 1.
 *   d_out_rgb, when given, receives the resulting slow.A_p.rgb of every pixel, whatever its code.
 *
 * What follows from it.  k = +inf with finite taps changes no bit: the bounds are -+inf, or NaN where v is 0 (inf 0),
 * and a NaN bound moves nothing either, every comparison with it being false.  A NaN or infinite fast colour poisons
 * only the boxes it enters - mean or v is NaN there - and those pixels are KEPT, not clamped to garbage.  A pixel's
 * own fast value is always among its box's inputs when it has one, so a pixel whose two histories agree and whose
 * surface is uniform stays inside its bounds: the clamp costs nothing where the histories agree.  A lane writes only
 * its own slow.A_p, and taps read `fast` and slow's guide planes, which nobody writes: the in-place update has no race.
 * An unmoved channel of a clamped pixel is (H / a~) a~, which may differ from H in its last bit.  The bounds are taken
 * of DEMODULATED radiance, so a texture edge inside the window does not widen them.
 *
 * Known limits.  The short history is noisy: at k standard deviations of fast_history frames of a few samples the
 * clamp also pulls a converged long history toward that noise - the price that "Defaults" measures.  The window is
 * spatial: a lighting edge inside it (a shadow boundary) widens the bounds and stale radiance within them stays.  It
 * sees per-channel boxes, not hue.
 *
 * Defaults.  Measured on the GPU (tools/rectify_sweep.py; DESIGN.md 4.33 has the tables), every run a temporal
 * preview, mis at 4 spp, e = mean((x - ref)^2 / (ref^2 + 0.01)) against mis at 1024 spp of the scene as it then stands,
 * over the preview's fast_history 2, 4, 8 x radius 1..3 x k 1, 1.5, 2, 3, 4 x cut 0, 0.5, 1 (135 settings; min_taps 4, the
 * sigmas and the floor of vimg_filter.h).  NO EDIT: the last frame of vimg_temporal.h's orbits, cornell_box_spheres
 * 64 x 64 and 256 x 256, disney_spheres 450 x 200.  EDIT, seven legs: the light x 0.25 and x 4 after the orbit, frames 1..8,
 * each also with antilag; vimg_motion.h's moved panel (variance-guided) and fast sphere (unfiltered, variance-guided)
 * with motion, the object's pixels.  A setting is ELIGIBLE when the geometric mean of its three no-edit e is within 2 %
 * of the plain preview's in the same run; the default is the eligible setting with the lowest geometric mean over the
 * edit legs (a leg's figure: the geometric mean of its e).
 *                                     no edit / plain (each)            edit legs / plain
 *   fast_history 2, radius 1, k 1, cut 1 (default)  0.883 (0.957 0.979 0.735)   0.428
 *   fast_history 2, radius 1, k 1, cut 0            0.830                       0.440
 *   fast_history 2, radius 2, k 1, cut 1            0.851                       0.481
 *   fast_history 4, radius 2, k 2, cut 0.5          0.956 (0.976 0.932 0.960)   0.745
 *   worst of the 135                                1.000 (h 4, r 1, k 4)       1.098 (h 8, r 1, k 3, cut 0)
 * All 135 settings are eligible - without an edit the clamp GAINS on every orbit, most on disney_spheres, whose glossy
 * spheres carry reprojection error - and the most eager one wins the edit legs: light x 0.25, frames 1..8, e = 0.143 0.007
 * 0.006 0.005 0.004 0.004 0.003 0.003 against 0.262 0.205 0.170 0.143 0.123 0.107 0.094 0.083 without the clamp.  At the
 * defaults 7.0 / 5.7 / 5.9 % of the pixels are clamped on the orbits' last frames.  With antilag the FIRST frame after
 * light x 0.25 is worse with the clamp (0.041 against 0.012): antilag cuts the slow history at once and the fast
 * history, which nobody cuts, still holds the old light for that frame; from the second frame on it is better (0.0033
 * against 0.0071).  With motion the clamp recovers the panel (0.00004 against 0.00012, and 0.00006 without motion) but
 * NOT the fast sphere (0.0219 against 0.0235 unfiltered and 0.0179 without motion; 0.0205 against 0.0227 and 0.0023
 * variance-guided): the gap vimg_motion.h reports is not closed there.
 *
 * VIMG_E_INVALID, each with its sentence: a NULL frames / params / slow / fast pointer; a struct_size below the
 * struct's; width or height 0 or above 32768; a history that is not 16-byte aligned; an albedo frame or an output
 * colour that is not 4-byte aligned; radius outside 1..3; min_taps outside 1..(2 radius + 1)^2; k below 0 or NaN; cut
 * outside 0..1 or NaN; a sigma or the albedo floor <= 0, NaN or infinite; the two histories overlapping; the albedo frame overlapping the slow history; an
 * output that overlaps a history, the albedo frame or the other output.
 * VIMG_E_DEVICE: a launch the HIP runtime refused.
 */
int vimg_rectify_clamp(const VimgRectifyFrames* frames, const VimgRectifyParams* params, void* d_out_rgb, void* d_out_code,
                       void* d_workspace, uint64_t workspace_bytes, void* stream);

const char* vimg_rectify_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
