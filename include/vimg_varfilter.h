/*
 * vimg_varfilter.h — C ABI of libvimg_varfilter.so: the variance-guided a-trous filter over frames that are already
 * in device memory (gfx950).
 *
 * A frame library of its own beside libvimg_filter.so and libvimg_temporal.so: it reads frames,
 * never a scene.  Where vimg_filter_atrous stops at colour edges with one frame-wide sigma_color, this filter stops
 * at a luminance difference measured against each pixel's own noise: the variance of the pixel's mean luminance, as
 * a progressive accumulator knows it (vimg_hip_progressive_state) or, where it does not, as the pixel's surroundings
 * suggest it (SVGF, Schied et al. 2017, without the temporal half).  It links the HIP runtime and none of the other
 * libraries; this header includes vimg_hip.h for the VIMG_E_* codes alone.
 *
 * Conventions: a call returns VIMG_OK or a negative VIMG_E_* code, vimg_varfilter_last_error() returns the message
 * of the calling thread's last failure.  A call only ENQUEUES on `stream` (NULL = HIP's null stream): the library has
 * no stream of its own, allocates nothing and waits for nothing; buffers belong to the caller and must stay alive
 * until the stream has passed the call.  Argument errors (VIMG_E_INVALID) are found before anything is enqueued
 * and give the same answer on a machine without a GPU.
 */
#ifndef VIMG_VARFILTER_H
#define VIMG_VARFILTER_H

#include <stdint.h>

#include "vimg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIMG_VARFILTER_MAX_EXTENT 32768u      /* largest width and height */
#define VIMG_VARFILTER_MAX_ITERATIONS 12u
#define VIMG_VARFILTER_WORKSPACE_PER_PIXEL 64u

/* The frames of one picture: DEVICE pointers, float32, tightly packed rows, 4-byte aligned.  The first eight fields
 * are those of VimgFilterFrames, and so is albedo. */
typedef struct VimgVarFilterFrames {
  uint32_t struct_size, width, height, reserved;
  const void* color;      /* w*h rgb triples, any row order as long as all frames share it                 */
  const void* normal;     /* w*h xyz  (the `normal` feature frame)                                          */
  const void* position;   /* w*h xyz  (`position`)                                                          */
  const void* depth;      /* w*h triples t t t (`depth`); the first component is read                       */
  const void* albedo;     /* w*h rgb (`albedo`), or NULL: no demodulation                                   */
  const void* variance;   /* w*h float32, one per pixel: the variance of the pixel's mean luminance Y (the weights
                           * of vimg_hip.h: 0.212671, 0.715160, 0.072169), as vimg_varfilter_variance gives it; or
                           * NULL.  A pixel's variance is KNOWN when v >= 0 && v < +inf (as comparisons): NaN, a
                           * negative value, +inf and a NULL frame all mean unknown, and the filter estimates it */
} VimgVarFilterFrames;

/* Parameters.  Defaults (vimg_varfilter_defaults): see "Defaults" below. */
typedef struct VimgVarFilterParams {
  uint32_t struct_size, iterations;    /* 1..12 */
  float sigma_luminance; /* > 0, may be +inf: the luminance difference, in standard deviations of the pixel's
                          * (prefiltered) noise, at which a tap's weight reaches 0.  Not halved per iteration: the
                          * filtered variance falls instead */
  float sigma_normal;    /* > 0, finite: as in VimgAtrousParams */
  float sigma_plane;     /* > 0, finite: as in VimgAtrousParams */
  float albedo_floor;    /* > 0, finite: as in VimgAtrousParams */
  float variance_floor;  /* > 0, finite: added to sigma_luminance^2 Vg, in units of demodulated luminance squared -
                          * the squared difference a pixel WITHOUT noise still averages over */
} VimgVarFilterParams;

/* struct_size and the defaults. */
void vimg_varfilter_defaults(VimgVarFilterParams* params);

/* Bytes of workspace vimg_varfilter_atrous needs for a w x h picture: 64 per pixel, as vimg_filter_atrous - two
 * colour planes (ping-pong) and two guide planes of float4; the colour planes' fourth component, which the a-trous
 * filter leaves unused, carries the variance.  Whatever the arguments (0 x 0 is 0). */
uint64_t vimg_varfilter_workspace(uint32_t width, uint32_t height);

/*
 * The variance-guided edge-avoiding a-trous filter.  iterations + 3 kernel launches on `stream`.  d_out_rgb (w*h rgb
 * triples) may be frames->color itself and d_out_variance (w*h float32, or NULL: not wanted) may be frames->variance
 * itself; neither may overlap anything else.  d_workspace: 16-byte aligned, at least vimg_varfilter_workspace(w, h)
 * bytes.
 *
 * The contract, which a float32 restatement reproduces BIT FOR BIT (tests/varfilter_ref.py): everything is float32
 * with IEEE + - * / and comparisons - no fused multiply-add, no fmaxf / fminf, no sqrt, no exp - evaluated in the
 * order written.  Y(v) = (v.x 0.212671f + v.y 0.715160f) + v.z 0.072169f.  s_n and s_p are the a-trous filter's
 * (vimg_filter.h):
 *     dn  = 1 - ((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z)        s_n = dn < 0 ? 0 : dn / sigma_normal
 *     e   = P_q - P_p;  d = (n_p.x e.x + n_p.y e.y) + n_p.z e.z     s_p = (d d) / ((sigma_plane z_p) (sigma_plane z_p))
 * A NaN anywhere in a tap's score S gives the tap weight 0.
 *
 *   Pack.  For every pixel: a~ = albedo > floor ? albedo : floor per component, C = color / a~, ya = Y(a~); without an
 *   albedo frame C = color and ya = 1.  G0 = {n.xyz, z}, G1 = {P.xyz, 0}.  A pixel is LIVE when z > 0 (misses and NaN
 *   depths are not).  V = v / (ya ya) where the pixel is live and its variance v is known; V = -1, the mark of
 *   "unknown", where it is live and v is not known; V = 0 where it is not live.
 *
 *   Estimate.  One launch; only live pixels with V < 0 do anything.  L = Y(C).  Taps q = p + (dx, dy), dy = -3..3
 *   outer, dx = -3..3 inner.  The centre has w = 1.  A tap outside the image, not live, or whose L_q is not finite
 *   ((L_q - L_q) == 0 fails) has w = 0.  Every other tap has S = s_n + s_p and w = S < 1 ? (1 - S) (1 - S) : 0 - no
 *   colour term and no kernel weight.  Taps with w > 0 add w to sw, w L_q to s1 and w (L_q L_q) to s2, in tap order.
 *   m1 = s1 / sw, m2 = s2 / sw, V = m2 - m1 m1, and V = 0 where that is < 0 (a NaN stays).  This is SVGF's spatial
 *   fallback; the values are already pixel means, so their spread is the estimate and nothing is divided by a sample
 *   count.  Only the V of the pixel itself is written: the estimate of one pixel never reads another's.
 *
 *   Iteration i = 0 .. iterations - 1, ping-pong on {C, V}.  A pixel that is not live copies its C and V.  For a live p:
 *     Vg: taps r = p + (dx, dy), dy = -1..1 outer, dx = -1..1 inner, g = b[dx + 1] b[dy + 1] with b = {1/4, 1/2, 1/4}.
 *     Taps inside the image and live (p itself is) add g to sg and g V_r to sv, in tap order; Vg = sv / sg.
 *     den = sl2 Vg + variance_floor, with sl2 = sigma_luminance sigma_luminance a host float.  (sigma_luminance = +inf
 *     makes the luminance term 0 wherever Vg > 0; where Vg is 0, inf 0 is a NaN and the pixel keeps its value.)
 *     Step s = 2^i, taps q = p + s (dx, dy), dy = -2..2 outer, dx = -2..2 inner, k = h[dx + 2] h[dy + 2] with
 *     h = {1/16, 1/4, 3/8, 1/4, 1/16}.  The centre tap has w = k, a tap outside the image or not live has w = 0, and
 *     every other tap
 *       dL = Y(C_p) - Y(C_q)       S = (s_n + s_p) + (dL dL) / den       w = S < 1 ? k ((1 - S) (1 - S)) : 0
 *     Taps with w > 0 add w to sumw, w C_q to sumc (per component) and (w w) V_q to sumv, in tap order.
 *     C' = sumc / sumw per component, V' = sumv / (sumw sumw).  sumw >= 9/64 always: there is no 0 / 0.
 *
 *   Unpack.  out = C a~ (C without an albedo frame), packed triples.  out_variance = V (ya ya): the variance of the
 *   filtered pixel's luminance, were the taps independent - 0 for a pixel that is not live.
 *
 * The limits of vimg_filter_atrous hold here too (guides of partly covered silhouette pixels).  A NaN colour is no
 * one's tap, in the estimate or in an iteration; the pixel itself stays NaN and its estimated V is NaN, which the
 * 3 x 3 prefilter hands to its eight neighbours: they keep their value too.
 *
 * Defaults.  iterations 3, sigma_luminance 8, variance_floor 1e-8, sigma_normal 0.5, sigma_plane 0.005, albedo_floor 1/64 (the last
 * three are vimg_filter_atrous's).  Chosen on the GPU by the procedure of vimg_filter.h (tools/varfilter_sweep.py; DESIGN.md
 * 4.21 has the tables): cornell_box_spheres (512 x 512) and disney_spheres (900 x 400), mis, against mis at 1024 spp,
 * e = mean((x - ref)^2 / (ref^2 + 0.01)) of the filtered frame over the noisy frame's, on three frames per scene - 4 spp in
 * one increment (no variance: estimated), 16 spp in four increments (K = 4) and render_adaptive(0.05, 4, 64) - score =
 * geometric mean of the six, 100 settings (iterations 2..6, sigma_luminance 1..16, variance_floor 1e-10..1e-4):
 *   e_filtered / e_noisy, cornell 4 / 16 / adaptive, disney 4 / 16 / adaptive, [cornell at 64 x 64: 4 / 16 / adaptive]
 *   this filter, defaults     0.051  0.068  0.245   0.113  0.079  0.255   score 0.111   [0.252  0.326  0.684]
 *   vimg_filter_atrous, its   0.029  0.051  0.116   0.085  0.140  0.278   score 0.091   [0.286  0.856  1.837]
 *   5 iterations              0.050  0.072  0.237   0.113  0.088  0.266   score 0.115   [0.260  0.422  0.813]
 * On these frames the FIXED filter has the better score: it wins four of the six large frames, cornell by a factor of up to
 * two.  This filter wins disney at 16 spp and adaptive, and every frame of the 64 x 64 picture, where the fixed filter leaves
 * the 16 spp frame nearly as it was and makes the adaptive one worse than unfiltered.  What it gives is one setting that is
 * never worse than the noisy frame, from 4 spp to a mostly converged adaptive frame; on a frame whose noise level sigma_color
 * 2 happens to fit, the fixed filter is the better one.  sigma_luminance decides (score 0.84, 0.61, 0.25, 0.111, 0.115 at
 * 1, 2, 4, 8, 16, three iterations); iterations 2..6 at sigma_luminance 8 score 0.120, 0.111, 0.114, 0.115, 0.117; variance_floor moves
 * the score by under 0.001 over 1e-10..1e-4 - the sweep holds no converged frame, which is what the floor is for, so it
 * stays at the smallest value that is well above float32 rounding of a luminance difference (1e-8: differences under 1e-4).
 *
 * VIMG_E_INVALID, each with its sentence: a NULL frames / params / color / normal / position / depth / out /
 * workspace pointer; a struct_size below the struct's; width or height 0 or above 32768; iterations outside 1..12;
 * a sigma or a floor <= 0 or NaN, or infinite (sigma_luminance alone may be +inf); a workspace too small or not
 * 16-byte aligned.  VIMG_E_DEVICE: a launch the HIP runtime refused.
 */
int vimg_varfilter_atrous(const VimgVarFilterFrames* frames, const VimgVarFilterParams* params, void* d_out_rgb,
                          void* d_out_variance, void* d_workspace, uint64_t workspace_bytes, void* stream);

/*
 * The variance frame of a progressive accumulator's state (vimg_hip_progressive_state): d_count uint32 N, d_batches
 * uint32 K, d_m2 float32 M2, one each per pixel of a width x height picture (or of any width * height items);
 * d_out_variance float32, which may be d_m2 itself.  One launch on `stream`.
 *     V = (K < 2 || N == 0) ? NaN : ((M2 < 0 ? 0 : M2) / float(K - 1)) / float(N)
 * - the quantity under the square root of `err` in vimg_hip.h, in the same order, so sqrt(V) / (|Y(S) / float(N)| + 1e-3f)
 * is vimg_hip_progressive_error bit for bit wherever K >= 2.  NaN is "unknown" to vimg_varfilter_atrous.
 * VIMG_E_INVALID: a NULL pointer; width or height 0 or above 32768.
 */
int vimg_varfilter_variance(uint32_t width, uint32_t height, const void* d_count, const void* d_batches, const void* d_m2,
                            void* d_out_variance, void* stream);

const char* vimg_varfilter_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
