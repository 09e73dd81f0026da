/*
 * vimg_antilag.h — C ABI of libvimg_antilag.so: shortens a reprojected history where the picture has changed, over
 * frames that are already in device memory (gfx950).  vimg_temporal_accumulate, vimg_moments_accumulate and
 * vimg_wtemporal_accumulate blend a history with the current frame wherever the SURFACE is the same; none of them asks
 * whether the light on it still is.  After an edit of a light or a material the old radiance then fades at
 * 1 / max_history per frame.  This library compares the current frame with the history, region by region, by a paired
 * t-test of their luminances, and multiplies the history LENGTHS - plane A's fourth component - by a scale in [0, 1]:
 * 1 where the two agree within their noise, 0 where they clearly do not.  It never writes a colour and never blends;
 * the accumulate call that follows runs unchanged and its taps simply find shorter, or zero, lengths.
 *
 * A seventh frame library beside libvimg_hip.so: it reads frames and no scene, links the HIP runtime and nothing of
 * the other libraries, whose ABIs stay closed; this header includes vimg_hip.h for the VIMG_E_* codes alone.  The
 * history is libvimg_temporal's - planes A = {r, g, b, L}, G0 = {n.x, n.y, n.z, z}, G1 = {P.x, P.y, P.z, 0} of w*h float4
 * each, laid out [3][h][w], 16-byte aligned (vimg_temporal_history_bytes) - or the first three planes of
 * libvimg_moments': plane M is neither read nor written.
 *
 * Conventions, as in vimg_temporal.h: a call returns VIMG_OK or a negative VIMG_E_* code,
 * vimg_antilag_last_error() returns the message of the calling thread's last failure.  A call only ENQUEUES on
 * `stream` (NULL = HIP's null stream): the library has no stream of its own, allocates nothing and waits for
 * nothing; buffers belong to the caller and must stay alive until the stream has passed the call.  Argument errors
 * (VIMG_E_INVALID) are found before anything is enqueued and give the same answer on a machine without a GPU.
 */
#ifndef VIMG_ANTILAG_H
#define VIMG_ANTILAG_H

#include <stdint.h>

#include "vimg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIMG_ANTILAG_MAX_EXTENT 32768u         /* largest width and height */
#define VIMG_ANTILAG_MAX_RADIUS 8u             /* largest window radius */
#define VIMG_ANTILAG_HISTORY_PER_PIXEL 48u     /* = VIMG_TEMPORAL_HISTORY_PER_PIXEL: the planes that are looked at */
#define VIMG_ANTILAG_WORKSPACE_PER_PIXEL 8u    /* {d, v}: the paired difference and whether the pixel is a pair */

/* The CURRENT picture: DEVICE pointers; the eight shared fields of VimgTemporalFrames (float32 packed triples, tightly
 * packed rows, 4-byte aligned). */
typedef struct VimgAntilagFrames {
  uint32_t struct_size, width, height, reserved;
  const void* color;      /* w*h rgb triples: what the history is compared with                              */
  const void* normal;     /* w*h xyz  (the `normal` feature frame)                                           */
  const void* position;   /* w*h xyz  (`position`): world-space first hits                                   */
  const void* depth;      /* w*h triples t t t (`depth`); the first component is read                        */
} VimgAntilagFrames;

/* Defaults (vimg_antilag_defaults): radius 2, t_low 2, t_high 3, min_matches 8, sigma_normal 0.1,
 * sigma_plane 0.00005 - see "Defaults" below. */
typedef struct VimgAntilagParams {
  uint32_t struct_size;
  uint32_t radius;       /* 1..8: the statistic's window is (2 radius + 1)^2 history pixels, clipped to the picture */
  float t_low;           /* > 0, finite: below t_low standard errors nothing happens */
  float t_high;          /* > t_low, finite: from t_high standard errors on the history is dropped */
  float min_matches;     /* >= 2, finite: with fewer matched pixels in the window there is no evidence: scale 1 */
  float sigma_normal;    /* > 0, finite: vimg_temporal.h's same-surface test, between a history pixel and the */
  float sigma_plane;     /* > 0, finite: current pixel it lands on                                            */
} VimgAntilagParams;

/* struct_size and the defaults above. */
void vimg_antilag_defaults(VimgAntilagParams* params);

/* Bytes of the workspace for a w x h picture: 8 per pixel (0 x 0 is 0). */
uint64_t vimg_antilag_workspace_bytes(uint32_t width, uint32_t height);

/*
 * Rescales the lengths of the history `d_history` IN PLACE, in the history's own pixel coordinates, by how well its
 * radiance agrees with the current frames `cur`.  `cur_world_to_pixel`: 12 floats in HOST memory, the row-major 3 x 4
 * matrix of the CURRENT camera (vimg_temporal.h describes it): a history pixel's position is projected INTO the
 * current picture - the opposite direction of the accumulate calls, which look the current pixel up in the history.
 * `d_workspace`: at least vimg_antilag_workspace_bytes(w, h) bytes, 16-byte aligned.  `d_scale_out`: NULL, or w*h
 * float32 (4-byte aligned) that get the scale of every history pixel.  Of the history only the fourth component of
 * plane A is written, and only where it is > 0.  The history, the four frames, the workspace and d_scale_out must
 * not overlap one another.  Two kernel launches on `stream`, one lane per history pixel.
 *
 * The contract, which a float32 restatement reproduces BIT FOR BIT (tests/antilag_ref.py): everything is float32
 * with IEEE + - * /, comparisons and floorf - no fused multiply-add, no fmaxf / fminf - evaluated in the order
 * written.  With M = cur_world_to_pixel, w, h as floats:
 *
 * Pass 1, per history pixel q:  A = hist.A_q;  d = 0;  v = 0.  When A.w > 0 and every step below holds:
 *     n_q, z_q = hist.G0_q;  P_q = hist.G1_q.xyz
 *     hx = ((M0 P_q.x + M1 P_q.y) + M2 P_q.z) + M3,  hy from M4..7,  hw from M8..11;            hw > 0
 *     fx = hx / hw - 0.5;  fy = hy / hw - 0.5;  cx = floorf(fx + 0.5);  cy = floorf(fy + 0.5)     (the NEAREST pixel)
 *     cx >= 0 && cx < w && cy >= 0 && cy < h                                                    (a NaN fails)
 *     p = the current pixel (cx, cy);  depth_p.x > 0
 *     dn = 1 - ((n_q.x n_p.x + n_q.y n_p.y) + n_q.z n_p.z);                                     dn < sigma_normal
 *     e = P_p - P_q;  dd = (n_q.x e.x + n_q.y e.y) + n_q.z e.z;               dd dd < (sigma_plane z_q) (sigma_plane z_q)
 *     d = lum(C_p) - lum(A.rgb),  lum(c) = (c.r 0.212671 + c.g 0.715160) + c.b 0.072169
 *     d - d == 0 (d is finite): v = 1;  otherwise d = 0
 *   The workspace gets {d, v}.
 *
 * Pass 2, per history pixel q at (x, y), over the window rows y - radius .. y + radius and columns x - radius ..
 * x + radius that lie inside the picture.  Per window row, over its columns ascending, each sum starting from 0:
 *     S1 = sum d;  S2 = sum d d;  S0 = sum v
 *   then over the rows ascending, each starting from 0:  sd = sum S1;  sq = sum S2;  c = sum S0
 *     s = 1
 *     if (c >= min_matches) {
 *       m = sd / c;  var = (sq - sd m) / (c - 1);  if (!(var > 0)) var = 0
 *       t2 = (m m) / (var / c)
 *       lo = t_low t_low;  hi = t_high t_high
 *       if (!(t2 > lo)) s = 1;  else if (!(t2 < hi)) s = 0;  else s = (hi - t2) / (hi - lo)
 *     }
 *   A.w > 0:  hist.A_q.w = A.w s  - that one float, nothing else of the history.   scale_out_q = s.
 *
 * t2 is the square of the paired t statistic: the mean difference of current and history luminance over the window's
 * matched pixels, in units of its standard error.  Texture and shading gradients cancel in the pair; one firefly
 * raises mean and variance together, so its t stays about 1; and the thresholds are in standard errors, so they do
 * not depend on how bright the scene is.
 *
 * NaN and zero rules.  A NaN guide or matrix product fails a comparison: no pair.  A NaN or infinite colour, here
 * or in the history, is no pair.  A noise-free window that has not changed has m = 0 and var = 0: t2 = 0 / 0 = NaN,
 * !(t2 > lo), keep.  A noise-free window that has changed has t2 = x / 0 = +inf: drop.  A pixel without history
 * (A.w <= 0 or NaN) is no pair, is not written and has scale 1.
 *
 * Defaults.  Chosen on the GPU (tools/antilag_sweep.py; DESIGN.md 4.26 has the tables) among radius 2 / 4 / 8 x t_low
 * 2 / 3 / 4 x t_high 1.5 / 2 / 3 t_low, mis at 4 spp, by e = mean((x - ref)^2 / (ref^2 + 0.01)) against mis at 1024 spp:
 * (i) vimg_temporal.h's three orbits without an edit, the last accumulated frame; (ii, iii) on cornell_box_spheres
 * 64 x 64 and 256 x 256 the light's emission times 0.25, times 4, and a wall recoloured after the orbit, frames 1 - 4
 * after the edit.  The rule: the lowest geometric mean of e over (ii, iii) among the settings whose geometric mean over
 * (i) stays within 2 % of accumulating without this library.  25 of the 27 do; radius 2, t_low 2, t_high 3 has 0.0177
 * over (ii, iii) where no rescaling has 0.0752 (radius 4, 3, 6: 0.0235), and 0.972 of the plain geometric mean over (i)
 * - 1.033 and 1.124 on the two cornell orbits, where 10 % of the history pixels are shortened by noise alone, and 0.792
 * on disney_spheres, whose glossy spheres carry reprojection error the test finds.  A caller who wants every unchanged
 * picture within 0.3 % passes radius 2, t_low 3, t_high 4.5 (0.890 over (i), 0.0203 over (ii, iii)).  min_matches 8 and
 * the two sigmas were not swept: the sigmas are vimg_temporal.h's, so a pair here is what a tap is there.
 *
 * VIMG_E_INVALID, each with its sentence, in this order: a NULL frames / params pointer; a struct_size below the
 * struct's; width or height 0 or above 32768; a NULL color / normal / position / depth frame; radius outside 1..8;
 * t_low <= 0, NaN or infinite; t_high <= t_low, NaN or infinite; min_matches below 2, NaN or infinite; sigma_normal
 * or sigma_plane <= 0, NaN or infinite; a NULL matrix; a NaN or infinite matrix entry; a NULL history; a history that
 * is not 16-byte aligned; a NULL, too small or misaligned workspace; a d_scale_out that is not 4-byte aligned; a
 * history (48 bytes per pixel) that overlaps a frame; a workspace that overlaps the history or a frame; a
 * d_scale_out that overlaps the history, a frame or the workspace.  VIMG_E_DEVICE: a launch the HIP runtime refused.
 */
int vimg_antilag_rescale(const VimgAntilagFrames* cur, const float cur_world_to_pixel[12], void* d_history,
                         const VimgAntilagParams* params, void* d_workspace, uint64_t workspace_bytes, void* d_scale_out,
                         void* stream);

const char* vimg_antilag_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
