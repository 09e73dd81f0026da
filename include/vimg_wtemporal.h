/*
 * vimg_wtemporal.h — C ABI of libvimg_wtemporal.so: temporal accumulation with a weight PER PIXEL, over frames that
 * are already in device memory (gfx950).  vimg_temporal_accumulate (vimg_temporal.h) has one current_weight for the
 * whole picture; here each pixel says how much its current colour is worth, so a picture whose pixels are partly
 * sampled and partly filled from their surroundings (vimg_infill.h) can be accumulated: a sampled pixel blends as it
 * does there, a filled pixel takes its reprojected history when it has one, and the fill is used only where the
 * history has nothing.
 *
 * A sixth frame library beside libvimg_hip.so: it reads frames and no scene, links the HIP runtime and nothing of the
 * other libraries, whose ABIs stay closed; this header includes vimg_hip.h for the VIMG_E_* codes alone.  It has no
 * history-bytes call of its own: the history IS libvimg_temporal's - 48 bytes per pixel, three planes of w*h float4
 * laid out [3][h][w], 16-byte aligned, A = {r, g, b, L}, G0 = {n.x, n.y, n.z, z}, G1 = {P.x, P.y, P.z, 0}
 * (vimg_temporal_history_bytes) - and either library continues what the other wrote.
 *
 * Conventions, as in vimg_temporal.h: a call returns VIMG_OK or a negative VIMG_E_* code,
 * vimg_wtemporal_last_error() returns the message of the calling thread's last failure.  A call only ENQUEUES on
 * `stream` (NULL = HIP's null stream): the library has no stream of its own, allocates nothing and waits for
 * nothing; buffers belong to the caller and must stay alive until the stream has passed the call.  Argument errors
 * (VIMG_E_INVALID) are found before anything is enqueued and give the same answer on a machine without a GPU.
 */
#ifndef VIMG_WTEMPORAL_H
#define VIMG_WTEMPORAL_H

#include <stdint.h>

#include "vimg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIMG_WTEMPORAL_MAX_EXTENT 32768u        /* largest width and height */
#define VIMG_WTEMPORAL_HISTORY_PER_PIXEL 48u    /* = VIMG_TEMPORAL_HISTORY_PER_PIXEL: the same history */

/* what a pixel did, d_out_code's values */
#define VIMG_WTEMPORAL_DEAD 0u         /* not live: {C, 0}                                              */
#define VIMG_WTEMPORAL_STARTED 1u      /* live, weight > 0, no usable history: {C, min(weight, 1)}      */
#define VIMG_WTEMPORAL_BLENDED 2u      /* live, weight > 0, history found: the blend                    */
#define VIMG_WTEMPORAL_CARRIED 3u      /* live, weight 0, history found: the history alone, C not used */
#define VIMG_WTEMPORAL_SHOWN 4u        /* live, weight 0, no usable history: {C, 0}, shown, not carried */

/* The CURRENT picture: DEVICE pointers; the eight shared fields of VimgTemporalFrames (float32 packed triples, tightly
 * packed rows, 4-byte aligned), then the weight frame. */
typedef struct VimgWTemporalFrames {
  uint32_t struct_size, width, height, reserved;
  const void* color;      /* w*h rgb triples                                                                 */
  const void* normal;     /* w*h xyz  (the `normal` feature frame)                                           */
  const void* position;   /* w*h xyz  (`position`): world-space first hits                                   */
  const void* depth;      /* w*h triples t t t (`depth`); the first component is read                        */
  const void* weight;     /* w*h float32, tightly packed, 4-byte aligned, one per pixel in the frames' row order:
                           * how many samples the pixel's colour is worth; 0 (or negative, or NaN): nothing    */
} VimgWTemporalFrames;

/* Defaults (vimg_wtemporal_defaults): max_history 32, sigma_normal 0.1, sigma_plane 0.00005 - vimg_temporal.h's
 * meanings, ranges and defaults.  There is no current_weight: the weight frame takes its place. */
typedef struct VimgWTemporalParams {
  uint32_t struct_size, reserved;
  float max_history;     /* >= 1, finite: cap of a pixel's history length */
  float sigma_normal;    /* > 0, finite: 1 - n_p . n_q below which a history tap is the same surface */
  float sigma_plane;     /* > 0, finite: distance of the tap's old position from p's tangent plane, as a fraction of
                          * p's depth, below which it is the same surface */
} VimgWTemporalParams;

/* struct_size and the defaults above. */
void vimg_wtemporal_defaults(VimgWTemporalParams* params);

/*
 * One step of temporal accumulation with per-pixel weights: reads the current frames, the weight frame and the
 * previous history `d_prev_history` (or NULL: no history), writes the next history `d_next_history`, when
 * `d_out_rgb` is not NULL plane A's rgb as w*h packed triples, and when `d_out_code` is not NULL w*h uint8, one
 * VIMG_WTEMPORAL_* code per pixel.  `prev_world_to_pixel`, the histories, the alignment and the overlap rules are
 * vimg_temporal_accumulate's: d_next_history must not overlap the previous history or any frame; d_out_rgb may be
 * frames->color itself (each lane reads its own colour before it writes) and must not overlap anything else.  In
 * addition the weight frame and d_out_code must overlap nothing that is written, and d_out_code nothing that is read.
 * One kernel launch on `stream`, one lane per pixel.
 *
 * The contract, which a float32 restatement reproduces BIT FOR BIT (tests/wtemporal_ref.py): everything is float32
 * with IEEE + - * /, comparisons and floorf - no fused multiply-add, no fmaxf / fminf - evaluated in the order
 * written.  For pixel p, with M = prev_world_to_pixel, w, h as floats:
 *
 *   z = depth_p.x;  C = color_p;  n = normal_p;  P = position_p;  next.G0 = {n, z};  next.G1 = {P, 0}
 *   wt = weight_p > 0 ? weight_p : 0                        (a NaN or negative weight is 0; +inf stays +inf)
 *   not live (!(z > 0)):                                    next.A = {C, 0}                     code 0
 *   live; "no usable history" is vimg_temporal.h's any of: prev == NULL; !(hw > 0);
 *   !(fx > -1 && fx < w && fy > -1 && fy < h); !(sumb > 0) - with hx, hy, hw, fx, fy, the four taps, their weights b,
 *   the tap test (inside the image, b > 0, L_q > 0, dn < sigma_normal, d d < (sigma_plane z)(sigma_plane z)) and the
 *   sums sumb, sumh, suml exactly as written there, in its order.  H = sumh / sumb;  L = suml / sumb.
 *   no usable history, wt > 0:                              next.A = {C, wt < 1 ? wt : 1}       code 1
 *   history found,     wt > 0:   N = L + wt;  if (N > max_history) N = max_history
 *                                a = wt / N;  if (a > 1) a = 1
 *                                                           next.A = {H + (C - H) a, N}         code 2
 *   history found,     wt == 0:  N = L;  if (N > max_history) N = max_history
 *                                                           next.A = {H, N}  (C is not used)   code 3
 *   no usable history, wt == 0:                             next.A = {C, 0}                     code 4
 *
 * Code 4 is shown this frame and not carried: its length 0 makes it nobody's tap in the next step, so a colour that
 * is worth nothing never enters a history.  With every weight equal to one value v >= 1 the next history and the
 * output are vimg_temporal_accumulate's at current_weight = v, bit for bit.
 *
 * NaN rules.  A NaN anywhere in a comparison makes it false: a NaN weight is weight 0; a NaN guide gives "no usable
 * history" (code 1 or 4, or code 0 for a NaN depth); a NaN history colour reaches only the pixels that tap it with
 * b > 0; a NaN history length is no tap.  An infinite weight at a pixel with history gives N = max_history and
 * a = inf / max_history = inf, cut to 1: the colour replaces the history.  In code 2, a NaN or infinite C reaches
 * plane A; in code 3, C is not used and cannot.  The known limits of vimg_temporal.h hold here as well.
 *
 * Defaults.  max_history, sigma_normal and sigma_plane are vimg_temporal.h's, checked there.  What is new is the
 * weight a caller gives a FILLED pixel; the library has no such parameter, vimg_amd.wtemporal.FILL_WEIGHT is 1/16.
 * Checked on the GPU (tools/wtemporal_sweep.py; DESIGN.md 4.24 has the tables) over vimg_temporal.h's orbit - 8 steps of
 * 1.5 degrees, mis at 4 spp, cornell_box_spheres 64 x 64 and 256 x 256, disney_spheres 450 x 200 - with every frame sampled
 * on one lattice of stride 2 or 3 whose phase cycles, filled by vimg_infill_reconstruct at radius = stride, weight 1 on a
 * sampled pixel, the fill weight on a guided fill and 0 on a fallback or a hole, by e = mean((x - ref)^2 / (ref^2 + 0.01))
 * of the last accumulated frame against mis at 1024 spp.  Fill weight 0 / 1/16 / 1/8 / 1/4 / 1/2 / 1: geometric mean of e
 * over the three pictures and both strides 0.02086 / 0.01775 / 0.01782 / 0.01821 / 0.01896 / 0.01995, lowest at 1/16;
 * stride 2 alone 0.01809 / 0.01601 / 0.01574 / 0.01563 / 0.01583 / 0.01640, stride 3 alone 0.02405 / 0.01969 / 0.02017 /
 * 0.02121 / 0.02270 / 0.02427.  The optimum moves with the picture (1/2 .. 1 on cornell 256 x 256, 1/16 on disney), 1/16 ..
 * 1/4 lie within 3 %, and the two ends - a fill never enters the history, a fill counts as a sample - are the worst.  At
 * stride 2 and 1/16 the three pictures have e = 0.0131, 0.0085, 0.0368, where the last sparse frame alone has 0.0314,
 * 0.0280, 0.0570 and vimg_temporal_accumulate with every pixel sampled 0.0097, 0.0039, 0.0159.
 *
 * VIMG_E_INVALID, each with its sentence: a NULL frames / params / next history / color / normal / position / depth /
 * weight pointer; a struct_size below the struct's; width or height 0 or above 32768; max_history below 1, NaN or
 * infinite; sigma_normal or sigma_plane <= 0, NaN or infinite; a next or a non-NULL previous history that is not
 * 16-byte aligned; a weight frame that is not 4-byte aligned; a NULL matrix with a non-NULL previous history; a NaN
 * or infinite matrix entry; a next history that overlaps the previous one, a frame or the weight frame; an output
 * that overlaps a history, a guide frame, the weight frame, or the colour frame without being it; output codes that
 * overlap a history, a frame, the weight frame or the output.  VIMG_E_DEVICE: a launch the HIP runtime refused.
 */
int vimg_wtemporal_accumulate(const VimgWTemporalFrames* cur, const void* d_prev_history,
                              const float prev_world_to_pixel[12], const VimgWTemporalParams* params,
                              void* d_next_history, void* d_out_rgb, void* d_out_code, void* stream);

const char* vimg_wtemporal_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
