/*
 * vimg_moments.h — C ABI of libvimg_moments.so: temporal accumulation of radiance AND of the first two moments of
 * luminance over frames that are already in device memory (gfx950).  From the moments and the history length it
 * derives, per pixel, the variance of the accumulated mean's luminance - what vimg_varfilter_atrous takes as its
 * variance frame - under a camera that moves.
 *
 * A frame library of its own beside libvimg_filter.so, libvimg_temporal.so and libvimg_varfilter.so (DESIGN.md 4.20,
 * 4.22): it reads frames, never a scene, and calls no entry point of another library, whose ABIs stay closed.  This is
 * the temporal half of SVGF (Schied et al. 2017) that vimg_varfilter.h leaves out.  It links the HIP runtime and none
 * of the project's libraries; this header includes vimg_hip.h for the VIMG_E_* codes alone.
 *
 * Conventions, as in vimg_temporal.h: a call returns VIMG_OK or a negative VIMG_E_* code, vimg_moments_last_error()
 * returns the message of the calling thread's last failure.  A call only ENQUEUES on `stream` (NULL = HIP's null
 * stream): the library has no stream of its own, allocates nothing and waits for nothing; buffers belong to the
 * caller and must stay alive until the stream has passed the call.  Argument errors (VIMG_E_INVALID) are found before
 * anything is enqueued and give the same answer on a machine without a GPU.
 */
#ifndef VIMG_MOMENTS_H
#define VIMG_MOMENTS_H

#include <stdint.h>

#include "vimg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIMG_MOMENTS_MAX_EXTENT 32768u        /* largest width and height */
#define VIMG_MOMENTS_HISTORY_PER_PIXEL 64u

/* The CURRENT picture: DEVICE pointers, float32, tightly packed rows, 4-byte aligned.  The first eight fields are
 * those of VimgTemporalFrames. */
typedef struct VimgMomentsFrames {
  uint32_t struct_size, width, height, reserved;
  const void* color;      /* w*h rgb triples: one frame, or the running mean of current_weight frames        */
  const void* normal;     /* w*h xyz  (the `normal` feature frame)                                          */
  const void* position;   /* w*h xyz  (`position`): world-space first hits                                  */
  const void* depth;      /* w*h triples t t t (`depth`); the first component is read                       */
  const void* variance;   /* w*h float32, one per pixel: the variance of the mean luminance Y of `color`, as
                           * vimg_varfilter_variance gives it; or NULL.  KNOWN under the rule of vimg_varfilter.h:
                           * v >= 0 && v < +inf (as comparisons); NaN, a negative value, +inf and a NULL frame all
                           * mean unknown */
} VimgMomentsFrames;

/* Defaults (vimg_moments_defaults): max_history 32, current_weight 1, sigma_normal 0.1, sigma_plane 0.00005 - those of
 * VimgTemporalParams, which the first four floats are - and min_history 4; see "Defaults" below. */
typedef struct VimgMomentsParams {
  uint32_t struct_size, reserved;
  float max_history;     /* >= 1, finite: as in VimgTemporalParams */
  float current_weight;  /* >= 1, finite: as in VimgTemporalParams (k when `color` is a running mean of k frames) */
  float sigma_normal;    /* > 0, finite: as in VimgTemporalParams */
  float sigma_plane;     /* > 0, finite: as in VimgTemporalParams */
  float min_history;     /* >= 1, finite, <= max_history: the history length N below which the variance derived from
                          * the moments is not trusted and NaN ("unknown") is given instead */
} VimgMomentsParams;

/* struct_size and the defaults above. */
void vimg_moments_defaults(VimgMomentsParams* params);

/*
 * Bytes of one history of a w x h picture: 64 per pixel (0 x 0 is 0).  A HISTORY is four planes of w*h float4, laid
 * out [4][h][w], 16-byte aligned, in the row order of the frames.  Planes A, G0 and G1 are exactly those of
 * vimg_temporal.h, so the first 48 w h bytes are a history of vimg_temporal_accumulate:
 *   A  = {r, g, b, L}        the accumulated radiance and the history length L; L == 0: the pixel holds no surface
 *   G0 = {n.x, n.y, n.z, z}  the guides the radiance was accumulated under (z: depth)
 *   G1 = {P.x, P.y, P.z, 0}  the world-space position
 *   M  = {m1, m2, V, 0}      the accumulated first and second moment of luminance, per FRAME (not per running mean),
 *                            and V, the variance of Y(A.rgb), NaN where it is unknown
 */
uint64_t vimg_moments_history_bytes(uint32_t width, uint32_t height);

/*
 * One step of temporal accumulation with moments.  Arguments as vimg_temporal_accumulate's; beside them `d_out_variance`,
 * w*h float32 or NULL, which gets plane M's V.  d_next_history must not overlap the previous history or any frame, the
 * variance frame included; d_out_rgb may be frames->color itself and d_out_variance may be frames->variance itself (each
 * lane reads its own value before it writes); neither may overlap anything else.  One kernel launch on `stream`, one lane
 * per pixel; the matrix and the parameters travel as kernel arguments.
 *
 * The contract, which a float32 restatement reproduces BIT FOR BIT (tests/moments_ref.py): everything is float32 with
 * IEEE + - * /, comparisons and floorf - no fused multiply-add, no fmaxf / fminf - evaluated in the order written.
 *
 *   1. Planes A, G0, G1 and d_out_rgb are the contract of vimg_temporal.h, operation for operation: the liveness test,
 *      the four taps in its order, which taps count, sumb, H, len = suml / sumb, N, a and the blend.
 *   2. Y(c) = (c.x 0.212671f + c.y 0.715160f) + c.z 0.072169f (vimg_varfilter.h).  Lc = Y(C);  v = variance_p;
 *      vk = the variance frame is not NULL and v >= 0 && v < +inf.
 *      x2 = Lc Lc;  if vk:  x2 = x2 + v (current_weight - 1)
 *      (a running mean of k frames has E[L^2] = mu^2 + sigma^2 / k = mu^2 + v; the term restores the second moment of ONE
 *      frame, mu^2 + sigma^2 = mu^2 + k v, in expectation.  At current_weight 1 it adds v 0.)
 *   3. not live:                                    next.M = {Lc, x2, 0, 0}
 *   4. live without usable history (every case in which next.A = {C, 1}):
 *                                                   next.M = {Lc, x2, vk ? v : NaN, 0}
 *   5. live with history: counted taps also add, in tap order, b m1_q to s1 and b m2_q to s2 (M_q of the previous history)
 *        m1h = s1 / sumb;  m2h = s2 / sumb;  sh = m2h - m1h m1h;  if (sh < 0) sh = 0;  Vh = sh / len
 *        m1 = m1h + (Lc - m1h) a;  m2 = m2h + (x2 - m2h) a;  sc = m2 - m1 m1;  if (sc < 0) sc = 0
 *        Vc = vk ? v : sc / current_weight
 *        u = 1 - a;  V = (u u) Vh + (a a) Vc;  if (!(N >= min_history)) V = NaN (the quiet NaN 0x7fc00000)
 *                                                   next.M = {m1, m2, V, 0}
 *   6. d_out_variance = next.M.z: NaN is "unknown" to vimg_varfilter_atrous, which then estimates the pixel's variance
 *      from its surroundings; 0 for a pixel that is not live.
 *
 * Why this V.  The accumulated colour is A = (1 - a) H + a C, history and current frame independent, so its luminance has
 * variance (1 - a)^2 Var(H) + a^2 Var(C).  Var(C) is v where the caller knows it, else the per-frame variance sc of the
 * updated moments over the current_weight frames in C.  Var(H) is the per-frame variance of the reprojected moments, sh,
 * over the reprojected history length len: exact while the history is a plain mean (N below the cap), and conservative
 * at the cap, where the exponential average's variance tends to sigma^2 / (2 max_history - 1) and sh / len to sigma^2 /
 * max_history.  sh itself is biased low by (1 - 1 / N) while N is small (the mean is estimated from the same N frames):
 * a float64 simulation of this recursion (iid noise, a static pixel) gives mean V / true variance 0.25 at N = 2, 0.56 at
 * N = 3, 0.69 at N = 4, rising to 0.97 at N = 32, and 1.56 at the cap (max_history 8, 32 frames in).
 *
 * A NaN anywhere in a comparison makes it false, as in vimg_temporal.h.  A NaN moment of the history reaches only the
 * pixels that tap it with b > 0, and only their plane M; the limits of vimg_temporal.h hold here too.
 *
 * Defaults.  max_history, sigma_normal, sigma_plane: vimg_temporal.h's, whose figures planes A, G0, G1 reproduce bit for
 * bit.  min_history 4 is SVGF's value, and the float64 simulation above is why: below 4 the estimate is less than 0.6 of
 * the true variance.  Checked on the GPU (tools/moments_cost.py; DESIGN.md 4.22 has the tables) on the orbit of
 * vimg_temporal.h's "Defaults" - cornell_box_spheres 64 x 64 and 256 x 256, disney_spheres 450 x 200, mis at 4 spp, 8 steps,
 * e against mis at 1024 spp - with vimg_varfilter_atrous at its defaults on the accumulated colour and this V:
 *   min_history 2 / 3 / 4 / 6 / 8:  e = 0.00724 / 0.00714 / 0.00714 / 0.00714 / 0.00714 (cornell 64 x 64),
 *   0.00223 / 0.00221 / 0.00223 / 0.00222 / 0.00222 (256 x 256), 0.01314 / 0.01355 / 0.01352 / 0.01355 / 0.01359 (disney);
 *   geometric mean 0.00596 / 0.00597 / 0.00599 / 0.00599 / 0.00599.  No value is lower than 4 on all three frames and the
 *   means lie within 0.5 % of each other (after nine frames few pixels have a history that short), so 4 stays.
 *   Beside it: the noisy frame 0.05302 / 0.04931 / 0.08564; the accumulated colour filtered by vimg_filter_atrous at
 *   sigma_color / sqrt(9), 0.01116 / 0.00237 / 0.01339 (geometric mean 0.00708): this V wins on cornell and loses on disney.
 *   mean(V) / mean((Y(A) - Y(ref))^2) over the live pixels with known V is 0.009 / 0.038 / 2.13: V is the noise of
 *   independent frames and holds neither the bias of reprojection nor correlated noise (vimg_temporal.h, "Known limits"),
 *   which a few pixels' large errors carry.  By the medians the ratio is 4.5 / 8.4 / 9.5, where an exact variance would give
 *   2.2: at the typical pixel V is two to four times too large, the conservative side.
 * Cost: one call takes 1.10 x (450 x 200, 0.056 ms) to 1.33 x (1800 x 800, 0.128 ms) the time of vimg_temporal_accumulate on the
 * same frames; by the bytes a lane requests, 196 against 156 per pixel with one tap and 388 against 300 with four.
 *
 * VIMG_E_INVALID, each with its sentence: everything vimg_temporal_accumulate refuses, under the prefix "moments:" and with
 * the 64-byte history; min_history below 1, NaN or infinite, or above max_history; a next history that overlaps the variance
 * frame; an output variance that overlaps a history, a guide frame, the colour frame or d_out_rgb, or the variance frame
 * without being it.  VIMG_E_DEVICE: a launch the HIP runtime refused.
 */
int vimg_moments_accumulate(const VimgMomentsFrames* cur, const void* d_prev_history, const float prev_world_to_pixel[12],
                            const VimgMomentsParams* params, void* d_next_history, void* d_out_rgb, void* d_out_variance,
                            void* stream);

const char* vimg_moments_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
