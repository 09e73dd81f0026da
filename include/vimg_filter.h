/*
 * vimg_filter.h — C ABI of libvimg_filter.so: filters over frames that are already in device memory (gfx950).
 *
 * A library of its own beside libvimg_hip.so: a filter over frames reads no scene, so it needs neither a
 * VimgDeviceScene nor an entry point or an integrator value of the render library, whose ABI stays closed
 * (DESIGN.md 4.18).  It links the HIP runtime and nothing of libvimg_hip; this header includes vimg_hip.h for the
 * VIMG_E_* codes alone.
 *
 * Conventions: a call returns VIMG_OK or a negative VIMG_E_* code, vimg_filter_last_error() returns the message of
 * the calling thread's last failure.  A call only ENQUEUES on `stream` (NULL = HIP's null stream): the library has
 * no stream of its own, allocates nothing and waits for nothing; buffers belong to the caller and must stay alive
 * until the stream has passed the call.  Argument errors (VIMG_E_INVALID) are found before anything is enqueued
 * and give the same answer on a machine without a GPU.
 */
#ifndef VIMG_FILTER_H
#define VIMG_FILTER_H

#include <stdint.h>

#include "vimg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIMG_FILTER_MAX_EXTENT 32768u      /* largest width and height */
#define VIMG_ATROUS_MAX_ITERATIONS 12u
#define VIMG_ATROUS_WORKSPACE_PER_PIXEL 64u

/* The frames of one picture: DEVICE pointers, float32, tightly packed rows, 4-byte aligned.  These are the
 * shapes of vimg_hip_render and of the first-hit feature integrators (vimg_hip.h) at tile_world == 1. */
typedef struct VimgFilterFrames {
  uint32_t struct_size, width, height, reserved;
  const void* color;      /* w*h rgb triples, any row order as long as all frames share it                */
  const void* normal;     /* w*h xyz  (the `normal` feature frame)                                         */
  const void* position;   /* w*h xyz  (`position`)                                                         */
  const void* depth;      /* w*h triples t t t (`depth`); the first component is read                      */
  const void* albedo;     /* w*h rgb (`albedo`), or NULL: no demodulation                                  */
} VimgFilterFrames;

/* Parameters of the edge-avoiding a-trous filter.  Defaults (vimg_filter_atrous_defaults): 3 iterations,
 * sigma_color 2, sigma_normal 0.5, sigma_plane 0.005, albedo_floor 1/64 - see "Defaults" below. */
typedef struct VimgAtrousParams {
  uint32_t struct_size, iterations;    /* 1..12 */
  float sigma_color;     /* > 0, may be +inf (the colour term is then 0 for finite colours); halves per iteration */
  float sigma_normal;    /* > 0, finite: 1 - n_p . n_q at which a tap's weight reaches 0 */
  float sigma_plane;     /* > 0, finite: distance of a tap from p's tangent plane, as a fraction of p's depth, at
                          * which the weight reaches 0 */
  float albedo_floor;    /* > 0, finite: albedo components at or below it demodulate by it instead.  A power of
                          * two keeps the bits of pixels without albedo (misses): x / f * f is then exact */
} VimgAtrousParams;

/* struct_size and the defaults above. */
void vimg_filter_atrous_defaults(VimgAtrousParams* params);

/* Bytes of workspace vimg_filter_atrous needs for a w x h picture: 64 per pixel - two colour planes (ping-pong)
 * and two guide planes of float4 - whatever the arguments (0 x 0 is 0). */
uint64_t vimg_filter_atrous_workspace(uint32_t width, uint32_t height);

/*
 * The edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with Tukey's biweight as the edge-stopping
 * function, over a noisy colour frame and the first-hit guides beside it.  iterations + 2 kernel launches on
 * `stream`.  d_out_rgb (w*h rgb triples) may be frames->color itself; it must not overlap any other frame or the
 * workspace.  d_workspace: 16-byte aligned, at least vimg_filter_atrous_workspace(w, h) bytes.
 *
 * The contract, which a float32 restatement reproduces BIT FOR BIT (tests/atrous_ref.py): everything is float32
 * with IEEE + - * / and comparisons - no fused multiply-add, no fmaxf / fminf, no exp - evaluated in the order
 * written.
 *
 *   Pack.  For every pixel: a~ = albedo > floor ? albedo : floor per component (1 without an albedo frame),
 *   C = color / a~, G0 = {n.xyz, z}, G1 = {P.xyz, 0}.  A pixel is LIVE when z > 0 (misses and NaN depths are not).
 *
 *   Iteration i = 0 .. iterations - 1, ping-pong on C.  Step s = 2^i, taps q = p + s (dx, dy), dy = -2..2 outer,
 *   dx = -2..2 inner, k = h[dx + 2] h[dy + 2] with h = {1/16, 1/4, 3/8, 1/4, 1/16}.  A pixel that is not live
 *   copies its C.  For a live p the centre tap has w = k, a tap outside the image or not live has w = 0, and
 *   every other tap
 *     dn  = 1 - ((n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z)        s_n = dn < 0 ? 0 : dn / sigma_normal
 *     e   = P_q - P_p;  d = (n_p.x e.x + n_p.y e.y) + n_p.z e.z     s_p = (d d) / ((sigma_plane z_p) (sigma_plane z_p))
 *     dc  = C_p - C_q;  sc_i = sigma_color 2^-i (host, float)       s_c = ((dc.x^2 + dc.y^2) + dc.z^2) / (sc_i sc_i)
 *     S   = (s_n + s_p) + s_c                                       w   = S < 1 ? k ((1 - S) (1 - S)) : 0
 *   (a NaN anywhere in S gives w = 0).  Taps with w > 0 add w to sumw and w C_q to sumc, in tap order; the result
 *   is sumc / sumw per component.  sumw >= 9/64 always: there is no 0 / 0.
 *
 *   Unpack.  out = C a~, packed triples.
 *
 * Known limit: the feature frames are antialiased means in which a miss counts as 0, so the guides of partly
 * covered silhouette pixels are scaled by coverage; such pixels match few neighbours and mostly keep their value.
 *
 * Defaults.  Chosen on the GPU on cornell_box_spheres (512 x 512) and disney_spheres (900 x 400), mis at 4 and 16 spp
 * with their albedo frame, against mis at 1024 spp, by the relative squared error e = mean((x - ref)^2 / (ref^2 + 0.01))
 * of the filtered frame over the noisy frame's, geometric mean of the four (two sweeps, 384 + 280 settings; DESIGN.md
 * 4.18 has the tables):
 *   iterations 3, sigma_color 2, sigma_normal 0.5, sigma_plane 0.005:  e_filtered / e_noisy = 0.029, 0.048 (cornell at
 *   4, 16 spp), 0.085, 0.141 (disney); 2 iterations: 0.038, 0.050, 0.093, 0.111; 5 iterations: 0.049, 0.138, 0.090, 0.172.
 *   sigma_color decides: at 3 iterations the mean ratio is 0.064 at sigma_color 2 against 0.12 at 1, 0.13 at 4 and 0.47
 *   at +inf, where disney at 16 spp comes out WORSE than the noisy frame (1.99): the guides know nothing of shadow
 *   edges and reflections, the colour term does.  sigma_normal (0.1 / 0.5) and sigma_plane (0.005 / 0.05) move the
 *   mean by under 0.005; albedo_floor (1/256, 1/64, 1/16) by under 0.0002, so it is the power of two in the middle.
 *   Small pictures take less filtering: cornell at 64 x 64 gives 0.29 (4 spp) and 0.82 (16 spp) at 3 iterations, 0.18
 *   and 0.41 at 2.
 *
 * VIMG_E_INVALID, each with its sentence: a NULL frames / params / color / normal / position / depth / out /
 * workspace pointer; a struct_size below the struct's; width or height 0 or above 32768; iterations outside 1..12;
 * a sigma or the albedo floor <= 0 or NaN, or infinite (sigma_color alone may be +inf); a workspace too small or
 * not 16-byte aligned.  VIMG_E_DEVICE: a launch the HIP runtime refused.
 */
int vimg_filter_atrous(const VimgFilterFrames* frames, const VimgAtrousParams* params, void* d_out_rgb,
                       void* d_workspace, uint64_t workspace_bytes, void* stream);

const char* vimg_filter_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
