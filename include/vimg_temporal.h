/*
 * vimg_temporal.h — C ABI of libvimg_temporal.so: temporal accumulation over frames that are already in device
 * memory (gfx950).  The last preview is reprojected into a moved camera and blended with the current frame.
 *
 * A third library beside libvimg_hip.so and libvimg_filter.so: it reads frames and no scene, so it needs neither a
 * VimgDeviceScene nor an entry point of the render library or of the filter library, whose ABIs stay closed
 * (DESIGN.md 4.19).  It links the HIP runtime and nothing of the other two; this header includes vimg_hip.h for the
 * VIMG_E_* codes alone.
 *
 * Conventions, as in vimg_filter.h: a call returns VIMG_OK or a negative VIMG_E_* code,
 * vimg_temporal_last_error() returns the message of the calling thread's last failure.  A call only ENQUEUES on
 * `stream` (NULL = HIP's null stream): the library has no stream of its own, allocates nothing and waits for
 * nothing; buffers belong to the caller and must stay alive until the stream has passed the call.  Argument errors
 * (VIMG_E_INVALID) are found before anything is enqueued and give the same answer on a machine without a GPU.
 */
#ifndef VIMG_TEMPORAL_H
#define VIMG_TEMPORAL_H

#include <stdint.h>

#include "vimg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIMG_TEMPORAL_MAX_EXTENT 32768u        /* largest width and height */
#define VIMG_TEMPORAL_HISTORY_PER_PIXEL 48u

/* The CURRENT picture: DEVICE pointers, float32 packed triples, tightly packed rows, 4-byte aligned - the shapes of
 * VimgFilterFrames (vimg_filter.h), i.e. of vimg_hip_render and the first-hit feature integrators at tile_world == 1. */
typedef struct VimgTemporalFrames {
  uint32_t struct_size, width, height, reserved;
  const void* color;      /* w*h rgb triples: one frame, or the running mean of current_weight frames        */
  const void* normal;     /* w*h xyz  (the `normal` feature frame)                                          */
  const void* position;   /* w*h xyz  (`position`): world-space first hits                                  */
  const void* depth;      /* w*h triples t t t (`depth`); the first component is read                       */
} VimgTemporalFrames;

/* Defaults (vimg_temporal_defaults): max_history 32, current_weight 1, sigma_normal 0.1, sigma_plane 0.00005 - see
 * "Defaults" below. */
typedef struct VimgTemporalParams {
  uint32_t struct_size, reserved;
  float max_history;     /* >= 1, finite: cap of a pixel's history length, i.e. the blend factor never falls below
                          * 1 / max_history */
  float current_weight;  /* >= 1, finite: weight of the current frame (1 for a single frame; k when `color` is a
                          * running mean of k frames) */
  float sigma_normal;    /* > 0, finite: 1 - n_p . n_q below which a history tap is the same surface */
  float sigma_plane;     /* > 0, finite: distance of the tap's old position from p's tangent plane, as a fraction of
                          * p's depth, below which it is the same surface */
} VimgTemporalParams;

/* struct_size and the defaults above. */
void vimg_temporal_defaults(VimgTemporalParams* params);

/*
 * Bytes of one history of a w x h picture: 48 per pixel (0 x 0 is 0).  A HISTORY is three planes of w*h float4,
 * laid out [3][h][w], 16-byte aligned, in the row order of the frames:
 *   A  = {r, g, b, L}      the accumulated radiance and the history length L; L == 0: the pixel holds no surface
 *   G0 = {n.x, n.y, n.z, z}  the guides the radiance was accumulated under (z: depth)
 *   G1 = {P.x, P.y, P.z, 0}  the world-space position
 * A caller may inspect it.
 */
uint64_t vimg_temporal_history_bytes(uint32_t width, uint32_t height);

/*
 * One step of temporal accumulation: reads the current frames and the previous history `d_prev_history` (or NULL:
 * no history), writes the next history `d_next_history` and, when `d_out_rgb` is not NULL, plane A's rgb as w*h
 * packed triples.  The caller ping-pongs two history buffers.  `prev_world_to_pixel`: 12 floats in HOST memory, the
 * row-major 3 x 4 matrix that takes a world-space point to homogeneous pixel coordinates (hx, hy, hw) of the picture
 * the previous history was rendered as - column hx / hw and row hy / hw in FRAME ARRAY coordinates, where pixel
 * (x, y) of the arrays covers [x, x + 1] x [y, y + 1]; it may be NULL with a NULL history.  d_next_history must not
 * overlap the previous history or any frame; d_out_rgb may be frames->color itself (each lane reads its own colour
 * before it writes) and must not overlap anything else: not the histories, not a guide frame, not the colour frame
 * partly.  One kernel launch on `stream`, one lane per pixel.
 *
 * The contract, which a float32 restatement reproduces BIT FOR BIT (tests/temporal_ref.py): everything is float32
 * with IEEE + - * /, comparisons and floorf - no fused multiply-add, no fmaxf / fminf - evaluated in the order
 * written.  For pixel p at column x, row y of the frame arrays, with M = prev_world_to_pixel, w, h as floats:
 *
 *   z = depth_p.x;  C = color_p;  n = normal_p;  P = position_p;  next.G0 = {n, z};  next.G1 = {P, 0}
 *   not live (!(z > 0)):   next.A = {C, 0}
 *   live, and any of: prev == NULL; !(hw > 0); !(fx > -1 && fx < w && fy > -1 && fy < h); !(sumb > 0):
 *                          next.A = {C, 1}
 *     hx = ((M0 P.x + M1 P.y) + M2 P.z) + M3,  hy from M4..7,  hw from M8..11
 *     fx = hx / hw - 0.5;  fy = hy / hw - 0.5;  x0 = floorf(fx), tx = fx - x0;  y0 = floorf(fy), ty = fy - y0
 *     taps q in the order (x0, y0) (x0 + 1, y0) (x0, y0 + 1) (x0 + 1, y0 + 1),
 *     b = (1 - tx) (1 - ty),  tx (1 - ty),  (1 - tx) ty,  tx ty
 *     a tap counts when q is inside the image, b > 0, L_q > 0 and
 *       dn = 1 - ((n.x nq.x + n.y nq.y) + n.z nq.z);   dn < sigma_normal
 *       e = Pq - P;  d = (n.x e.x + n.y e.y) + n.z e.z;  d d < (sigma_plane z) (sigma_plane z)
 *     counted taps add, in tap order, b to sumb, b Hq (rgb of A_q) to sumh, b L_q to suml
 *   otherwise:  H = sumh / sumb;  L = suml / sumb;  N = L + current_weight;  if (N > max_history) N = max_history
 *               a = current_weight / N;  if (a > 1) a = 1;  next.A = {H + (C - H) a, N}
 *
 * A NaN anywhere in a comparison makes it false: a NaN guide gives "no history" (length 1, or 0 for a NaN depth), and
 * a NaN history colour reaches only the pixels that tap it with b > 0.
 *
 * Known limits.  Correlated noise: the renderer seeds a pixel's random stream by its image index, so frames rendered
 * after a reset repeat their random numbers per pixel and history only adds information where the motion is at least
 * about a pixel.  Stale shading: history is reprojected radiance, so view-dependent shading and edits of the scene lag
 * behind and fade at 1 / max_history per frame.  Silhouettes: partly covered pixels carry coverage-scaled guides, as in
 * vimg_filter.h; they match few taps and mostly restart.  Thin lens: a world-to-pixel matrix describes a pinhole.
 *
 * Defaults.  Checked on the GPU (tools/temporal_cost.py; DESIGN.md 4.19 has the tables) over an orbit of 8 steps of 1.5
 * degrees, about 3 px of motion per step, mis at 4 spp, on cornell_box_spheres (64 x 64, 256 x 256) and disney_spheres
 * (450 x 200), by e = mean((x - ref)^2 / (ref^2 + 0.01)) of the last accumulated frame over the last noisy frame's, against
 * mis at 1024 spp, for max_history 2 .. 32 x sigma_normal 0.02 .. 0.5 x sigma_plane 0.00001 .. 0.01 (three sweeps):
 *   max_history 32, sigma_normal 0.1, sigma_plane 0.00005:  e_temporal / e_noisy = 0.182, 0.079 (cornell), 0.186 (disney).
 *   sigma_plane decides, and the starting value 0.01 does not survive: cornell's light lies one unit below the ceiling,
 *   1100 away, same normal - at sigma_plane 0.0005 and above the two are one surface, every step smears the light's
 *   radiance of 15 a pixel further over the ceiling, and the ratio is 34.6, 8.5 (0.0005) and 37.2, 10.3 (0.001 .. 0.01) - far
 *   worse than the noisy frame.  Below that, sigma_plane 0.0002 / 0.0001 / 0.00005 / 0.00002 / 0.00001 give 0.167 / 0.181 /
 *   0.182 / 0.182 / 0.182 (cornell 64 x 64), 0.076 / 0.077 / 0.079 / 0.089 / 0.111 (256 x 256) and 0.412 / 0.246 / 0.186 /
 *   0.180 / 0.200 (disney): geometric mean 0.174 / 0.151 / 0.139 / 0.143 / 0.159, lowest at 0.00005.  sigma_normal 0.02 and
 *   0.1 give the same figures to three digits, 0.5 moves them by under 0.03.  max_history 2 / 4 / 8 / 16 and 32 at
 *   sigma_plane 0.00005: 0.391 / 0.228 / 0.184 / 0.182 (cornell 64 x 64), 0.316 / 0.132 / 0.081 / 0.079 (256 x 256),
 *   0.341 / 0.198 / 0.185 / 0.186 (disney); 16 and 32 are the same because the orbit has nine frames.
 *
 * VIMG_E_INVALID, each with its sentence: a NULL frames / params / next history / color / normal / position / depth
 * pointer; a struct_size below the struct's; width or height 0 or above 32768; max_history or current_weight below 1,
 * NaN or infinite; sigma_normal or sigma_plane <= 0, NaN or infinite; a next or a non-NULL previous history that is
 * not 16-byte aligned; a NULL matrix with a non-NULL previous history; a NaN or infinite matrix entry; a next history
 * that overlaps the previous one or a frame; an output that overlaps a history, a guide frame, or the colour frame
 * without being it.  VIMG_E_DEVICE: a launch the HIP runtime refused.
 */
int vimg_temporal_accumulate(const VimgTemporalFrames* cur, const void* d_prev_history,
                             const float prev_world_to_pixel[12], const VimgTemporalParams* params,
                             void* d_next_history, void* d_out_rgb, void* stream);

const char* vimg_temporal_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
