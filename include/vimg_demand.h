/*
 * vimg_demand.h — C ABI of libvimg_demand.so: the sampling mask of a sparse preview, decided BEFORE the frame is
 * rendered from what the history will have to offer (gfx950).  A sparse preview (vimg_infill.h, vimg_wtemporal.h,
 * DESIGN.md 4.24) samples one pixel in stride^2 per frame on a lattice that knows nothing about the history: a pixel the
 * camera move has just uncovered waits up to stride^2 frames for its first sample with nothing to show but the fill.  This
 * library looks every pixel up in the previous history exactly as the accumulate call of the same frame will, and turns
 * "the lookup finds nothing" into "sample this pixel now": the mask is the lattice and, beside it, every live pixel whose
 * reprojected history is shorter than min_history.
 *
 * An eleventh frame library beside libvimg_filter.so ... libvimg_exposure.so: it reads frames, never a
 * scene, and calls no entry point of another library, whose ABIs stay closed.  It links the HIP runtime and none of the
 * project's libraries; this header includes vimg_hip.h for the VIMG_E_* codes alone.  The history is libvimg_temporal's -
 * 48 bytes per pixel, three planes of w*h float4 laid out [3][h][w], 16-byte aligned, A = {r, g, b, L},
 * G0 = {n.x, n.y, n.z, z}, G1 = {P.x, P.y, P.z, 0} (vimg_temporal.h); the first three planes of libvimg_moments' serve as
 * well.  It is only read.
 *
 * Conventions, as in vimg_wtemporal.h: a call returns VIMG_OK or a negative VIMG_E_* code, vimg_demand_last_error()
 * returns the message of the calling thread's last failure.  A call only ENQUEUES on `stream` (NULL = HIP's null
 * stream): the library has no stream of its own, allocates nothing, waits for nothing and reads nothing back - the
 * counts stay in device memory until the caller copies them; buffers belong to the caller and must stay alive until the
 * stream has passed the call.  Argument errors (VIMG_E_INVALID) are found before anything is enqueued and give the same
 * answer on a machine without a GPU.
 */
#ifndef VIMG_DEMAND_H
#define VIMG_DEMAND_H

#include <stdint.h>

#include "vimg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIMG_DEMAND_MAX_EXTENT 32768u        /* largest width and height */
#define VIMG_DEMAND_HISTORY_PER_PIXEL 48u    /* = VIMG_TEMPORAL_HISTORY_PER_PIXEL: the same history */
#define VIMG_DEMAND_MAX_STRIDE 4u            /* = vimg_amd.infill's largest lattice stride */
#define VIMG_DEMAND_COUNTS 4u                /* d_out_counts' words: masked, needed, extra, live */

/* The guides of the picture ABOUT TO BE rendered: DEVICE pointers, float32 packed triples, tightly packed rows, 4-byte
 * aligned.  There is no colour frame - the call runs before there is one - so this is not the eight shared fields of
 * the other frame libraries' structs. */
typedef struct VimgDemandFrames {
  uint32_t struct_size, width, height, reserved;
  const void* normal;     /* w*h xyz  (the `normal` feature frame)                                           */
  const void* position;   /* w*h xyz  (`position`): world-space first hits - or, when the history is reprojected
                           * through moved geometry (vimg_motion.h), the previous-world positions Q: whatever the
                           * accumulate call of this frame will be given                                        */
  const void* depth;      /* w*h triples t t t (`depth`); the first component is read                        */
} VimgDemandFrames;

/* Defaults (vimg_demand_defaults): stride 2, phase 0, min_history 1, sigma_normal 0.1, sigma_plane 0.00005 - see
 * "Defaults" below. */
typedef struct VimgDemandParams {
  uint32_t struct_size;
  uint32_t stride;       /* 0: no lattice, the mask is the needed pixels alone; 2..4: the lattice's stride            */
  uint32_t phase;        /* below stride^2 (0 at stride 0): which of the stride^2 lattices                            */
  uint32_t reserved;
  float min_history;     /* >= 0, finite: a live pixel whose reprojected history length is BELOW it is needed; 0: none is */
  float sigma_normal;    /* > 0, finite: vimg_temporal.h's; give the values the accumulate call of this frame gets   */
  float sigma_plane;     /* > 0, finite: likewise                                                                      */
} VimgDemandParams;

/* struct_size and the defaults above. */
void vimg_demand_defaults(VimgDemandParams* params);

/*
 * Writes the sampling mask of the frame whose guides are `cur`, against the previous history `d_prev_history` (or
 * NULL: no history) and its matrix `prev_world_to_pixel` (12 floats in HOST memory, vimg_temporal.h's; it may be NULL
 * with a NULL history).  d_out_mask: w*h uint8, 1 = sample this pixel (vimg_hip_progressive_render_masked's mask).
 * d_out_length: w*h float32, 4-byte aligned, the history length the lookup finds, or NULL.  d_out_counts:
 * VIMG_DEMAND_COUNTS uint32, 4-byte aligned, or NULL.  The history and the guides are only read; an output must overlap
 * neither them nor another output.
 *
 * The contract, which a float32 restatement reproduces BIT FOR BIT (tests/demand_ref.py): float32 + - * /,
 * comparisons and floorf - no fused multiply-add, no fmaxf / fminf - in the order written.  For pixel p = (x, y) in the
 * frames' row order:
 *
 *   z = depth_p.x;  live = z > 0
 *   (cx, cy) = (phase % stride, (phase / stride + phase % stride) % stride)     (integers: vimg_amd.infill.lattice_cell)
 *   lat  = stride != 0 && x % stride == cx && y % stride == cy
 *   L    = live and the history lookup finds a usable history ? suml / sumb : 0
 *          The lookup is vimg_temporal.h's, with n = normal_p, P = position_p and M = prev_world_to_pixel: "no usable
 *          history" is any of prev == NULL; !(hw > 0); !(fx > -1 && fx < w && fy > -1 && fy < h); !(sumb > 0) - with hx,
 *          hy, hw, fx, fy, the four taps, their weights b, the tap test (inside the image, b > 0, L_q > 0,
 *          dn < sigma_normal, d d < (sigma_plane z)(sigma_plane z)) and the sums sumb and suml exactly as written
 *          there, in its order.  The colour sums are not needed and plane A's rgb decide nothing.
 *   need = live && L < min_history
 *   mask_p   = lat || need ? 1 : 0
 *   length_p = L
 *   counts[0] += mask_p;  counts[1] += need;  counts[2] += need && !lat;  counts[3] += live
 *
 * The counts are zeroed by the call and are integers: the order in which they are added up cannot change a bit.
 *
 * What follows from it.  L is the length vimg_wtemporal_accumulate carries for a pixel of weight 0 on the same inputs
 * (its code 3, at a max_history above every length), and 0 where that call shows a pixel without carrying it (code 4)
 * or starts one (code 1): given the sigmas of that call, L is that call's own answer and not an estimate.  At
 * min_history 0 nothing is needed and the mask is the lattice's bytes.  With no previous history every live pixel is
 * needed (min_history > 0).  A pixel that is not live is never needed - no sample can give it a surface - but is masked on
 * its lattice turn like any other.  NaN rules are vimg_temporal.h's: a NaN guide gives no usable history, so the pixel
 * is needed if it is live; a NaN depth is not live; a NaN or non-positive history length is no tap.
 *
 * Known limits.  The lengths are those BEFORE this frame's increment: a caller that shortens the history afterwards
 * (vimg_antilag.h) has the pixels it cut demanded one frame later.  A pixel is needed or not, there is no budget: after
 * a cut every live pixel is needed and the frame is a full one.
 *
 * The launch.  One kernel launch on `stream`, one lane per pixel, workgroups of 64 x 4: a wave is 64 consecutive
 * pixels of one row, the current frame's reads and both per-pixel writes are contiguous per wave, the taps are
 * vimg_wtemporal_accumulate's gathers.  The counts are reduced per wave with a ballot and a population count, per
 * workgroup in LDS, and a workgroup ends with at most one atomic add per counter; the four words are cleared on the
 * stream before the kernel.
 *
 * Defaults.  stride 2 and phase 0 are placeholders a caller replaces per frame; the sigmas are vimg_temporal.h's.
 * min_history 1: less than one real sample's worth - a pixel that vimg_infill_reconstruct filled weighs 1/16
 * (vimg_amd.wtemporal.FILL_WEIGHT), so a history of fills alone stays below 1 for sixteen frames, and one real sample
 * reaches it.  Measured on the GPU (tools/demand_sweep.py; DESIGN.md 4.32 has the tables) over vimg_wtemporal.h's orbit,
 * strides 2 to 4, min_history 0 / 0.5 / 1 / 2 / 4: geometric mean of e over the three pictures and three strides 0.02077 /
 * 0.01878 / 0.01878 / 0.01729 / 0.01579 at 14.1 / 20.6 / 20.6 / 30.2 / 46.5 % of the pixels sampled per moved frame.  0 is
 * the lattice alone; 0.5 and 1 are one preview (with the call in use a history starts with a real sample, so no length
 * lies in (0, 1)); 2 and 4 buy their lower e with more samples, so the default stands.  Over the live pixels alone the
 * geometric mean is 0.03078 / 0.02358 / 0.02358 / 0.01994 / 0.01742 and every picture and stride gains.  On disney_spheres
 * at strides 3 and 4 the whole frame's e is nevertheless WORSE than the lattice alone (0.03614 -> 0.04886, 0.05917 ->
 * 0.09007 at 1): the misses next to a silhouette that was just sampled on demand are filled by vimg_infill_reconstruct,
 * which cannot tell a sampled miss from a sampled surface, and the dense surface samples bleed into them.
 *
 * Cost (tools/demand_cost.py on one MI355X): a call has a median of 0.061 ms at 450 x 200 and 0.128 ms at 1800 x 800
 * (device events around the Python call), 1.11 and 1.30 times vimg_temporal_accumulate against the same history in the
 * same run; with d_out_length and d_out_counts NULL 0.052 and 0.077 ms, and the lengths cost 0.002 of the difference:
 * the rest is the counters' same-address atomics.
 *
 * VIMG_E_INVALID, each with its sentence, in THIS ORDER when two faults meet: a NULL frames, then params pointer; a
 * frames, then params struct_size below the struct's; width or height 0 or above 32768; a NULL normal, position or
 * depth frame (in that order); a NULL mask; stride 1 or above 4; phase not below stride^2 (not 0 at stride 0);
 * min_history negative, NaN or infinite; sigma_normal, then sigma_plane <= 0, NaN or infinite; a previous history that
 * is not 16-byte aligned; a NULL matrix with a previous history; a NaN or infinite matrix entry (the lowest index); a
 * length, then counts output that is not 4-byte aligned; the mask overlapping the previous history, then the normal,
 * position or depth frame; the lengths overlapping those in that order, then the mask; the counts overlapping those
 * in that order, then the mask, then the lengths.  VIMG_E_DEVICE: the clear or the launch the HIP runtime refused.
 */
int vimg_demand_mask(const VimgDemandFrames* cur, const void* d_prev_history, const float prev_world_to_pixel[12],
                     const VimgDemandParams* params, void* d_out_mask, void* d_out_length, void* d_out_counts, void* stream);

const char* vimg_demand_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
