/*
 * vimg_exposure.h — C ABI of libvimg_exposure.so: histogram auto-exposure of a linear HDR frame in device memory
 * (gfx950), with the exposure state kept in device memory from frame to frame.  The preview stack turns a few samples
 * per pixel into a clean linear frame; this library gives that frame a sensible brightness.  It meters the frame's
 * luminance into a log2 histogram, takes the mean log luminance of the ranks between two permilles - so a firefly,
 * which is one rank among thousands, cannot move it, where the maximum that vimg_hip_post_rgb8's Reinhard operator
 * scales by IS the firefly - moves the exposure toward key / metered at a stated rate, and scales the frame by it.
 *
 * A frame library of its own beside libvimg_filter.so ... libvimg_despeckle.so: it reads
 * frames, never a scene, and calls no entry point of another library, whose ABIs stay closed.  It links the HIP runtime
 * and none of the project's libraries; this header includes vimg_hip.h for the VIMG_E_* codes alone.
 *
 * Conventions, as in vimg_despeckle.h: a call returns VIMG_OK or a negative VIMG_E_* code, vimg_exposure_last_error()
 * returns the message of the calling thread's last failure.  A call only ENQUEUES on `stream` (NULL = HIP's null
 * stream): the library has no stream of its own, allocates nothing, waits for nothing and reads nothing back - the
 * exposure a frame is scaled by never visits the host; buffers belong to the caller and must stay alive until the
 * stream has passed the call.  Argument errors (VIMG_E_INVALID) are found before anything is enqueued and give the same
 * answer on a machine without a GPU.
 */
#ifndef VIMG_EXPOSURE_H
#define VIMG_EXPOSURE_H

#include <stdint.h>

#include "vimg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIMG_EXPOSURE_MAX_EXTENT 32768u   /* largest width and height */
#define VIMG_EXPOSURE_BINS 256u           /* eight per octave over 2^-16 .. 2^16 */
/* The state, in DEVICE memory, 16-byte aligned:
 *   offset    0  uint32 hist[256]   the histogram; zero between calls
 *          1024  float  exposure    E, what the last call scaled by; meaningful once frames > 0
 *          1028  uint32 frames      the calls that metered something
 *          1032  float  metered     the luminance the last such call metered
 *          1036  uint32 counted     the pixels the last call counted (T)
 * 1040 zero bytes are a fresh state (hipMemsetAsync, torch.zeros): there is no init entry point.  While frames is 0 the
 * stored exposure is not read: the exposure of such a state IS 1, for Apply and for a reader. */
#define VIMG_EXPOSURE_STATE_BYTES 1040u
/* The meter kernel's grid is capped at this many workgroups of 256 lanes, which walk the frame in a grid-stride loop.
 * Every workgroup ends by adding its non-zero bins to the state's histogram, so the cap bounds those global atomics at
 * 256 x 256 = 65536 whatever the frame (one workgroup per 256 pixels of a 32768 x 32768 frame would flush 4 M times).
 * 256 is one workgroup for each of the MI355X's compute units.  It was first written as 512, two per unit, to have
 * more waves to hide the loads behind; measured at 1800 x 800 (meter and resolve, 50 calls back to back, per call, two
 * alternating rounds, in ms) the flush into 256 shared words outweighs that:
 *   cap     64             128            256            512            1024           2048
 *           0.0467 0.0469  0.0394 0.0394  0.0371 0.0371  0.0408 0.0403  0.0481 0.0479  0.0663 0.0658
 * (512 .. 2048 against 256 in one run, 64 .. 512 in another, where 256 read 0.0365 0.0364.)  At 450 x 200, 352
 * workgroups' worth of pixels, the caps do not differ by more than the runs do. */
#define VIMG_EXPOSURE_MAX_WORKGROUPS 256u

/* The frame: DEVICE pointers, tightly packed rows, 4-byte aligned. */
typedef struct VimgExposureFrames {
  uint32_t struct_size, width, height, reserved;
  const void* color;   /* w*h rgb triples, float32                                                      */
  const void* depth;   /* w*h triples t t t (`depth`; the first component is read), or NULL: every pixel is metered */
} VimgExposureFrames;

/* Defaults (vimg_exposure_defaults): low 500, high 950, key 0.18, min 1/64, max 64, rate_brighten 0.25,
 * rate_darken 0.5 - see "Defaults" below. */
typedef struct VimgExposureParams {
  uint32_t struct_size;
  uint32_t low_permille, high_permille;  /* 0 <= low < high <= 1000: the ranks [T low / 1000, T high / 1000) are metered */
  float key;                             /* > 0, finite: the luminance the metered luminance is brought to              */
  float min_exposure, max_exposure;      /* 0 < min <= max, finite: the target exposure is clamped to them              */
  float rate_brighten, rate_darken;      /* (0, 1]: the share of the way to the target a call goes; the exposure falls
                                          * faster than it rises, as an eye's does                                      */
} VimgExposureParams;

/* struct_size and the defaults above. */
void vimg_exposure_defaults(VimgExposureParams* params);

/*
 * Meters `color`, moves the exposure in d_state and, when d_out_rgb is given, writes color times that exposure.
 * Two kernel launches on `stream` (meter, resolve), three with an output (apply).  d_state: VIMG_EXPOSURE_STATE_BYTES,
 * 16-byte aligned, read and written.  d_out_rgb: w*h rgb triples, or NULL: meter only; it may be frames->color itself -
 * in place is the preview's normal use - and must not overlap anything else.
 *
 * The contract, which a numpy restatement reproduces BIT FOR BIT, the state's bytes and the output both
 * (tests/exposure_ref.py): integer arithmetic and float32 + - * / in the order written; no fused multiply-add, no
 * transcendental, comparisons instead of fmaxf / fminf.
 *
 *   Meter, every pixel.  L = (r 0.212671 + g 0.715160) + b 0.072169, the luminance of vimg_varfilter.h.  The pixel is
 *   COUNTED when L > 0 and L < +inf (a NaN fails both) and (depth == NULL or z > 0).  Its bin is a piecewise-linear
 *   log2, eight bins per octave, read from the float's bits: k = int(bits(L) >> 20) - 888, clamped to 0..255 - the
 *   exponent and the top three bits of the mantissa.  Bin 0 starts at 2^-16 and takes everything below, denormals
 *   included; bin 255 ends at 2^16 and takes everything above.  hist[k] += 1: integers, so the order of the atomic
 *   additions cannot change a bit.
 *
 *   Resolve, once.  T = sum of hist;  lo = T low_permille / 1000,  hi = T high_permille / 1000  (uint64, integer
 *   division).
 *     T == 0 or hi == lo    exposure, metered and frames keep their values; counted = T.
 *     otherwise             The counted pixels have ranks 0 .. T - 1, ascending by bin.
 *                             S = sum over bins b of  b * |ranks of bin b within [lo, hi)|        (uint64)
 *                             m = float(S) / float(hi - lo)        (each conversion rounds to nearest even)
 *                             i = floor(m) as an integer,  f = m - float(i)
 *                             edge(b) = float_from_bits((b + 888) << 20)        (bin b starts there; edge(256) = 2^16)
 *                             metered = edge(i) + f * (edge(i + 1) - edge(i))
 *                             E* = key / metered;  if E* < min, E* = min;  if E* > max, E* = max
 *                             frames == 0:  E' = E*
 *                             otherwise:    E' = E + (E* - E) * rate,  rate = rate_darken when E* < E, else rate_brighten
 *                             exposure = E',  metered,  frames += 1,  counted = T
 *     In both cases hist is zero again when the kernel ends.
 *
 *   Apply, when d_out_rgb is given, every pixel.  out = c * E' per component, E' read from the state in device
 *   memory: 1 while frames == 0, else exposure.
 *
 * What follows from it.  A NaN or infinite colour stays what it is (NaN E' = NaN, inf E' = inf: E' is finite and
 * above 0) and is not metered: the post chain's NaN rule stays visible.  Misses are scaled like everything else; with
 * a depth frame they are not metered.  An all-black frame (T == 0) leaves the exposure where it was instead of
 * driving it to max_exposure.  One bright pixel is one rank: among T counted pixels it moves S by at most 255, m by at
 * most 255 / (hi - lo) of a bin.  The bins are equal steps of the MANTISSA, not of the logarithm: L -> k is the float's
 * own piecewise-linear log2, exact at the powers of two and up to 0.086 octave (6 %) off a true log2 between them, and
 * edge() with its linear interpolation inverts exactly that map.  A pixel counts as its bin's START, so a frame of one
 * luminance L meters within one bin (a sixteenth to an eighth of L) below L, and `metered` lies below the geometric mean
 * of the windowed luminances, which a true log of every pixel would give, by at most that bin (an eighth of an octave)
 * and the 0.086 octave: up to 14 %, about half of it on a spread-out frame.  It is the same bias on every frame, so it
 * cannot flicker, and it is inside what key is chosen to.
 *
 * Known limits.  One global exposure: no local operator, no highlight roll-off - a tonemapper (vimg_hip_post_rgb8)
 * still follows.  Radiance outside 2^-16 .. 2^16 is metered as the range's ends.  The adaptation is per CALL, not per
 * second: a caller with a varying frame time scales the rates itself.  The command-line program does not use it.
 *
 * Defaults.  low 500, high 950: the upper half of the counted pixels without the brightest twentieth - a preview's
 * picture is read by its lit surfaces, not by its shadows, and its fireflies and light sources sit in the top ranks.
 * key 0.18 is the photographic middle grey; min 1/64 and max 64 are six stops either way; rate_brighten 0.25,
 * rate_darken 0.5.  Measured on the GPU (tools/exposure_sweep.py --permilles: a standing camera, mis, 16 independent
 * frames of 4 spp, and the same through temporal_preview; DESIGN.md 4.31 has the tables), the largest frame-to-frame
 * relative change of E* at the defaults against that of 1 / max luminance, Reinhard's scale:
 *                                                        E*, raw 4 spp   1 / max, raw   E*, preview   1 / max, preview
 *   cornell_box_spheres 64 x 64                          2.5 %           0.0 %          0.9 %         5.6 %
 *   disney_spheres 450 x 200                             1.0 %           0.0 %          0.6 %         0.3 %
 *   cornell_box_spheres 64 x 64, the light out of view   2.4 %           61.5 %         0.5 %         35.6 %
 * Where the camera sees a light source its radiance is every frame's maximum, and Reinhard's scale is steady (and dark);
 * as soon as the maximum is a highlight or a firefly it jumps by half from frame to frame, and E* does not.  The
 * defaults stand, the sweep gave no reason to move them: over the windows 0-1000, 100-900, 250-750, 500-950, 500-990,
 * 500-1000 and 800-990 permille E*'s largest change on the raw cornell frames is 17.5, 6.0, 4.4, 2.5, 2.4, 2.2 and 4.2 % -
 * what flickers at 4 spp is the bottom of the histogram, every window from the median up is steady to within what 16
 * frames resolve, and the top twentieth stays out for the outliers the sweep's scenes do not have.
 *
 * Cost (tools/exposure_cost.py on one MI355X): a call in place - three launches - has a median of
 * 0.048 ms at 450 x 200 and 0.064 ms at 1800 x 800 (device events around the Python call), 0.97 and 0.65 times
 * vimg_temporal_accumulate against a history in the same run (0.050 and 0.098 ms); despeckle's clamp 0.052 and 0.090 ms.
 * A frame of one colour, where every lane of a wave adds to the same LDS word, is not slower than a log-uniform one.
 *
 * VIMG_E_INVALID, each with its sentence: a NULL frames / params / color / state pointer; a struct_size below the
 * struct's; width or height 0 or above 32768; a state that is not 16-byte aligned; low_permille >= high_permille or
 * high_permille above 1000; key, min_exposure or max_exposure <= 0, NaN or infinite; min_exposure > max_exposure; a
 * rate <= 0, above 1, NaN or infinite; an output that overlaps the colour frame without being it, or the depth frame
 * or the state; a state that overlaps the colour or the depth frame.  VIMG_E_DEVICE: a launch the HIP runtime refused.
 */
int vimg_exposure_adapt(const VimgExposureFrames* frames, const VimgExposureParams* params, void* d_state, void* d_out_rgb,
                        void* stream);

const char* vimg_exposure_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
