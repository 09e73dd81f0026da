// What the libraries that reproject a history share (libvimg_temporal.so, libvimg_moments.so, libvimg_wtemporal.so,
// libvimg_demand.so): the reprojection of include/vimg_temporal.h's contract, from the projection of a
// pixel's surface point to the weighted means of its accepted history taps; the check of a previous history and its
// matrix; and the argument checks of a call that also takes a next history and outputs.  Internal, like frame_lib.h,
// which a unit includes first: shared source in an anonymous namespace, compiled into every library that includes it,
// never a dynamic symbol.
#pragma once

namespace vimg_frames {
namespace {

// the kernel arguments of the reprojection
struct Reprojection {
  float m[12];     // prev_world_to_pixel, row-major 3 x 4
  float sigma_normal, sigma_plane;
};

// the bilinear means of the accepted taps: plane A's {r, g, b, L}, and the weight they were divided by
struct Reprojected {
  float hr, hg, hb, len, sumb;
};

// Looks the live pixel with normal n, position P and depth z up in `prev` (planes A, G0, G1 of w x h float4 each;
// null: no history): true, and `r`, when a tap counts.  `tap(b_i, q)` is called once per ACCEPTED tap, in tap order
// 0..3, with its bilinear weight and its pixel index - for what a library sums from further planes, which a rejected
// tap then never touches.  The operations and their order are the contract's.
template <class Tap>
__device__ inline bool reproject(uint32_t w, uint32_t h, const float4* __restrict__ prev, const Reprojection& k, float nx,
                                 float ny, float nz, float px, float py, float pz, float z, Reprojected& r, Tap&& tap) {
  if (!prev) return false;
  const float hx = ((k.m[0] * px + k.m[1] * py) + k.m[2] * pz) + k.m[3];
  const float hy = ((k.m[4] * px + k.m[5] * py) + k.m[6] * pz) + k.m[7];
  const float hw = ((k.m[8] * px + k.m[9] * py) + k.m[10] * pz) + k.m[11];
  if (!(hw > 0.f)) return false;
  const float fx = hx / hw - 0.5f, fy = hy / hw - 0.5f;
  if (!(fx > -1.f && fx < float(w) && fy > -1.f && fy < float(h))) return false;
  const float x0 = floorf(fx), y0 = floorf(fy);      // -1 .. w - 1, -1 .. h - 1: exact as int
  const float tx = fx - x0, ty = fy - y0;
  const float ux = 1.f - tx, uy = 1.f - ty;
  const float b[4] = {ux * uy, tx * uy, ux * ty, tx * ty};
  const int ix = int(x0), iy = int(y0);
  const size_t n = size_t(w) * h;
  const float sz = k.sigma_plane * z;
  const float plane = sz * sz;
  float sumb = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sl = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int qx = ix + (i & 1), qy = iy + (i >> 1);
    if (uint32_t(qx) >= w || uint32_t(qy) >= h) continue;
    if (!(b[i] > 0.f)) continue;
    const size_t q = size_t(qy) * w + size_t(qx);
    const float4 hq = prev[q];
    if (!(hq.w > 0.f)) continue;
    const float4 nq = prev[n + q];
    const float dn = 1.f - ((nx * nq.x + ny * nq.y) + nz * nq.z);
    if (!(dn < k.sigma_normal)) continue;
    const float4 pq = prev[2 * n + q];
    const float ex = pq.x - px, ey = pq.y - py, ez = pq.z - pz;
    const float d = (nx * ex + ny * ey) + nz * ez;
    if (!(d * d < plane)) continue;
    tap(b[i], q);
    sumb = sumb + b[i];
    sr = sr + b[i] * hq.x;
    sg = sg + b[i] * hq.y;
    sb = sb + b[i] * hq.z;
    sl = sl + b[i] * hq.w;
  }
  if (!(sumb > 0.f)) return false;
  r = {sr / sumb, sg / sumb, sb / sumb, sl / sumb, sumb};
  return true;
}

// ---- the host half: what vimg_*_accumulate checks after check_head and its own parameters --------------------------
// a frame the kernel reads beside the shared four (null: not given); `align`: its bytes, 0 for "any"
struct ReadFrame {
  const void* p;
  uint64_t bytes;
  const char* name;
  uint32_t align = 0;
};

// an output beside d_out_rgb (null: not asked for): `says` opens its sentences ("output codes overlap"), `own` is the
// index in `reads` of the one frame it may be itself, -1 for none
struct ExtraOutput {
  const void* p = nullptr;
  uint64_t bytes = 0;
  const char* says = "";
  int own = -1;
};

// the history a call reprojects (null: none) and the matrix it is projected with, which is copied to `k`
int check_previous(const void* prev, const float* matrix, Reprojection& k) {
  if (prev) {
    if (misaligned(prev, 16)) return fail(VIMG_E_INVALID, FRAME_LIB ": the previous history must be 16-byte aligned");
    if (!matrix) return fail(VIMG_E_INVALID, FRAME_LIB ": a previous history needs its world-to-pixel matrix");
  }
  if (matrix)
    for (int i = 0; i < 12; ++i) {
      if (!std::isfinite(matrix[i]))
        return fail(VIMG_E_INVALID, FRAME_LIB ": world-to-pixel entry %d is not finite (%g)", i, double(matrix[i]));
      k.m[i] = matrix[i];
    }
  return VIMG_OK;
}

// In this order: the alignment of the next history and of `reads`; check_previous; what the next history must not
// overlap; what d_out_rgb must not - other lanes gather from prev and read the guides, so of all frames only the
// colour frame itself may be the output; the same for `extra`, whose own frame is looked at last.  `hist`: the bytes
// of one history.
template <class Frames>
int check_reprojection(const Frames* f, const void* prev, const float* matrix, const void* next, uint64_t hist,
                       std::span<const ReadFrame> reads, const void* out, const ExtraOutput& extra, Reprojection& k) {
  if (misaligned(next, 16)) return fail(VIMG_E_INVALID, FRAME_LIB ": the next history must be 16-byte aligned");
  for (const ReadFrame& r : reads)
    if (r.p && r.align && misaligned(r.p, r.align))
      return fail(VIMG_E_INVALID, FRAME_LIB ": the %s frame must be %u-byte aligned", r.name, r.align);
  if (const int rc = check_previous(prev, matrix, k)) return rc;
  const uint64_t frame = uint64_t(12) * f->width * f->height;
  if (prev && overlaps(next, hist, prev, hist))
    return fail(VIMG_E_INVALID, FRAME_LIB ": the next history overlaps the previous one");
  Range all[8] = {{f->color, frame, "color"}, {f->normal, frame, "normal"}, {f->position, frame, "position"}, {f->depth, frame, "depth"}};
  size_t n = 4;
  for (const ReadFrame& r : reads) all[n++] = {r.p, r.bytes, r.name};      // (a null one keeps its place and is passed over)
  const std::span<const Range> frames(all, n);
  if (const Range* r = first_overlap(next, hist, frames))
    return fail(VIMG_E_INVALID, FRAME_LIB ": the next history overlaps the %s frame", r->name);
  if (out) {
    if (prev && overlaps(out, frame, prev, hist)) return fail(VIMG_E_INVALID, FRAME_LIB ": the output overlaps the previous history");
    if (overlaps(out, frame, next, hist)) return fail(VIMG_E_INVALID, FRAME_LIB ": the output overlaps the next history");
    if (const Range* r = first_overlap(out, frame, frames.subspan(out == f->color ? 1 : 0)))
      return fail(VIMG_E_INVALID, r == all ? FRAME_LIB ": the output overlaps the %s frame without being it"
                                           : FRAME_LIB ": the output overlaps the %s frame", r->name);
  }
  if (extra.p) {
    Range own{};      // taken out of its place, to be looked at last
    if (extra.own >= 0) std::swap(own, all[4 + extra.own]);
    if (prev && overlaps(extra.p, extra.bytes, prev, hist))
      return fail(VIMG_E_INVALID, FRAME_LIB ": the %s the previous history", extra.says);
    if (overlaps(extra.p, extra.bytes, next, hist)) return fail(VIMG_E_INVALID, FRAME_LIB ": the %s the next history", extra.says);
    if (const Range* r = first_overlap(extra.p, extra.bytes, frames))
      return fail(VIMG_E_INVALID, FRAME_LIB ": the %s the %s frame", extra.says, r->name);
    if (out && overlaps(extra.p, extra.bytes, out, frame)) return fail(VIMG_E_INVALID, FRAME_LIB ": the %s the output", extra.says);
    if (extra.p != own.p && first_overlap(extra.p, extra.bytes, {&own, 1}))
      return fail(VIMG_E_INVALID, FRAME_LIB ": the %s the %s frame without being it", extra.says, own.name);
  }
  return VIMG_OK;
}

}  // namespace
}  // namespace vimg_frames
