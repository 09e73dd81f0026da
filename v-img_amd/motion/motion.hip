// libvimg_motion.so: the previous-world position of include/vimg_motion.h.
//
// One kernel, frames/frame_lib.h's launch shape: one lane per pixel, blockDim (64, 4), a wave is 64 consecutive pixels
// of a row.  Per wave the hits are 1 KiB read contiguously (one 16-byte load per lane), the position triples 768
// contiguous bytes, the output triples and the 64 code bytes likewise.  What costs are the gathers, and only lanes
// that hit issue them: the pixel's VimgPrim (8 B), then for a triangle its row of tri_vertices (12 B) and six vertex
// rows (12 B each), for a sphere the two sphere records (16 B each) and the pixel's ray (two 16-byte loads,
// contiguous over the wave's sphere lanes).  Neighbouring pixels mostly hit the same or an adjacent triangle, so a
// wave's gathers fall into few cache lines.  No LDS, no loop.
//
// EVERY gather is bounds-tested here: the tables and the hits come from a caller, and an index that is out of range
// gets code 3 and reads nothing behind it.
//
// The arithmetic is the header's contract, operation for operation: built with -ffp-contract=off and without
// fast-math, so + - * / round once each.
#include "vimg_motion.h"

#define FRAME_LIB "motion"
#include "../frames/frame_lib.h"

namespace vimg_motion {

using namespace vimg_frames;

struct Tables {
  uint32_t num_prims, num_tris, num_vertices, num_spheres;
  const uint2* prims;            // {type, index}
  const uint32_t* tri_vertices;
  const float* old_vertices;     // both NULL or both set
  const float* new_vertices;
  const float4* old_spheres;     // both NULL or both set
  const float4* new_spheres;
};

__global__ __launch_bounds__(WAVE_X * ROWS) void motion_previous_kernel(uint32_t w, uint32_t h, const float* __restrict__ position,
                                                                        const float4* __restrict__ hits,
                                                                        const float4* __restrict__ rays, Tables g,
                                                                        float* __restrict__ previous,
                                                                        uint8_t* __restrict__ code_out) {
  int x, y;
  if (!pixel_of(w, h, x, y)) return;
  const size_t q = size_t(y) * w + size_t(x);
  const float px = position[3 * q], py = position[3 * q + 1], pz = position[3 * q + 2];
  const float4 hit = hits[q];                       // {t, prim, b1, b2}
  const uint32_t prim = __float_as_uint(hit.y);
  float dx = 0.f, dy = 0.f, dz = 0.f;
  uint32_t code = VIMG_MOTION_STATIC;
  if (prim != VIMG_NO_HIT) {
    code = VIMG_MOTION_OUT_OF_RANGE;
    if (prim < g.num_prims) {
      const uint2 p = g.prims[prim];
      if (p.x == VIMG_PRIM_TRIANGLE) {
        if (p.y < g.num_tris) {
          const uint32_t* row = g.tri_vertices + 3 * size_t(p.y);
          const uint32_t i0 = row[0], i1 = row[1], i2 = row[2];
          if (i0 < g.num_vertices && i1 < g.num_vertices && i2 < g.num_vertices) {
            code = VIMG_MOTION_TRIANGLE;
            if (g.old_vertices) {
              const float *o0 = g.old_vertices + 3 * size_t(i0), *n0 = g.new_vertices + 3 * size_t(i0);
              const float *o1 = g.old_vertices + 3 * size_t(i1), *n1 = g.new_vertices + 3 * size_t(i1);
              const float *o2 = g.old_vertices + 3 * size_t(i2), *n2 = g.new_vertices + 3 * size_t(i2);
              const float b1 = hit.z, b2 = hit.w, w0 = (1.f - b1) - b2;
              dx = (w0 * (o0[0] - n0[0]) + b1 * (o1[0] - n1[0])) + b2 * (o2[0] - n2[0]);
              dy = (w0 * (o0[1] - n0[1]) + b1 * (o1[1] - n1[1])) + b2 * (o2[1] - n2[1]);
              dz = (w0 * (o0[2] - n0[2]) + b1 * (o1[2] - n1[2])) + b2 * (o2[2] - n2[2]);
            }
          }
        }
      } else if (p.x == VIMG_PRIM_SPHERE) {
        if (p.y < g.num_spheres) {
          code = VIMG_MOTION_SPHERE;
          if (g.old_spheres) {
            const float4 so = g.old_spheres[p.y], sn = g.new_spheres[p.y];
            dx = so.x - sn.x;
            dy = so.y - sn.y;
            dz = so.z - sn.z;
            if (sn.w > 0.f) {
              const float4 ro = rays[2 * q], rd = rays[2 * q + 1];      // {org, t_min}, {dir, t_max}
              const float t = hit.x, s = so.w / sn.w;
              const float ux = (ro.x + t * rd.x) - sn.x, uy = (ro.y + t * rd.y) - sn.y, uz = (ro.z + t * rd.z) - sn.z;
              dx = dx + (ux * s - ux);
              dy = dy + (uy * s - uy);
              dz = dz + (uz * s - uz);
            }
          }
        }
      }
    }
  }
  float qx = px, qy = py, qz = pz;                  // D == 0: P's bits, a select
  if (!(dx == 0.f && dy == 0.f && dz == 0.f)) {
    qx = px + dx;
    qy = py + dy;
    qz = pz + dz;
  } else if (code != VIMG_MOTION_OUT_OF_RANGE) {
    code = VIMG_MOTION_STATIC;
  }
  previous[3 * q] = qx;
  previous[3 * q + 1] = qy;
  previous[3 * q + 2] = qz;
  if (code_out) code_out[q] = uint8_t(code);
}

}  // namespace vimg_motion

using namespace vimg_motion;

extern "C" {

int vimg_motion_previous_position(const VimgMotionFrames* f, const VimgMotionGeometry* g, void* d_out_previous, void* d_out_code,
                                  void* stream) {
  static_assert(sizeof(VimgRayHit) == sizeof(float4) && sizeof(VimgRay) == 2 * sizeof(float4) && sizeof(VimgPrim) == sizeof(uint2),
                "the records the kernel reads as vectors");
  if (const int rc = check_structs(f, g, "geometry", VIMG_MOTION_MAX_EXTENT)) return rc;
  if (const int rc = check_present({{f->position, "position"}, {f->hits, "hits"}})) return rc;
  if (misaligned(f->position, 4)) return fail(VIMG_E_INVALID, "motion: the position frame must be 4-byte aligned");
  if (misaligned(f->hits, 16)) return fail(VIMG_E_INVALID, "motion: the hits must be 16-byte aligned");
  if (misaligned(f->rays, 16)) return fail(VIMG_E_INVALID, "motion: the rays must be 16-byte aligned");
  if (!f->rays && g->num_spheres > 0)
    return fail(VIMG_E_INVALID, "motion: null rays with %u spheres: a sphere hit reads its ray", g->num_spheres);
  if (g->num_prims > 0 && !g->prims) return fail(VIMG_E_INVALID, "motion: null prims table with num_prims %u", g->num_prims);
  if (g->num_tris > 0 && !g->tri_vertices)
    return fail(VIMG_E_INVALID, "motion: null tri_vertices table with num_tris %u", g->num_tris);
  if (misaligned(g->prims, 8)) return fail(VIMG_E_INVALID, "motion: the prims table must be 8-byte aligned");
  if (misaligned(g->tri_vertices, 4)) return fail(VIMG_E_INVALID, "motion: the tri_vertices table must be 4-byte aligned");
  if (!g->old_vertices != !g->new_vertices)
    return fail(VIMG_E_INVALID, "motion: old_vertices and new_vertices go together: %s is null", !g->old_vertices ? "old_vertices" : "new_vertices");
  if (!g->old_spheres != !g->new_spheres)
    return fail(VIMG_E_INVALID, "motion: old_spheres and new_spheres go together: %s is null", !g->old_spheres ? "old_spheres" : "new_spheres");
  if (misaligned(g->old_vertices, 4) || misaligned(g->new_vertices, 4))
    return fail(VIMG_E_INVALID, "motion: the vertex tables must be 4-byte aligned");
  if (misaligned(g->old_spheres, 16) || misaligned(g->new_spheres, 16))
    return fail(VIMG_E_INVALID, "motion: the sphere tables must be 16-byte aligned");
  if (!d_out_previous) return fail(VIMG_E_INVALID, "motion: null previous-position output");
  if (misaligned(d_out_previous, 4)) return fail(VIMG_E_INVALID, "motion: the previous-position output must be 4-byte aligned");
  const uint32_t w = f->width, h = f->height;
  const uint64_t n = uint64_t(w) * h;
  // what the kernel reads: a table that is NULL or empty is never read
  const Range in[9] = {{f->position, 12 * n, "position frame"},
                       {f->hits, 16 * n, "hits"},
                       {f->rays, 32 * n, "rays"},
                       {g->prims, uint64_t(8) * g->num_prims, "prims table"},
                       {g->tri_vertices, uint64_t(12) * g->num_tris, "tri_vertices table"},
                       {g->old_vertices, uint64_t(12) * g->num_vertices, "old_vertices table"},
                       {g->new_vertices, uint64_t(12) * g->num_vertices, "new_vertices table"},
                       {g->old_spheres, uint64_t(16) * g->num_spheres, "old_spheres table"},
                       {g->new_spheres, uint64_t(16) * g->num_spheres, "new_spheres table"}};
  if (const Range* r = first_overlap(d_out_previous, 12 * n, in))
    return fail(VIMG_E_INVALID, "motion: the previous-position output overlaps the %s", r->name);
  if (d_out_code) {
    if (const Range* r = first_overlap(d_out_code, n, in)) return fail(VIMG_E_INVALID, "motion: the code output overlaps the %s", r->name);
    if (overlaps(d_out_code, n, d_out_previous, 12 * n))
      return fail(VIMG_E_INVALID, "motion: the code output overlaps the previous-position output");
  }

  const Tables t{g->num_prims,
                 g->num_tris,
                 g->num_vertices,
                 g->num_spheres,
                 static_cast<const uint2*>(g->prims),
                 static_cast<const uint32_t*>(g->tri_vertices),
                 static_cast<const float*>(g->old_vertices),
                 static_cast<const float*>(g->new_vertices),
                 static_cast<const float4*>(g->old_spheres),
                 static_cast<const float4*>(g->new_spheres)};
  clear_stale_error();
  motion_previous_kernel<<<pixel_grid(w, h), pixel_block(), 0, static_cast<hipStream_t>(stream)>>>(
      w, h, static_cast<const float*>(f->position), static_cast<const float4*>(f->hits), static_cast<const float4*>(f->rays), t,
      static_cast<float*>(d_out_previous), static_cast<uint8_t*>(d_out_code));
  return launched();
}

const char* vimg_motion_last_error(void) { return g_error; }

}  // extern "C"
