// The primitive bounds of prim_bounds (host/bvh_build.cpp) and the builders' union, stated once for the
// device: the refit of scene_update.hip folds them per leaf slot, scene_rebuild.hip writes them per primitive
// for the GPU builders.  Minima and maxima are the host's selects (b < a ? b : a, a < b ? b : a;
// host/hmath.hpp), never v_min / v_max: the Morton keys, and with them a whole tree, depend on these bits.
#pragma once
#include "device_math.h"

namespace vimg {

struct Box3 {
  f3 lo, hi;
};

VD Box3 grow(Box3 a, Box3 b) {
  return Box3{mk3(sel_min(a.lo.x, b.lo.x), sel_min(a.lo.y, b.lo.y), sel_min(a.lo.z, b.lo.z)),
              mk3(sel_max(a.hi.x, b.hi.x), sel_max(a.hi.y, b.hi.y), sel_max(a.hi.z, b.hi.z))};
}

// Triangle::bounds: vmin(v0, vmin(v1, v2)), vmax(v0, vmax(v1, v2))
VD Box3 tri_box(f3 v0, f3 v1, f3 v2) {
  const Box3 b12{mk3(sel_min(v1.x, v2.x), sel_min(v1.y, v2.y), sel_min(v1.z, v2.z)),
                 mk3(sel_max(v1.x, v2.x), sel_max(v1.y, v2.y), sel_max(v1.z, v2.z))};
  return Box3{mk3(sel_min(v0.x, b12.lo.x), sel_min(v0.y, b12.lo.y), sel_min(v0.z, b12.lo.z)),
              mk3(sel_max(v0.x, b12.hi.x), sel_max(v0.y, b12.hi.y), sel_max(v0.z, b12.hi.z))};
}

// Sphere::bounds: centre - r, centre + r
VD Box3 sphere_box(f3 c, float r) {
  return Box3{mk3(c.x - r, c.y - r, c.z - r), mk3(c.x + r, c.y + r, c.z + r)};
}

}  // namespace vimg
