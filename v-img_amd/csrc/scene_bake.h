// The records the upload bakes from positions, stated once: vimg_hip_scene_upload_opts (host) and the
// scene_update_* kernels (device) both call these, so a geometry update gives bit for bit what a fresh
// upload gives.  Plain float expressions, evaluated with IEEE +, -, *, / and no contraction on both
// sides (-ffp-contract=off).  Square root is spelled __builtin_sqrtf everywhere: sqrtss on the host,
// the correctly rounded v_sqrt_f32 expansion on gfx950 (hipcc's default for float sqrt).
#pragma once
#include "device_scene.h"

namespace vimg {

#define VHD static __host__ __device__ __forceinline__

// cross(p2 - p0, p1 - p0) of the triangle v = p0 p1 p2 (nine floats)
VHD void tri_cross21(const float* v, float c21[3]) {
  const float e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]};
  const float e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
  c21[0] = e2[1] * e1[2] - e1[1] * e2[2];
  c21[1] = e2[2] * e1[0] - e1[2] * e2[0];
  c21[2] = e2[0] * e1[1] - e1[0] * e2[1];
}

// tri_normal and the area pdf with the reference's float expressions
// (src/geometry/triangle.cpp:19-25,229-231; glm cross / normalize as in device_math.h)
VHD void bake_tri_normal_pdf(const float* v, float n[3], float* area_pdf) {
  const float e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]};
  const float e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
  const float c12[3] = {e1[1] * e2[2] - e2[1] * e1[2], e1[2] * e2[0] - e2[2] * e1[0],
                        e1[0] * e2[1] - e2[0] * e1[1]};
  const float inv_len = 1.0f / __builtin_sqrtf(c12[0] * c12[0] + c12[1] * c12[1] + c12[2] * c12[2]);
  for (int a = 0; a < 3; ++a) n[a] = c12[a] * inv_len;
  float c21[3];
  tri_cross21(v, c21);
  const float area = __builtin_sqrtf(c21[0] * c21[0] + c21[1] * c21[1] + c21[2] * c21[2]) / 2.0f;
  *area_pdf = 1.f / area;
}

// DLeafPrim of a triangle: positions and kind.  The degenerate-triangle reject of the reference
// (triangle.h:86-92) depends on the vertices only: evaluated once, with the same float expression
VHD void bake_leaf_tri(const float* v, DLeafPrim& lp) {
  lp.a = v4f{v[0], v[1], v[2], v[3]};
  lp.b = v4f{v[4], v[5], v[6], v[7]};
  lp.c0 = v[8];
  float c[3];
  tri_cross21(v, c);
  const float l2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  lp.kind = (l2 == 0.f) ? 2u : 0u;
}
// ... of a sphere: centre and radius (its kind, 1, never changes)
VHD void bake_leaf_sphere(const VimgSphere& sp, DLeafPrim& lp) {
  lp.a = v4f{sp.center[0], sp.center[1], sp.center[2], sp.radius};
}

// the geometric fields of a DLight: a triangle's positions, face normal and area pdf, a sphere's centre and radius
VHD void bake_light_tri(const DTriShade& ts, float area_pdf, DLight& L) {
  L.a = v4f{ts.p[0], ts.p[1], ts.p[2], ts.p[3]};
  L.b = v4f{ts.p[4], ts.p[5], ts.p[6], ts.p[7]};
  L.c = v4f{ts.p[8], ts.n[0], ts.n[1], ts.n[2]};
  L.d.w = area_pdf;
}
VHD void bake_light_sphere(const VimgSphere& sp, DLight& L) {
  L.a = v4f{sp.center[0], sp.center[1], sp.center[2], sp.radius};
}

// ---- what the upload derives from the material table: stated once for the upload (host) and for the
// material update's kernels (scene_relight.hip)
// the vertex queue a hit is routed into (DLeafPrim::cls)
VHD uint32_t bake_material_class(uint32_t type) {
  return type == VIMG_MAT_DIFFUSE_LIGHT ? 0u : type == VIMG_MAT_LAMBERTIAN ? 1u : type == VIMG_MAT_PRINCIPLED ? 2u : 3u;
}
// whether the table holds a material of class 3, "other" (plain_build.h: PF_NO_OTHER asks)
inline bool table_holds_other(const VimgMaterial* materials, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (bake_material_class(materials[i].type) == 3u) return true;
  return false;
}
VHD uint32_t bake_material_flags(const VimgMaterial& m, const VimgTexture* textures) {
  uint32_t f = 0;
  if (m.type == VIMG_MAT_PRINCIPLED) f |= MATF_NEEDS_FRAME;
  if (m.tex >= 0 && textures[m.tex].type != VIMG_TEX_CONST) f |= MATF_NEEDS_UV;
  if (m.mr_tex >= 0 || m.normal_map >= 0) f |= MATF_NEEDS_UV;
  return f;
}
// the material of a primitive (shade: the per-triangle records, which carry the triangle's mesh)
VHD uint32_t bake_prim_material(const VimgPrim& p, const DTriShade* shade, const VimgMesh* meshes, const VimgSphere* spheres) {
  return p.type == VIMG_PRIM_TRIANGLE ? meshes[shade[p.index].mesh].material : spheres[p.index].material;
}
// one whole DLight: kind, index, the geometric fields and the material's emission (zero when it is no DiffuseLight:
// Material::emitted of the others)
VHD DLight bake_light(const VimgLight& l, const VimgPrim* prims, const DTriShade* shade, const float* area_pdf, const VimgMesh* meshes,
                      const VimgSphere* spheres, const VimgMaterial* materials) {
  DLight L{};
  if (l.type == VIMG_LIGHT_BACKGROUND) {
    L.kind = 0u;
    return L;
  }
  const VimgPrim p = prims[l.prim];
  L.index = p.index;
  uint32_t mat;
  if (p.type == VIMG_PRIM_TRIANGLE) {
    const VimgMesh& mesh = meshes[shade[p.index].mesh];
    L.kind = mesh.has_normals ? 2u : 1u;
    bake_light_tri(shade[p.index], area_pdf[p.index], L);
    mat = mesh.material;
  } else {
    const VimgSphere& sp = spheres[p.index];
    L.kind = 3u;
    bake_light_sphere(sp, L);
    mat = sp.material;
  }
  const VimgMaterial& m = materials[mat];
  if (m.type == VIMG_MAT_DIFFUSE_LIGHT) L.d.x = m.emit[0], L.d.y = m.emit[1], L.d.z = m.emit[2];
  return L;
}

// the boxes of a DNode's two children: a = Lmin Lmax.x, b = Lmax.yz Rmin.xy, c = Rmin.z Rmax
VHD void pack_boxes(DNode& n, const float* lmin, const float* lmax, const float* rmin, const float* rmax) {
  n.a = v4f{lmin[0], lmin[1], lmin[2], lmax[0]};
  n.b = v4f{lmax[1], lmax[2], rmin[0], rmin[1]};
  n.c = v4f{rmin[2], rmax[0], rmax[1], rmax[2]};
}

#undef VHD

}  // namespace vimg
