// New materials, texture contents, emitters and background for a resident scene: the fields of a
// VimgGeometryUpdate behind `spheres` (vimg_hip_scene_update_geometry).  The upload bakes little
// from these tables, and all of it is derived again here from what is resident, with the upload's own statements
// (scene_bake.h), so that a launch afterwards reads the bytes of a fresh upload of the equally edited host scene:
//
//   scene_relight_flags    one thread per material: material_flags
//   scene_relight_cls      one thread per leaf slot: the material class of its primitive (a later rebuild of the
//                          tree carries the classes over from the slots, scene_rebuild.hip)
//   scene_bake_materials   one thread per material: its DMaterial (material_terms.h), at upload and after every edit
//                          of materials or texture records, into a buffer beside the live one
//   scene_relight_lights   one thread per emitter: the whole DLight - kind, index, the triangle's or sphere's
//                          fields, the material's emission - from the emitter list it is given
//   (precompute.hip)       an image's mip chain in place, level by level, and the env map's sampling CDFs
//
// The materials and texture records are small tables copied from the host; texels only ever move device to device.
// The host keeps what it decides by: the TEX / non-TEX kernel family, background_emissive, the copies of the
// tables the next update is checked against.
#include <hip/hip_runtime.h>

#include <cstring>

#include "device_math.h"
#include "hip_internal.h"
#include "material_terms.h"
#include "scene_bake.h"

namespace vimg {

namespace {

constexpr uint32_t kBlock = 256;

template <typename T>
VD T* flat(gptr<T> p) {
  return (T*)p;
}

dim3 blocks_for(uint32_t n) { return dim3((n + kBlock - 1) / kBlock); }

}  // namespace

__global__ void __launch_bounds__(kBlock) scene_relight_flags(const DScene d, uint32_t num_materials) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_materials) return;
  flat(d.material_flags)[i] = bake_material_flags(flat(d.materials)[i], flat(d.textures));
}

__global__ void __launch_bounds__(kBlock) scene_relight_cls(const DScene d, uint32_t num_slots) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= num_slots) return;
  DLeafPrim* lp = flat(d.leaf_prims) + j;
  const VimgPrim p = flat(d.prims)[lp->prim];
  lp->cls = bake_material_class(flat(d.materials)[bake_prim_material(p, flat(d.tri_shade), flat(d.meshes), flat(d.spheres))].type);
}

__global__ void __launch_bounds__(kBlock)
scene_relight_lights(const DScene d, const VimgLight* __restrict__ lights, uint32_t num_lights, DLight* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_lights) return;
  out[i] = bake_light(lights[i], flat(d.prims), flat(d.tri_shade), flat(d.tri_area_pdf), flat(d.meshes), flat(d.spheres), flat(d.materials));
}

// Baked on the device, never on the host: F_log is OCML's log here and in the stages, glibc's there.
__global__ void __launch_bounds__(kBlock) scene_bake_materials(const DScene d, uint32_t num_materials, DMaterial* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_materials) return;
  const VimgMaterial m = flat(d.materials)[i];
  const uint32_t bits = dmaterial_bits(m, flat(d.textures));
  f3 base{0.f, 0.f, 0.f};
  if (bits & DMAT_COLOUR) {
    const VimgTexture* t = flat(d.textures) + m.tex;
    base = f3{t->col_a[0], t->col_a[1], t->col_a[2]};
  }
  out[i] = bake_dmaterial(m, bits, base);
}

int enqueue_material_bake(const DScene& d, uint32_t num_materials, DMaterial* out, hipStream_t st) {
  if (!num_materials) return VIMG_OK;
  hipLaunchKernelGGL(scene_bake_materials, blocks_for(num_materials), dim3(kBlock), 0, st, d, num_materials, out);
  HIP_TRY(hipGetLastError());
  return VIMG_OK;
}

namespace {

bool is_env_image(const VimgBackground& bg, uint32_t texture) {
  return bg.type == VIMG_BG_ENVMAP && bg.env_tex >= 0 && static_cast<uint32_t>(bg.env_tex) == texture;
}

// the mip kernels read level l - 1 while they write level l: in place only when no two levels share texels
bool levels_disjoint(const VimgTexture& t) {
  for (uint32_t a = 0; a < t.num_levels; ++a)
    for (uint32_t b = a + 1; b < t.num_levels; ++b) {
      const uint64_t na = uint64_t(std::max(t.width >> a, 1u)) * std::max(t.height >> a, 1u);
      const uint64_t nb = uint64_t(std::max(t.width >> b, 1u)) * std::max(t.height >> b, 1u);
      if (t.level_offset[a] < t.level_offset[b] + nb && t.level_offset[b] < t.level_offset[a] + na) return false;
    }
  return true;
}

}  // namespace

int check_relight(const VimgDeviceScene* s, const VimgGeometryUpdate* u) {
  const uint32_t num_textures = static_cast<uint32_t>(s->textures.size());
  if (u->textures)
    for (uint32_t i = 0; i < num_textures; ++i) {
      const VimgTexture &a = s->textures[i], &b = u->textures[i];
      if (a.type != b.type) return fail(VIMG_E_INVALID, "update: a texture record must keep its type");
      if (a.type != VIMG_TEX_IMAGE) continue;
      if (a.width != b.width || a.height != b.height || a.num_levels != b.num_levels || a.wrap_u != b.wrap_u || a.wrap_v != b.wrap_v ||
          std::memcmp(a.level_offset, b.level_offset, sizeof(uint64_t) * a.num_levels) != 0)
        return fail(VIMG_E_INVALID, "update: an image texture must keep its size, levels, offsets and wrap modes");
    }
  const VimgTexture* textures = u->textures ? u->textures : s->textures.data();
  if (u->materials)
    if (int rc = validate_materials(u->materials, static_cast<uint32_t>(s->materials.size()), textures, num_textures, s->num_rg_textures))
      return rc;
  if (u->background) {
    const VimgBackground &a = s->d.background, &b = *u->background;
    if (a.type != b.type || a.env_tex != b.env_tex || a.row_cdf_offset != b.row_cdf_offset || a.col_cdf_offset != b.col_cdf_offset)
      return fail(VIMG_E_INVALID, "update: the background must keep its type, env_tex and cdf offsets");
  }
  if (u->set_lights) {
    if (u->num_lights && !u->lights) return fail(VIMG_E_INVALID, "update: num_lights without lights");
    if (int rc = validate_lights(u->lights, u->num_lights, s->num_leaf_prims)) return rc;
    uint32_t backgrounds = 0;
    for (uint32_t i = 0; i < u->num_lights; ++i) backgrounds += u->lights[i].type == VIMG_LIGHT_BACKGROUND;
    if (backgrounds > 1) return fail(VIMG_E_INVALID, "update: more than one background entry in lights");
  }
  if (u->num_images && !u->images) return fail(VIMG_E_INVALID, "update: num_images without images");
  for (uint32_t k = 0; k < u->num_images; ++k) {
    const VimgTextureImage& im = u->images[k];
    if (im.texture >= num_textures || s->textures[im.texture].type != VIMG_TEX_IMAGE)
      return fail(VIMG_E_INVALID, "update: images: texture is not a resident image texture");
    if (!im.level0 || (reinterpret_cast<uintptr_t>(im.level0) & 3u))
      return fail(VIMG_E_INVALID, "update: images: level0 is null or not 4-byte aligned");
    if (!levels_disjoint(s->textures[im.texture]))
      return fail(VIMG_E_UNSUPPORTED, "update: images: the texture's mip levels overlap in the texel pool");
  }
  return VIMG_OK;
}

int prepare_relight(const VimgDeviceScene* s, const VimgGeometryUpdate* u, RelightPlan* plan) {
  plan->any = u->materials || u->textures || u->set_lights || u->background || u->num_images;
  if (!plan->any) return VIMG_OK;
  if (g_device < 0) return fail(VIMG_E_DEVICE, "update: no device");
  if (u->set_lights) {   // beside the scene's, swapped in when everything has succeeded; an empty list gets one element's worth, as at upload
    if (int rc = plan->new_lights.alloc(std::max<size_t>(u->num_lights, 1) * sizeof(VimgLight))) return rc;
    if (int rc = plan->new_dlights.alloc(std::max<size_t>(u->num_lights, 1) * sizeof(DLight))) return rc;
  }
  if ((u->materials || u->textures) && !s->materials.empty())
    if (int rc = plan->new_dmaterials.alloc(s->materials.size() * sizeof(DMaterial))) return rc;
  for (uint32_t k = 0; k < u->num_images; ++k)
    if (is_env_image(s->d.background, u->images[k].texture) && !plan->lum.p) {
      const VimgTexture& t = s->textures[u->images[k].texture];
      plan->sin_table = env_sin_table(t.height);
      if (int rc = plan->sin_elev.alloc(size_t(t.height) * sizeof(float))) return rc;
      if (int rc = plan->lum.alloc(size_t(t.width) * t.height * sizeof(float))) return rc;
      if (int rc = plan->row_int.alloc(size_t(t.height) * sizeof(float))) return rc;
      if (int rc = plan->row_tot.alloc(sizeof(float))) return rc;
    }
  return VIMG_OK;
}

int enqueue_relight(VimgDeviceScene* s, const VimgGeometryUpdate* u, RelightPlan* plan, hipStream_t st) {
  const DScene& d = s->d;
  // 1. images: level 0 from the caller's device buffer, then the chain and (env map) the CDFs where they are
  float* texels = (float*)d.texels;
  float* cdf_pool = (float*)d.cdf_pool;
  for (uint32_t k = 0; k < u->num_images; ++k) {
    const VimgTextureImage& im = u->images[k];
    const VimgTexture& t = s->textures[im.texture];
    float* level0 = texels + t.level_offset[0] * 3;
    HIP_TRY(hipMemcpyAsync(level0, im.level0, size_t(t.width) * t.height * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
    enqueue_mip_levels(texels, t.level_offset, t.num_levels, t.width, t.height, t.wrap_u, t.wrap_v, st);
    if (is_env_image(d.background, im.texture)) {
      HIP_TRY(hipMemcpyAsync(plan->sin_elev.p, plan->sin_table.data(), plan->sin_table.size() * sizeof(float), hipMemcpyHostToDevice, st));
      enqueue_env_cdfs(level0, t.width, t.height,
                       EnvCdfScratch{plan->sin_elev.as<float>(), plan->lum.as<float>(), plan->row_int.as<float>(), plan->row_tot.as<float>()},
                       cdf_pool + d.background.row_cdf_offset, cdf_pool + d.background.col_cdf_offset, st);
    }
  }
  // 2. tables, and what the upload derives from them
  if (u->textures && !s->textures.empty())
    HIP_TRY(hipMemcpyAsync((void*)d.textures, u->textures, s->textures.size() * sizeof(VimgTexture), hipMemcpyHostToDevice, st));
  if (u->materials && !s->materials.empty()) {
    const uint32_t n = static_cast<uint32_t>(s->materials.size());
    HIP_TRY(hipMemcpyAsync((void*)d.materials, u->materials, size_t(n) * sizeof(VimgMaterial), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(scene_relight_flags, blocks_for(n), dim3(kBlock), 0, st, d, n);
    hipLaunchKernelGGL(scene_relight_cls, blocks_for(s->num_leaf_prims), dim3(kBlock), 0, st, d, s->num_leaf_prims);
  }
  if (plan->new_dmaterials.p)   // (after both copies: a record reads its material and its colour texture)
    if (int rc = enqueue_material_bake(d, static_cast<uint32_t>(s->materials.size()), plan->new_dmaterials.as<DMaterial>(), st)) return rc;
  // 3. emitters: the new list into its new buffers, or the resident list again with the new materials' emission
  if (u->set_lights) {
    if (u->num_lights) {
      HIP_TRY(hipMemcpyAsync(plan->new_lights.p, u->lights, size_t(u->num_lights) * sizeof(VimgLight), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(scene_relight_lights, blocks_for(u->num_lights), dim3(kBlock), 0, st, d, plan->new_lights.as<const VimgLight>(),
                         u->num_lights, plan->new_dlights.as<DLight>());
    }
  } else if (u->materials && d.num_lights) {
    hipLaunchKernelGGL(scene_relight_lights, blocks_for(d.num_lights), dim3(kBlock), 0, st, d, (const VimgLight*)d.lights, d.num_lights,
                       (DLight*)d.dlights);
  }
  HIP_TRY(hipGetLastError());
  return VIMG_OK;
}

void commit_relight(VimgDeviceScene* s, const VimgGeometryUpdate* u, RelightPlan* plan) {
  DScene& d = s->d;
  if (u->textures) s->textures.assign(u->textures, u->textures + s->textures.size());
  if (u->materials) {
    s->materials.assign(u->materials, u->materials + s->materials.size());
    s->has_other = table_holds_other(s->materials.data(), s->materials.size());   // (a type may have changed: PF_NO_OTHER)
  }
  if (u->background) {
    d.background = *u->background;
    d.background_emissive = background_is_emissive(d.background);
  }
  if (plan->new_dmaterials.p) {   // (the same size: the scene's bytes stay)
    DevBuf& dmaterials = s->tables[s->dmaterials_table];
    dmaterials = std::move(plan->new_dmaterials);
    d.dmaterials = (decltype(d.dmaterials))dmaterials.p;
  }
  s->textured = tables_textured(s->materials.data(), static_cast<uint32_t>(s->materials.size()), s->textures.data(), d.background);
  if (u->set_lights) {
    DevBuf& lights = s->tables[s->lights_table];
    DevBuf& dlights = s->tables[s->dlights_table];
    s->total_bytes = s->total_bytes - lights.bytes - dlights.bytes + plan->new_lights.bytes + plan->new_dlights.bytes;
    lights = std::move(plan->new_lights);      // (a move frees what the scene held)
    dlights = std::move(plan->new_dlights);
    d.lights = (decltype(d.lights))lights.p;
    d.dlights = (decltype(d.dlights))dlights.p;
    d.num_lights = u->num_lights;
    s->lights.assign(u->lights, u->lights + u->num_lights);
    s->waves_per_simd = (s->total_bytes > (32u << 20)) ? 3 : 2;   // (the policy of the upload, on the bytes an upload would count)
  }
}

}  // namespace vimg
