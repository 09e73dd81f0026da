// A scene's way onto the device: shape checks, the baking of the caller's tables into the device layout
// (once per scene; scene_bake.h states the baked expressions), the upload, and the changes of a resident
// scene (vimg_hip_scene_update_geometry, vimg_hip_scene_set_camera).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numbers>

#include "hip_internal.h"
#include "scene_bake.h"
#include "scene_update.h"

using namespace vimg;

namespace {

// a table of the scene into `b`, counted in the scene's bytes (an empty table still gets one element's worth)
template <typename T>
int upload(VimgDeviceScene* s, DevBuf& b, const T* host, size_t count) {
  if (int rc = b.alloc(std::max<size_t>(count, 1) * sizeof(T))) return rc;
  s->total_bytes += b.bytes;
  if (count) HIP_TRY(hipMemcpy(b.p, host, count * sizeof(T), hipMemcpyHostToDevice));
  return VIMG_OK;
}

}  // namespace

// the material and the emitter table: checked at upload, and again when an update replaces them
int vimg::validate_materials(const VimgMaterial* materials, uint32_t num_materials, const VimgTexture* textures, uint32_t num_textures,
                             uint32_t num_rg_textures) {
  for (uint32_t i = 0; i < num_materials; ++i) {
    const VimgMaterial& m = materials[i];
    if (m.type > VIMG_MAT_PRINCIPLED) return fail(VIMG_E_INVALID, "material: unknown type");
    auto tex_ok = [&](int32_t t) { return t >= -1 && t < int32_t(num_textures); };
    if (!tex_ok(m.tex) || !tex_ok(m.normal_map) || m.mr_tex < -1 || m.mr_tex >= int32_t(num_rg_textures))
      return fail(VIMG_E_INVALID, "material: texture index out of range");
    if ((m.type == VIMG_MAT_LAMBERTIAN || m.type == VIMG_MAT_PRINCIPLED) && m.tex < 0)
      return fail(VIMG_E_INVALID, "material: missing colour texture");
    if (m.normal_map >= 0 && textures[m.normal_map].type != VIMG_TEX_IMAGE)
      return fail(VIMG_E_INVALID, "material: normal map must be an image");
  }
  return VIMG_OK;
}

int vimg::validate_lights(const VimgLight* lights, uint32_t num_lights, uint32_t num_prims) {
  for (uint32_t i = 0; i < num_lights; ++i) {
    const VimgLight& l = lights[i];
    if (l.type == VIMG_LIGHT_PRIM) {
      if (l.prim >= num_prims) return fail(VIMG_E_INVALID, "light: prim out of range");
    } else if (l.type != VIMG_LIGHT_BACKGROUND) {
      return fail(VIMG_E_INVALID, "light: unknown type");
    }
  }
  return VIMG_OK;
}

// whether the tables need the TEX kernels (cones, image textures, env map)
bool vimg::tables_textured(const VimgMaterial* materials, uint32_t num_materials, const VimgTexture* textures, const VimgBackground& bg) {
  bool textured = (bg.type == VIMG_BG_ENVMAP);
  for (uint32_t i = 0; i < num_materials; ++i) {
    const VimgMaterial& m = materials[i];
    if (m.tex >= 0 && textures[m.tex].type == VIMG_TEX_IMAGE) textured = true;
    if (m.mr_tex >= 0 || m.normal_map >= 0) textured = true;
  }
  return textured;
}

// Background::is_emissive (reference include/background.h:51-56,176)
bool vimg::background_is_emissive(const VimgBackground& bg) {
  return (bg.type == VIMG_BG_ENVMAP) || !(bg.col[0] == 0.f && bg.col[1] == 0.f && bg.col[2] == 0.f);
}

namespace {

// Shape checks so that no kernel ever indexes outside its tables.
int validate(const VimgScene* sc) {
  if (!sc) return fail(VIMG_E_INVALID, "scene is null");
  if (sc->camera.res_x <= 0 || sc->camera.res_y <= 0) return fail(VIMG_E_INVALID, "bad resolution");
  if (sc->num_prims == 0 || !sc->prims) return fail(VIMG_E_INVALID, "scene has no primitives");
  const VimgBVH& b = sc->bvh;
  if (b.num_nodes == 0 || !b.nodes || !b.bb_mins_maxes || !b.obj_indices)
    return fail(VIMG_E_INVALID, "scene has no BVH");
  if (b.max_depth + 2 > 96) return fail(VIMG_E_INVALID, "BVH deeper than the 94-level stack bound");
  for (uint32_t i = 0; i < sc->num_prims; ++i) {
    const VimgPrim& p = sc->prims[i];
    if (p.type == VIMG_PRIM_TRIANGLE) {
      if (p.index >= sc->num_tris) return fail(VIMG_E_INVALID, "prim: triangle index out of range");
    } else if (p.type == VIMG_PRIM_SPHERE) {
      if (p.index >= sc->num_spheres) return fail(VIMG_E_INVALID, "prim: sphere index out of range");
    } else {
      return fail(VIMG_E_INVALID, "prim: unknown type");
    }
  }
  for (uint32_t t = 0; t < sc->num_tris; ++t) {
    if (sc->tri_mesh[t] >= sc->num_meshes) return fail(VIMG_E_INVALID, "tri: mesh out of range");
    const VimgMesh& m = sc->meshes[sc->tri_mesh[t]];
    for (int k = 0; k < 3; ++k)
      if (sc->tri_indices[t * 3 + k] >= m.num_vertices)
        return fail(VIMG_E_INVALID, "tri: vertex index out of range");
  }
  for (uint32_t i = 0; i < sc->num_meshes; ++i) {
    const VimgMesh& m = sc->meshes[i];
    if (uint64_t(m.first_vertex) + m.num_vertices > sc->num_vertices)
      return fail(VIMG_E_INVALID, "mesh: vertex range out of bounds");
    if (m.material >= sc->num_materials) return fail(VIMG_E_INVALID, "mesh: material out of range");
    if (m.num_uv_sets > VIMG_MAX_UV_SETS) return fail(VIMG_E_INVALID, "mesh: too many uv sets");
    for (uint32_t k = 0; k < m.num_uv_sets; ++k)
      if (uint64_t(m.uv_offset[k]) + m.num_vertices > sc->num_uvs)
        return fail(VIMG_E_INVALID, "mesh: uv set out of bounds");
    auto ok = [&](uint32_t u) { return u == VIMG_NO_UV || u < m.num_uv_sets; };
    if (!ok(m.color_tex_uv) || !ok(m.normal_tex_uv) || !ok(m.metallic_roughness_tex_uv))
      return fail(VIMG_E_INVALID, "mesh: uv selector out of range");
  }
  for (uint32_t i = 0; i < sc->num_spheres; ++i)
    if (sc->spheres[i].material >= sc->num_materials)
      return fail(VIMG_E_INVALID, "sphere: material out of range");
  for (uint32_t i = 0; i < sc->num_textures; ++i) {
    const VimgTexture& t = sc->textures[i];
    if (t.type > VIMG_TEX_IMAGE) return fail(VIMG_E_INVALID, "texture: unknown type");
    if (t.type == VIMG_TEX_IMAGE) {
      if (t.num_levels == 0 || t.num_levels > VIMG_MAX_MIP_LEVELS || t.width == 0 || t.height == 0)
        return fail(VIMG_E_INVALID, "texture: bad mip chain");
      for (uint32_t l = 0; l < t.num_levels; ++l) {
        uint64_t w = std::max(t.width >> l, 1u), h = std::max(t.height >> l, 1u);
        if (t.level_offset[l] + w * h > sc->num_texels)
          return fail(VIMG_E_INVALID, "texture: level out of bounds");
      }
    }
  }
  for (uint32_t i = 0; i < sc->num_rg_textures; ++i) {
    const VimgTextureRG& t = sc->rg_textures[i];
    if (t.width == 0 || t.height == 0 || t.wrap_u > 2 || t.wrap_v > 2)
      return fail(VIMG_E_INVALID, "rg texture: bad size or wrap mode");
    // The reference indexes the +x neighbours with "* height" instead of "* width" (quirk Q6,
    // include/texture/texture_RG.h:47,52).  For width >= height the largest such index,
    // (w-1) + (h-1) h, stays inside the w x h array: the WRONG texel is read, reproducibly, and the
    // kernels and the oracle reproduce it.  For height > width the reference reads beyond its
    // vector (undefined there): refused.
    if (t.height > t.width)
      return fail(VIMG_E_UNSUPPORTED,
                  "metallic-roughness map taller than wide: the reference reads outside the image there");
    if (t.offset + uint64_t(t.width) * t.height > sc->num_rg_texels)
      return fail(VIMG_E_INVALID, "rg texture out of bounds");
  }
  if (int rc = validate_materials(sc->materials, sc->num_materials, sc->textures, sc->num_textures, sc->num_rg_textures)) return rc;
  if (int rc = validate_lights(sc->lights, sc->num_lights, sc->num_prims)) return rc;
  if (sc->background.type == VIMG_BG_ENVMAP) {
    const int32_t t = sc->background.env_tex;
    if (t < 0 || t >= int32_t(sc->num_textures) || sc->textures[t].type != VIMG_TEX_IMAGE)
      return fail(VIMG_E_INVALID, "background: env_tex must be an image texture");
    const VimgTexture& img = sc->textures[t];
    if (sc->background.row_cdf_offset + img.height + 1 > sc->num_cdf ||
        sc->background.col_cdf_offset + uint64_t(img.height) * (img.width + 1) > sc->num_cdf)
      return fail(VIMG_E_INVALID, "background: cdf out of bounds");
  } else if (sc->background.type != VIMG_BG_CONST) {
    return fail(VIMG_E_INVALID, "background: unknown type");
  }
  // BVH: every node reachable from the root exactly once, children and leaf ranges in bounds
  std::vector<uint8_t> seen(b.num_nodes, 0);
  std::vector<uint32_t> todo{0};
  seen[0] = 1;
  while (!todo.empty()) {
    uint32_t n = todo.back();
    todo.pop_back();
    const VimgBVHNode& node = b.nodes[n];
    if (node.obj_count != 0) {
      if (uint64_t(node.first_index) + node.obj_count > sc->num_prims)
        return fail(VIMG_E_INVALID, "bvh: leaf range out of bounds");
      for (uint32_t i = 0; i < node.obj_count; ++i)
        if (b.obj_indices[node.first_index + i] >= sc->num_prims)
          return fail(VIMG_E_INVALID, "bvh: obj index out of range");
    } else {
      if (uint64_t(node.first_index) + 1 >= b.num_nodes || node.first_index == 0)
        return fail(VIMG_E_INVALID, "bvh: child index out of range");
      for (uint32_t c = node.first_index; c <= node.first_index + 1; ++c) {
        if (seen[c]) return fail(VIMG_E_INVALID, "bvh: node reachable twice (not a tree)");
        seen[c] = 1;
        todo.push_back(c);
      }
    }
  }
  return VIMG_OK;
}

// tools/ only: VIMG_HIP_* environment variables override single option fields at upload (sweeps
// and profiles without a rebuild of the caller); tests and the product pass VimgHipOptions
void options_from_env(VimgHipOptions* o) {
  if (const char* e = getenv("VIMG_HIP_SCHED")) {
    const std::string v(e);
    o->scheduler = v == "lane" ? VIMG_SCHED_LANE : v == "pool" ? VIMG_SCHED_POOL : v == "stage" ? VIMG_SCHED_STAGE
                 : v == "pool4" ? VIMG_SCHED_POOL4 : v == "pool4g" ? VIMG_SCHED_POOL4G : v == "cu" ? VIMG_SCHED_CU : atoi(e);
  }
  struct { const char* name; int32_t* field; } vars[] = {
      {"VIMG_HIP_WAVES_PER_SIMD", &o->waves_per_simd}, {"VIMG_HIP_LDS_BUDGET_KB", &o->lds_budget_kb},
      {"VIMG_HIP_POOL_SLOTS", &o->pool_slots},         {"VIMG_HIP_POOL_SEGMENTS", &o->pool_segments},
      {"VIMG_HIP_POOL_REFILL", &o->pool_refill},       {"VIMG_HIP_POOL_VBATCH", &o->pool_vbatch},
      {"VIMG_HIP_POOL_CLASSES", &o->pool_classes},     {"VIMG_HIP_POOL_STARVE", &o->pool_starve},
      {"VIMG_HIP_POOL_BOXMIN", &o->pool_boxmin},       {"VIMG_HIP_LDS_LEAF", &o->lds_leaf},
      {"VIMG_HIP_LDS_STACK", &o->lds_stack},           {"VIMG_HIP_CU_WAVES", &o->cu_waves},
      {"VIMG_HIP_CU_WALKERS", &o->cu_walkers},         {"VIMG_HIP_CU_FLEX", &o->cu_flex},
      {"VIMG_HIP_CU_LOWWATER", &o->cu_lowwater},       {"VIMG_HIP_CU_PATIENCE", &o->cu_patience},
      {"VIMG_HIP_CU_JOIN", &o->cu_join},               {"VIMG_HIP_CU_SLEEP", &o->cu_sleep}};
  for (auto& v : vars)
    if (const char* e = getenv(v.name)) *v.field = atoi(e);
}

// ---- camera: TLCam ctor (reference src/tl_camera.cpp:6-23) and the primary ray cone
// (include/ray.h:44-48) are per-render constants, evaluated here with the expressions the
// reference uses (tan is an unqualified call there: double).  The upload and
// vimg_hip_scene_set_camera both bake through this.
void bake_camera(const VimgCamera& cam, DScene& d) {
  std::memcpy(d.cam_to_world, cam.cam_to_world, sizeof(d.cam_to_world));
  {
    float theta = (cam.vfov_deg * std::numbers::pi) / 180.0;
    float ratio = static_cast<float>(cam.res_x) / cam.res_y;
    float img_height = 2.0f * (::tan(static_cast<double>(theta / 2.0f)));
    d.p_size0 = ratio * img_height;
    d.p_size1 = img_height;
    float vfov = (cam.vfov_deg * std::numbers::pi) / 180.f;
    // std::atan / std::tan of floats, evaluated in double and rounded once (DESIGN.md Numerics)
    float t = static_cast<float>(::tan(static_cast<double>(vfov / 2.f)));
    d.cone_spread = static_cast<float>(
        ::atan(static_cast<double>(2.f * t / static_cast<float>(static_cast<uint32_t>(cam.res_y)))));
  }
  d.aperture_radius = cam.aperture_radius;
  d.focal_dist = cam.focal_dist;
  d.res_x = cam.res_x;
  d.res_y = cam.res_y;
}

// ---- BVH: only internal nodes get a record; they are renumbered breadth-first (root = 0) so
// that the lowest indices are the top of the tree - the part staged into LDS.  Traversal order
// depends on the tree, not on the numbering, so results are unchanged.
struct Tree {
  std::vector<DNode> nodes;             // the internal nodes, breadth-first; renumber_bvh appends the chain records
  std::vector<DNode> chain;             // chain records of the leaves over 127 primitives
  std::vector<uint32_t> chain_leaf;     // per chain record: first slot and count of its whole leaf (for a refit)
  std::vector<uint32_t> level_begin;    // breadth-first levels: [level_begin[k], level_begin[k+1])
  uint32_t n_internal = 0, chain_depth = 0, root_ref = 0;
};

// A child reference packs "count << 25 | first leaf slot": 7 bits of count.  A leaf of more than
// 127 primitives (no builder of this repository makes one - theirs stop at 8 - but a caller's
// builder may) becomes a CHAIN of extra records: the first 127 primitives as the RIGHT child, the
// rest as the left one, both with the leaf's own box.  With equal boxes the walk takes the right
// child first (closest hit: `h2 > h1` is false; any hit: second sibling first), so the
// primitives are still tested in obj_indices order, and a chunk the shortened ray no longer
// reaches holds no hit the reference could have accepted (its entry distance exceeds maxT).
// Images are identical; the event counts gain the chain's node visits.
bool leaf_ref(Tree& t, const VimgBVHNode& n, const float* bmin, const float* bmax, uint32_t& out) {
  if (uint64_t(n.first_index) + n.obj_count > (1u << 25)) return false;
  uint32_t first = n.first_index, count = n.obj_count, links = 0;
  if (count <= 127u) {
    out = (count << 25) | first;
    return true;
  }
  // build the chain back to front: the last link's left child is the (<= 127) remainder
  std::vector<std::pair<uint32_t, uint32_t>> chunks;   // (first, count) in test order
  while (count > 127u) {
    chunks.push_back({first, 127u});
    first += 127u, count -= 127u;
  }
  uint32_t rest = (count << 25) | first;
  for (size_t i = chunks.size(); i-- > 0;) {
    DNode dn{};
    pack_boxes(dn, bmin, bmax, bmin, bmax);
    dn.left_ref = rest;
    dn.right_ref = (chunks[i].second << 25) | chunks[i].first;
    t.chain.push_back(dn);
    t.chain_leaf.push_back(n.first_index);
    t.chain_leaf.push_back(n.obj_count);
    rest = static_cast<uint32_t>(t.n_internal + t.chain.size() - 1);
    ++links;
  }
  t.chain_depth = std::max(t.chain_depth, links);
  out = rest;
  return true;
}

int renumber_bvh(const VimgBVH& b, Tree& t) {
  std::vector<uint32_t> order;   // internal nodes: new index -> old index
  std::vector<uint32_t> new_of(b.num_nodes, 0);
  std::vector<uint32_t> level;   // internal nodes: new index -> depth below the root
  if (b.nodes[0].obj_count == 0) order.push_back(0), level.push_back(0);
  for (size_t head = 0; head < order.size(); ++head) {
    const VimgBVHNode& n = b.nodes[order[head]];
    for (uint32_t c = n.first_index; c <= n.first_index + 1; ++c)
      if (b.nodes[c].obj_count == 0) {
        new_of[c] = static_cast<uint32_t>(order.size());
        order.push_back(c);
        level.push_back(level[head] + 1);
      }
  }
  t.n_internal = static_cast<uint32_t>(order.size());
  // breadth-first numbering makes every level one index range: a refit runs them deepest first
  for (size_t i = 0; i < order.size(); ++i)
    if (i == 0 || level[i] != level[i - 1]) t.level_begin.push_back(static_cast<uint32_t>(i));
  t.level_begin.push_back(t.n_internal);
  t.nodes.resize(order.size());
  for (size_t i = 0; i < order.size(); ++i) {
    const VimgBVHNode& n = b.nodes[order[i]];
    DNode dn{};
    uint32_t refs[2];
    const float* bb = b.bb_mins_maxes + (size_t(n.first_index) * 2 + 2) * 3;
    const float* lmin = bb, *rmin = bb + 3, *lmax = bb + 6, *rmax = bb + 9;
    for (int k = 0; k < 2; ++k) {
      const uint32_t c = n.first_index + k;
      if (b.nodes[c].obj_count == 0) {
        refs[k] = new_of[c];
      } else if (!leaf_ref(t, b.nodes[c], k == 0 ? lmin : rmin, k == 0 ? lmax : rmax, refs[k])) {
        return fail(VIMG_E_UNSUPPORTED, "BVH with more than 2^25 primitives");
      }
    }
    dn.left_ref = refs[0];
    dn.right_ref = refs[1];
    pack_boxes(dn, lmin, lmax, rmin, rmax);
    t.nodes[i] = dn;
  }
  if (b.nodes[0].obj_count == 0) {
    t.root_ref = 0;
  } else if (!leaf_ref(t, b.nodes[0], b.bb_mins_maxes + 0, b.bb_mins_maxes + 6, t.root_ref)) {
    return fail(VIMG_E_UNSUPPORTED, "BVH with more than 2^25 primitives");
  }
  t.nodes.insert(t.nodes.end(), t.chain.begin(), t.chain.end());
  if (t.nodes.size() >= (1u << 25)) return fail(VIMG_E_UNSUPPORTED, "BVH has more than 2^25 internal nodes");
  if (b.max_depth + t.chain_depth + 2 > 96) return fail(VIMG_E_INVALID, "BVH (with its leaf chains) deeper than the 94-level stack bound");
  return VIMG_OK;
}

// ---- per-triangle shading records and area pdfs
void bake_triangles(const VimgScene* sc, std::vector<DTriShade>& shade, std::vector<float>& area_pdf) {
  shade.resize(sc->num_tris);
  area_pdf.resize(sc->num_tris);
  for (uint32_t t = 0; t < sc->num_tris; ++t) {
    const VimgMesh& m = sc->meshes[sc->tri_mesh[t]];
    DTriShade ts{};
    ts.mesh = sc->tri_mesh[t];
    ts.i0 = m.first_vertex + sc->tri_indices[t * 3 + 0];
    ts.i1 = m.first_vertex + sc->tri_indices[t * 3 + 1];
    ts.i2 = m.first_vertex + sc->tri_indices[t * 3 + 2];
    const uint32_t ids[3] = {ts.i0, ts.i1, ts.i2};
    for (int k = 0; k < 3; ++k)
      for (int a = 0; a < 3; ++a) ts.p[k * 3 + a] = sc->vertices[size_t(ids[k]) * 3 + a];
    bake_tri_normal_pdf(ts.p, ts.n, &area_pdf[t]);
    shade[t] = ts;
  }
}

// ---- leaf slots, in obj_indices order
std::vector<DLeafPrim> bake_leaves(const VimgScene* sc, const std::vector<DTriShade>& shade) {
  std::vector<DLeafPrim> leaf(sc->num_prims);
  for (uint32_t j = 0; j < sc->num_prims; ++j) {
    const uint32_t prim = sc->bvh.obj_indices[j];
    const VimgPrim& p = sc->prims[prim];
    DLeafPrim lp{};
    lp.prim = prim;
    lp.cls = bake_material_class(sc->materials[bake_prim_material(p, shade.data(), sc->meshes, sc->spheres)].type);
    if (p.type == VIMG_PRIM_TRIANGLE) {
      bake_leaf_tri(shade[p.index].p, lp);
    } else {
      bake_leaf_sphere(sc->spheres[p.index], lp);
      lp.kind = 1u;
    }
    leaf[j] = lp;
  }
  return leaf;
}

// ---- emitters, baked (device_scene.h: DLight)
std::vector<DLight> bake_lights(const VimgScene* sc, const std::vector<DTriShade>& shade, const std::vector<float>& area_pdf) {
  std::vector<DLight> dlights(sc->num_lights);
  for (uint32_t i = 0; i < sc->num_lights; ++i)
    dlights[i] = bake_light(sc->lights[i], sc->prims, shade.data(), area_pdf.data(), sc->meshes, sc->spheres, sc->materials);
  return dlights;
}

std::vector<uint32_t> material_flags(const VimgScene* sc, bool* textured) {
  std::vector<uint32_t> mflags(sc->num_materials, 0);
  for (uint32_t i = 0; i < sc->num_materials; ++i) mflags[i] = bake_material_flags(sc->materials[i], sc->textures);
  *textured = tables_textured(sc->materials, sc->num_materials, sc->textures, sc->background);
  return mflags;
}

// the baked and the caller's tables, in the order vimg_hip_scene_bytes has always counted them
int upload_tables(VimgDeviceScene* s, const VimgScene* sc, const Tree& t, const std::vector<DTriShade>& shade,
                  const std::vector<float>& area_pdf, const std::vector<DLeafPrim>& leaf,
                  const std::vector<DLight>& dlights, const std::vector<uint32_t>& mflags) {
  DScene& d = s->d;
#define UP_TO(owner, field, host, count)                     \
  do {                                                       \
    DevBuf& b_ = owner;                                      \
    if (int rc_ = upload(s, b_, host, count)) return rc_;    \
    d.field = (decltype(d.field))b_.p;                       \
  } while (0)
#define UP(field, host, count) UP_TO(s->tables.emplace_back(), field, host, count)
  UP_TO(s->nodes, nodes, t.nodes.data(), t.nodes.size());
  UP_TO(s->leaf_prims, leaf_prims, leaf.data(), leaf.size());
  s->num_leaf_prims = static_cast<uint32_t>(leaf.size());
  UP(prims, sc->prims, sc->num_prims);
  UP(tri_shade, shade.data(), shade.size());
  UP(tri_area_pdf, area_pdf.data(), area_pdf.size());
  UP(meshes, sc->meshes, sc->num_meshes);
  UP(normals, sc->normals, size_t(sc->num_vertices) * 3);
  UP(uvs, sc->uvs, sc->num_uvs * 2);
  UP(spheres, sc->spheres, sc->num_spheres);
  UP(materials, sc->materials, sc->num_materials);
  UP(material_flags, mflags.data(), mflags.size());
  UP(textures, sc->textures, sc->num_textures);
  UP(texels, sc->texels, sc->num_texels * 3);
  UP(rg_textures, sc->rg_textures, sc->num_rg_textures);
  UP(rg_texels, sc->rg_texels, sc->num_rg_texels * 2);
  UP(lights, sc->lights, sc->num_lights);
  s->lights_table = s->tables.size() - 1;   // (a material update may swap these two)
  UP(dlights, dlights.data(), dlights.size());
  s->dlights_table = s->tables.size() - 1;
  UP(cdf_pool, sc->cdf_pool, sc->num_cdf);
#undef UP
#undef UP_TO
  {   // the baked material records: filled by a kernel, from the materials and texture records now resident
    DevBuf& b = s->tables.emplace_back();
    if (int rc = b.alloc(std::max<size_t>(sc->num_materials, 1) * sizeof(DMaterial))) return rc;
    s->total_bytes += b.bytes;
    s->dmaterials_table = s->tables.size() - 1;
    d.dmaterials = (decltype(d.dmaterials))b.p;
    if (int rc = enqueue_material_bake(d, sc->num_materials, b.as<DMaterial>(), nullptr)) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
  }
  if (!t.chain_leaf.empty()) {   // (refit bookkeeping: not counted in the scene's bytes)
    if (int rc = s->chain_leaf.alloc(t.chain_leaf.size() * sizeof(uint32_t))) return rc;
    HIP_TRY(hipMemcpy(s->chain_leaf.p, t.chain_leaf.data(), s->chain_leaf.bytes, hipMemcpyHostToDevice));
  }
  return VIMG_OK;
}

// what a later update needs of the caller's tables: the counts, the vertex rows that carry normals, and the small
// tables a material update is checked against
void record_for_updates(VimgDeviceScene* s, const VimgScene* sc) {
  s->materials.assign(sc->materials, sc->materials + sc->num_materials);
  s->has_other = table_holds_other(s->materials.data(), s->materials.size());
  s->textures.assign(sc->textures, sc->textures + sc->num_textures);
  s->lights.assign(sc->lights, sc->lights + sc->num_lights);
  s->num_rg_textures = sc->num_rg_textures;
  s->num_texels = sc->num_texels;
  s->num_cdf = sc->num_cdf;
  s->num_vertices = sc->num_vertices;
  s->num_tris = sc->num_tris;
  s->num_spheres = sc->num_spheres;
  s->num_meshes = sc->num_meshes;
  for (uint32_t i = 0; i < sc->num_meshes; ++i) {
    const VimgMesh& m = sc->meshes[i];
    if (!m.has_normals || m.num_vertices == 0) continue;
    auto& r = s->normal_rows;
    if (!r.empty() && r.back().first + r.back().second == m.first_vertex)
      r.back().second += m.num_vertices;
    else
      r.push_back({m.first_vertex, m.num_vertices});
  }
}

// the caller's options, the tools' environment overrides, and what the library derives from the scene
int resolve_options(VimgDeviceScene* s, const VimgHipOptions* opts) {
  // LANE register budget: scenes beyond the on-chip caches are latency-bound and want more waves
  // per SIMD; small scenes are VALU-bound and want the build that spills least
  s->waves_per_simd = (s->total_bytes > (32u << 20)) ? 3 : 2;
  vimg_hip_options_default(&s->opt);
  if (opts) {
    // accept shorter (older) structs: fields beyond the caller's struct_size stay AUTO
    const size_t n = std::min<size_t>(opts->struct_size, sizeof(VimgHipOptions));
    if (n >= sizeof(uint32_t)) std::memcpy(&s->opt, opts, n);
    s->opt.struct_size = sizeof(VimgHipOptions);
  }
  options_from_env(&s->opt);
  if (const char* e = getenv("VIMG_HIP_QUERY_BLOCKS")) s->query_launch = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("VIMG_HIP_PLAIN")) s->force_general = atoi(e) == 0;   // 0: the general build of render_cu_kernel for every launch
  if (const char* e = getenv("VIMG_HIP_LDS_TABLES")) s->no_lds_tables = atoi(e) == 0;   // 0: the shading tables stay in global memory
  if (s->opt.scheduler != VIMG_OPT_AUTO && (s->opt.scheduler < VIMG_SCHED_LANE || s->opt.scheduler > VIMG_SCHED_CU))
    return fail(VIMG_E_INVALID, "options: unknown scheduler");
  // the one gate: every launch builder relies on a resident scene's scheduler being AUTO, LANE or CU
  if (s->opt.scheduler != VIMG_OPT_AUTO && s->opt.scheduler != VIMG_SCHED_LANE && s->opt.scheduler != VIMG_SCHED_CU)
    return fail(VIMG_E_UNSUPPORTED, "options: the schedulers POOL, POOL4, POOL4G and STAGE are retired; "
                                    "the library renders with CU (AUTO) or LANE");
  s->too_wide = (s->d.res_x > 65535 || s->d.res_y > 65535);   // slots pack pixel coordinates in 16 bits
  return VIMG_OK;
}

int alloc_scratch(VimgDeviceScene* s) {
  hipDeviceProp_t prop{};
  if (hipGetDeviceProperties(&prop, g_device) != hipSuccess) return fail(VIMG_E_DEVICE, "hipGetDeviceProperties failed");
  s->num_cus = static_cast<uint32_t>(prop.multiProcessorCount);
  if (int rc = s->stats.alloc(sizeof(DeviceStats))) return rc;
  if (int rc = s->counter.alloc(2 * sizeof(unsigned int))) return rc;
  if (int rc = s->root_box.alloc(6 * sizeof(float))) return rc;
  HIP_TRY(hipMemset(s->counter.p, 0, s->counter.bytes));
  return VIMG_OK;
}

// validated scene -> resident scene; on an error the caller drops `s` and what it holds by then
int build_scene(VimgDeviceScene* s, const VimgScene* sc, const VimgHipOptions* opts) {
  DScene& d = s->d;
  bake_camera(sc->camera, d);
  Tree tree;
  if (int rc = renumber_bvh(sc->bvh, tree)) return rc;
  d.root_ref = tree.root_ref;
  for (int a = 0; a < 3; ++a) {
    d.root_min[a] = sc->bvh.bb_mins_maxes[0 * 3 + a];
    d.root_max[a] = sc->bvh.bb_mins_maxes[2 * 3 + a];
  }
  d.num_nodes = static_cast<uint32_t>(tree.nodes.size());
  d.max_depth = sc->bvh.max_depth + tree.chain_depth;   // a chain link pushes one entry like any internal node
  s->n_internal = tree.n_internal;
  s->n_chain = static_cast<uint32_t>(tree.chain.size());
  s->level_begin = tree.level_begin;
  std::vector<DTriShade> shade;
  std::vector<float> area_pdf;
  bake_triangles(sc, shade, area_pdf);
  const std::vector<DLeafPrim> leaf = bake_leaves(sc, shade);
  const std::vector<DLight> dlights = bake_lights(sc, shade, area_pdf);
  const std::vector<uint32_t> mflags = material_flags(sc, &s->textured);
  if (int rc = upload_tables(s, sc, tree, shade, area_pdf, leaf, dlights, mflags)) return rc;
  record_for_updates(s, sc);
  d.num_lights = sc->num_lights;
  d.background = sc->background;
  d.background_emissive = background_is_emissive(sc->background);
  if (int rc = resolve_options(s, opts)) return rc;
  return alloc_scratch(s);
}

}  // namespace

extern "C" {

int vimg_hip_scene_upload(const VimgScene* sc, VimgDeviceScene** out) {
  return vimg_hip_scene_upload_opts(sc, nullptr, out);
}

int vimg_hip_scene_upload_opts(const VimgScene* sc, const VimgHipOptions* opts, VimgDeviceScene** out) {
  if (!out) return fail(VIMG_E_INVALID, "null output pointer");
  *out = nullptr;
  if (g_device < 0) {
    int rc = vimg_hip_init(0);
    if (rc) return rc;
  }
  int rc = validate(sc);
  if (rc) return rc;
  auto s = std::make_unique<VimgDeviceScene>();
  rc = build_scene(s.get(), sc, opts);
  if (rc) return rc;
  *out = s.release();
  return VIMG_OK;
}

int vimg_hip_scene_free(VimgDeviceScene* s) {
  if (!s) return VIMG_OK;
  delete s;
  return VIMG_OK;
}

int64_t vimg_hip_scene_bytes(const VimgDeviceScene* s) {
  return s ? static_cast<int64_t>(s->total_bytes) : 0;
}

// ---- changes of a resident scene.  Argument errors are found before anything is enqueued,
// so they leave the scene as it was; a change that passes them bumps the scene's generation, which a progressive
// accumulator compares before its next increment.  The scene's update entry point: positions, then (callers
// whose struct has the fields) images, tables and emitters.
int vimg_hip_scene_update_geometry(VimgDeviceScene* s, const VimgGeometryUpdate* caller, void* stream) {
  if (!s || !caller) return fail(VIMG_E_INVALID, "update_geometry: null scene or update");
  if (caller->struct_size != VIMG_GEOMETRY_UPDATE_V1_SIZE && caller->struct_size < sizeof(VimgGeometryUpdate))
    return fail(VIMG_E_INVALID, "update_geometry: struct_size is neither the 32 bytes of the first layout nor sizeof(VimgGeometryUpdate)");
  VimgGeometryUpdate update{};   // the caller's fields; the ones its struct does not have stay 0 = unchanged
  std::memcpy(&update, caller, std::min<size_t>(caller->struct_size, sizeof(update)));
  const VimgGeometryUpdate* u = &update;
  if (int rc = check_relight(s, u)) return rc;
  RelightPlan plan;
  if (int rc = prepare_relight(s, u, &plan)) return rc;
  hipStream_t st = stream_of(stream);
  ++s->generation;
  if (u->normals)   // rows of meshes without normals keep what the upload gave them
    for (const auto& r : s->normal_rows)
      HIP_TRY(hipMemcpyAsync((float*)s->d.normals + size_t(r.first) * 3, static_cast<const float*>(u->normals) + size_t(r.first) * 3,
                             size_t(r.second) * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
  SceneUpdate up{};
  up.vertices = static_cast<const float*>(u->vertices);
  up.spheres = static_cast<const float*>(u->spheres);
  up.num_tris = s->num_tris;
  up.num_spheres = s->num_spheres;
  up.num_slots = s->num_leaf_prims;
  up.n_internal = s->n_internal;
  up.n_chain = s->n_chain;
  up.chain_leaf = s->chain_leaf.as<const uint32_t>();
  up.level_begin = s->level_begin.data();
  up.num_levels = static_cast<uint32_t>(s->level_begin.size() - 1);
  up.root_box = s->root_box.as<float>();
  HIP_TRY(enqueue_scene_update(s->d, up, st));
  if (plan.any)
    if (int rc = enqueue_relight(s, u, &plan, st)) return rc;
  float box[6];
  HIP_TRY(hipMemcpyAsync(box, s->root_box.p, sizeof(box), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int a = 0; a < 3; ++a) s->d.root_min[a] = box[a], s->d.root_max[a] = box[3 + a];
  if (plan.any) commit_relight(s, u, &plan);
  return VIMG_OK;
}

int vimg_hip_scene_set_camera(VimgDeviceScene* s, const VimgCamera* cam) {
  if (!s || !cam) return fail(VIMG_E_INVALID, "set_camera: null scene or camera");
  if (cam->res_x != s->d.res_x || cam->res_y != s->d.res_y)
    return fail(VIMG_E_INVALID, "set_camera: the resolution is fixed at upload");
  bake_camera(*cam, s->d);
  ++s->generation;
  return VIMG_OK;
}

}  // extern "C"
