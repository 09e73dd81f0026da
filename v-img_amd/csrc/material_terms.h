// The terms of a Principled or Lambertian vertex that depend on the material record alone, stated once.  Two
// callers run these statements: scene_bake_materials (scene_relight.hip), which fills a DMaterial per material at
// upload and after every edit, and the stages of render_kernels.h for a material whose validity bit is clear
// (a checkerboard or image base colour; a metallic-roughness map in the TEX builds).  Every unit that includes
// this header is built with -ffp-contract=off and without fast-math, and F_log is one OCML call, so a stage that
// loads a baked field reads the bits it would have computed.
//
// The expressions are those of the reference's lobes (include/material/principled.h:100-205,
// src/material/principled.cpp:5-58, disney_helpers/*.h) with their operand order and their promotions to double.
#pragma once
#include "device_math.h"
#include "material_record.h"

namespace vimg {

VD void regularize_alpha(float& ax, float& ay) {   // MatConst, include/material/material.h:19-23
  ax = ax < 0.1f ? clampf(2.f * ax, 0.03f, 0.1f) : ax;
  ay = ay < 0.1f ? clampf(2.f * ay, 0.03f, 0.1f) : ay;
}

// alphax, alphay of a roughness: the evaluation and the glass lobe pass clampf(roughness, 0.01f, 1.f), the metal
// lobe's sampling the roughness itself (disney_glass.h:118 vs disney_metal.h:92-96)
VD void mat_alphas(float roughness, float anisotropic, bool regularize, float& alphax, float& alphay) {
  constexpr float alpha_min = 0.0001;
  const float aspect = sqrt_f(1.f - 0.9f * anisotropic);
  const float roughness_square = roughness * roughness;
  alphax = sel_max(alpha_min, roughness_square / aspect);
  alphay = sel_max(alpha_min, roughness_square * aspect);
  if (regularize) regularize_alpha(alphax, alphay);
}
// ... and what the D of the glass and of the metal lobe forms of them
VD DMatAlpha mat_alpha_terms(float roughness, float anisotropic, bool regularize) {
  DMatAlpha a;
  mat_alphas(roughness, anisotropic, regularize, a.ax, a.ay);
  a.ax2 = a.ax * a.ax;
  a.ay2 = a.ay * a.ay;
  a.pi_axay = kPi * a.ax * a.ay;
  return a;
}

// the clearcoat lobe's alpha_g (disney_clearcoat.h:66-70,113-117) and the terms of its D
VD float mat_alpha_g(float gloss, bool regularize) {
  float alpha_g = (1.f - gloss) * 0.1f + gloss * 0.001f;
  alpha_g = regularize && (alpha_g < 0.1f) ? clampf(2.f * alpha_g, 0.03f, 0.1f) : alpha_g;
  return alpha_g;
}
VD DMatCoat mat_coat_terms(float gloss, bool regularize) {
  DMatCoat c;
  c.alpha_g = mat_alpha_g(gloss, regularize);
  const float ag2 = c.alpha_g * c.alpha_g;
  c.ag2 = ag2;
  c.ag2m1 = (ag2 - 1.f);
  c.pad = 0.f;
  c.ag2m1_d = (ag2 - 1.);
  c.pi_log = kPi * F_log(ag2);
  return c;
}

// the glass lobe's eta on the side the ray comes from (disney_glass.h:120,196)
VD DMatEta mat_eta_terms(float mat_eta, bool entering) {
  DMatEta e;
  e.eta = entering ? mat_eta : 1.f / mat_eta;
  e.eta2 = e.eta * e.eta;
  e.inv_eta2 = 1.f / (e.eta * e.eta);
  e.pad = 0.f;
  return e;
}

// the metal lobe's R0 (disney_metal.h:131) and the scalar factor of its c_0
VD float mat_r0(float eta) { return ((eta - 1.f) * (eta - 1.f)) / ((eta + 1.f) * (eta + 1.f)); }
VD float mat_spec_r0(float specular, float R0, float metallic) { return (specular * R0 * (1.f - metallic)); }

// lobe weights, the choice among them and the mixing factors of eval_principled
VD DMatWeights mat_weight_terms(float metallic, float st, float clearcoat, float sheen) {
  DMatWeights w;
  w.mix_diff = (1.f - st) * (1.f - metallic);
  w.mix_sheen = (1.f - metallic) * sheen;
  w.mix_coat = 0.25f * clearcoat;
  w.mix_metal = (1.f - st * (1.f - metallic));
  w.mix_glass = (1.f - metallic) * st;
  float diffuse_weight = (1.f - metallic) * (1.f - st);
  float clearcoat_weight = 0.25f * clearcoat;
  float metal_weight = (1.f - st * (1.f - metallic));
  float glass_weight = (1.f - metallic) * st;
  float total_w = diffuse_weight + clearcoat_weight + metal_weight + glass_weight;
  w.choose_diff = diffuse_weight / total_w;
  w.choose_clearcoat = clearcoat_weight / total_w;
  w.choose_metal = metal_weight / total_w;
  w.choose_glass = glass_weight / total_w;
  w.sum2 = (w.choose_diff + w.choose_clearcoat);
  w.sum3 = (w.choose_diff + w.choose_clearcoat + w.choose_metal);
  w.sum4 = (w.choose_diff + w.choose_clearcoat + w.choose_metal + w.choose_glass);
  return w;
}

// ---- the colour group
VD f3 mat_c_tint(f3 base_color) {
  const float base_lum = dot(base_color, f3{0.212671f, 0.715160f, 0.072169f});   // luminance()
  return base_lum > 0 ? base_color / base_lum : splat3(1.f);
}
VD f3 mat_c_sheen(f3 c_tint, float sheen_tint) { return (splat3(1.f) - splat3(sheen_tint)) + sheen_tint * c_tint; }
VD f3 mat_k_s(f3 c_tint, float spec_tint) { return (splat3(1.f) - splat3(spec_tint)) + spec_tint * c_tint; }
VD f3 mat_c_0(float spec_r0, f3 k_s, float metallic, f3 base_color) { return spec_r0 * k_s + metallic * base_color; }
VD f3 mat_one_minus(f3 c_0) { return (splat3(1.f) - c_0); }
VD f3 mat_sqrt3(f3 base_color) { return f3{sqrt_f(base_color.x), sqrt_f(base_color.y), sqrt_f(base_color.z)}; }

// One whole record.  metallic and roughness are the factors themselves (principled_prologue without a map:
// 1.f * factor); base_color is read only when the colour bit is set.
VD DMaterial bake_dmaterial(const VimgMaterial& m, uint32_t bits, f3 base_color) {
  DMaterial r{};
  r.bits = bits;
  if (m.type == VIMG_MAT_PRINCIPLED) {
    const float metallic = 1.f * m.metallic_factor, roughness = 1.f * m.roughness_factor;
    r.r0 = mat_r0(m.eta);
    r.spec_r0 = mat_spec_r0(m.specular, r.r0, metallic);
    r.w = mat_weight_terms(metallic, m.specular_transmission, m.clearcoat, m.sheen);
    for (int reg = 0; reg < 2; ++reg) {
      r.alpha[reg] = mat_alpha_terms(clampf(roughness, 0.01f, 1.f), m.anisotropic, reg != 0);
      mat_alphas(roughness, m.anisotropic, reg != 0, r.salpha[reg][0], r.salpha[reg][1]);
      r.coat[reg] = mat_coat_terms(m.clearcoat_gloss, reg != 0);
    }
    r.eta[0] = mat_eta_terms(m.eta, true);
    r.eta[1] = mat_eta_terms(m.eta, false);
  }
  if (bits & DMAT_COLOUR) {
    auto put = [](float* dst, f3 v) { dst[0] = v.x, dst[1] = v.y, dst[2] = v.z; };
    put(r.base, base_color);
    if (m.type == VIMG_MAT_PRINCIPLED) {
      const f3 c_tint = mat_c_tint(base_color);
      const f3 k_s = mat_k_s(c_tint, m.specular_tint);
      const f3 c_0 = mat_c_0(r.spec_r0, k_s, 1.f * m.metallic_factor, base_color);
      put(r.c_sheen, mat_c_sheen(c_tint, m.sheen_tint));
      put(r.k_s, k_s);
      put(r.c_0, c_0);
      put(r.one_minus_c_0, mat_one_minus(c_0));
      put(r.sqrt_base, mat_sqrt3(base_color));
    }
  }
  return r;
}

}  // namespace vimg
