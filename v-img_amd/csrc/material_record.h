// DMaterial: what a Principled or Lambertian vertex derives from its material record alone, baked once per
// material.  Plain C++ (no HIP): device_scene.h includes it beside DLight, the host asks
// dmaterial_bits, and tests/test_material_bake.py compiles it stand-alone.
//
// Every field is the value of an expression of principled_eval_pdf, sample_mat or eval_pdf_pair
// (render_kernels.h), evaluated by the statements of material_terms.h in a kernel (scene_bake_materials,
// scene_relight.hip): the same text the stages run for a material whose validity bit is clear, compiled with the
// same flags, so a stage that loads a field gets the bits it would have computed.
//
// Read today: by sample_mat w.choose_* and w.sum*, coat[].alpha_g, alpha[].ax / ay, salpha, eta[].eta; by
// principled_eval_pdf base, c_sheen, k_s, sqrt_base, all of alpha[] and all of coat[]; by the Lambertian
// evaluation base.  Baked and NOT read by any stage yet: r0, spec_r0, c_0, one_minus_c_0, eta[].eta2,
// eta[].inv_eta2 and w.mix_*.  principled_eval_pdf computes these, because loading them there put scratch into
// the untextured render kernels; they stay in the record, kept fresh by the same bake, for the
// attempt that finds the registers.
#pragma once
#include <stdint.h>

#include "../../include/vimg_scene.h"

#if defined(__HIP__) || defined(__CUDACC__)
#define VIMG_HD __host__ __device__ inline
#else
#define VIMG_HD inline
#endif

namespace vimg {

// alphax, alphay of one roughness and one regularisation variant, and what the glass and the metal lobe form of them
struct DMatAlpha {
  float ax, ay;
  float ax2, ay2;     // alphax * alphax, alphay * alphay
  double pi_axay;     // kPi * alphax * alphay (the double it is in the lobes' D)
};
// the clearcoat lobe's alpha_g of one regularisation variant
struct DMatCoat {
  float alpha_g, ag2;   // ag2 = alpha_g * alpha_g
  float ag2m1;          // (ag2 - 1.f)
  float pad;
  double ag2m1_d;       // (ag2 - 1.)
  double pi_log;        // kPi * F_log(ag2)
};
// the glass lobe's eta on one side of the surface
struct DMatEta {
  float eta, eta2, inv_eta2;   // eta * eta, 1.f / (eta * eta)
  float pad;
};
// lobe choice and mixing: principled.h:168-205, principled.cpp:28-52
struct DMatWeights {
  float choose_diff, choose_clearcoat, choose_metal, choose_glass;
  float sum2, sum3, sum4;   // the partial sums of choose_* that sample_mat compares its draw with
  float mix_diff, mix_sheen, mix_coat, mix_metal, mix_glass;   // the factors of eval_principled
};

enum : uint32_t {
  DMAT_SCALARS = 1u,   // the scalar group holds for the textured builds too: a Principled material without mr_tex
  DMAT_COLOUR = 2u,    // the colour group holds: Lambertian or Principled with a VIMG_TEX_CONST colour texture
};

struct __attribute__((aligned(16))) DMaterial {
  uint32_t bits;               // DMAT_*
  // ---- scalar group: from metallic_factor, roughness_factor (a metallic-roughness map scales both per hit: bit clear)
  float r0;                    // the metal lobe's R0 of eta
  float spec_r0;               // specular * R0 * (1.f - metallic)
  float pad0;
  DMatWeights w;
  DMatAlpha alpha[2];          // clamped roughness (evaluation; the glass lobe when sampling): [regularize]
  float salpha[2][2];          // unclamped roughness (the metal lobe when sampling): [regularize]{alphax, alphay}
  DMatCoat coat[2];            // [regularize]
  DMatEta eta[2];              // [0] entering (dot(ng, dir_in) >= 0): the material's eta, [1] leaving: 1.f / eta
  // ---- colour group
  float base[3];               // the constant base colour
  float c_sheen[3], k_s[3];
  float c_0[3], one_minus_c_0[3];   // (these two need the scalar group as well)
  float sqrt_base[3];
  float pad1[2];
};
static_assert(sizeof(DMatAlpha) == 24 && sizeof(DMatCoat) == 32 && sizeof(DMatEta) == 16 && sizeof(DMatWeights) == 48,
              "DMaterial's groups have fixed sizes");
static_assert(sizeof(DMaterial) == 304 && alignof(DMaterial) == 16, "DMaterial must be 304 bytes, 16-byte aligned");

// which groups of a material's record the stages may load
VIMG_HD uint32_t dmaterial_bits(const VimgMaterial& m, const VimgTexture* textures) {
  uint32_t b = 0;
  if (m.type == VIMG_MAT_PRINCIPLED && m.mr_tex < 0) b |= DMAT_SCALARS;
  if ((m.type == VIMG_MAT_PRINCIPLED || m.type == VIMG_MAT_LAMBERTIAN) && m.tex >= 0 && textures[m.tex].type == VIMG_TEX_CONST)
    b |= DMAT_COLOUR;
  return b;
}

}  // namespace vimg
