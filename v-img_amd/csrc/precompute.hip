// Work around a scene's upload, on the GPU with host buffers in and out: the texture pre-pass (mip chains,
// environment-map CDFs, 8-bit decodes) and the tonemap / 8-bit post step of a finished frame.
#include <cmath>

#include "hip_internal.h"
#include "post_kernels.h"
#include "pre_kernels.h"

using namespace vimg;

extern "C" {

int vimg_hip_post_rgb8(const void* d_rgb, int w, int h, int tonemapper, void* d_rgb8, void* stream) {
  if (!d_rgb || !d_rgb8 || w <= 0 || h <= 0 || tonemapper < 0 || tonemapper > 3)
    return fail(VIMG_E_INVALID, "post_rgb8: bad arguments");
  if (g_device < 0) {
    int rc = vimg_hip_init(0);
    if (rc) return rc;
  }
  hipStream_t st = stream_of(stream);
  const size_t n = size_t(w) * h;
  static unsigned int* d_max = nullptr;   // (deliberately of the process, never freed: per call it would add an allocation to every post step)
  if (!d_max) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_max), sizeof(unsigned int)));
  if (tonemapper == 2) {
    HIP_TRY(hipMemsetAsync(d_max, 0, sizeof(unsigned int), st));
    hipLaunchKernelGGL(post_max_luminance_kernel, dim3(1024), dim3(256), 0, st,
                       static_cast<const float*>(d_rgb), n, d_max);
  }
  hipLaunchKernelGGL(post_rgb8_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0,
                     st, static_cast<const float*>(d_rgb), n, tonemapper, d_max,
                     static_cast<unsigned char*>(d_rgb8));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));
  return VIMG_OK;
}

// ---- the pre-step of the path on the GPU; host buffers in and out: these
// replace the host library's OpenMP loops while a scene is being assembled, before the upload
namespace {
int pre_ready() {
  if (g_device < 0) return vimg_hip_init(0);
  return VIMG_OK;
}
uint32_t pre_grid(size_t n) { return static_cast<uint32_t>(std::min<size_t>((n + 255) / 256, 65536)); }
}  // namespace

}  // extern "C"

// ---- the launches themselves, on device buffers: the host-buffer entry points below and the image update of a
// resident scene (scene_relight.hip) both go through these, so both run the same kernels on the same grids
namespace vimg {

void enqueue_mip_levels(float* texels, const uint64_t* level_offset, uint32_t levels, uint32_t w, uint32_t h, uint32_t wrap_u,
                        uint32_t wrap_v, hipStream_t st) {
  uint32_t pw = w, ph = h;
  for (uint32_t l = 1; l < levels; ++l) {
    const uint32_t nw = std::max(pw / 2u, 1u), nh = std::max(ph / 2u, 1u);
    hipLaunchKernelGGL(pre_mip_level_kernel, dim3((nw + 31) / 32, (nh + 7) / 8), dim3(256), 0, st, texels + level_offset[l - 1] * 3, pw, ph,
                       texels + level_offset[l] * 3, nw, nh, wrap_u, wrap_v);
    pw = nw, ph = nh;
  }
}

std::vector<float> env_sin_table(uint32_t h) {
  // sin(pi * v) per row, in double as the reference evaluates it (sampling.h:180-181)
  std::vector<float> sin_elev(h);
  for (uint32_t y = 0; y < h; ++y) {
    float v = (static_cast<float>(y) + 0.5f) / static_cast<float>(h);
    sin_elev[y] = static_cast<float>(std::sin(3.141592653589793238462643383279502884 * v));
  }
  return sin_elev;
}

void enqueue_env_cdfs(const float* img, uint32_t w, uint32_t h, const EnvCdfScratch& t, float* row_cdf, float* col_cdfs, hipStream_t st) {
  const size_t n = size_t(w) * h;
  hipLaunchKernelGGL(pre_env_lum_kernel, dim3(pre_grid(n)), dim3(256), 0, st, img, w, h, t.sin_elev, t.lum);
  // one conditional distribution per image row, then the marginal over the row integrals
  hipLaunchKernelGGL(pre_cdf_scan_kernel, dim3(h), dim3(64), 0, st, t.lum, h, w, col_cdfs, t.row_int);
  hipLaunchKernelGGL(pre_cdf_normalise_kernel, dim3(pre_grid(size_t(h) * (w + 1))), dim3(256), 0, st, col_cdfs, h, w, t.row_int);
  hipLaunchKernelGGL(pre_cdf_scan_kernel, dim3(1), dim3(64), 0, st, t.row_int, 1u, h, row_cdf, t.row_tot);
  hipLaunchKernelGGL(pre_cdf_normalise_kernel, dim3(pre_grid(size_t(h) + 1)), dim3(256), 0, st, row_cdf, 1u, h, t.row_tot);
}

}  // namespace vimg

extern "C" {

uint64_t vimg_hip_mip_chain_texels(uint32_t w, uint32_t h, uint32_t* num_levels) {
  if (w == 0 || h == 0) {
    if (num_levels) *num_levels = 0;
    return 0;
  }
  // level count of the reference: min(ceil(log2(min(w, h))), 15), never fewer than level 0
  const int levels = std::max(1, std::min(static_cast<int>(std::ceil(std::log2(static_cast<float>(std::min(w, h))))),
                                          VIMG_MAX_MIP_LEVELS));
  uint64_t total = 0;
  uint32_t lw = w, lh = h;
  for (int l = 0; l < levels; ++l) {
    total += uint64_t(lw) * lh;
    lw = std::max(lw / 2u, 1u), lh = std::max(lh / 2u, 1u);
  }
  if (num_levels) *num_levels = static_cast<uint32_t>(levels);
  return total;
}

int vimg_hip_build_mip_chain(uint32_t w, uint32_t h, const float* level0, uint32_t wrap_u,
                             uint32_t wrap_v, float* out_levels) {
  if (!level0 || !out_levels || w == 0 || h == 0 || wrap_u > 2 || wrap_v > 2)
    return fail(VIMG_E_INVALID, "build_mip_chain: bad arguments");
  if (int rc = pre_ready()) return rc;
  uint32_t levels = 0;
  const uint64_t texels = vimg_hip_mip_chain_texels(w, h, &levels);
  DevBuf d;
  if (int rc = d.alloc(texels * 3 * sizeof(float))) return rc;
  float* base = d.as<float>();
  HIP_TRY(hipMemcpyAsync(base, level0, size_t(w) * h * 3 * sizeof(float), hipMemcpyHostToDevice, g_stream));
  uint64_t offsets[VIMG_MAX_MIP_LEVELS] = {0};   // each level behind the one before
  {
    uint32_t lw = w, lh = h;
    for (uint32_t l = 1; l < levels; ++l) {
      offsets[l] = offsets[l - 1] + uint64_t(lw) * lh;
      lw = std::max(lw / 2u, 1u), lh = std::max(lh / 2u, 1u);
    }
  }
  enqueue_mip_levels(base, offsets, levels, w, h, wrap_u, wrap_v, g_stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out_levels, base, texels * 3 * sizeof(float), hipMemcpyDeviceToHost, g_stream));
  HIP_TRY(hipStreamSynchronize(g_stream));
  return VIMG_OK;
}

int vimg_hip_build_env_cdfs(const float* img, uint32_t w, uint32_t h, float* row_cdf, float* col_cdfs) {
  if (!img || !row_cdf || !col_cdfs || w == 0 || h == 0)
    return fail(VIMG_E_INVALID, "build_env_cdfs: bad arguments");
  if (int rc = pre_ready()) return rc;
  const std::vector<float> sin_elev = env_sin_table(h);
  const size_t n = size_t(w) * h;
  DevBuf d_img, d_sin, d_lum, d_cdf, d_rowint, d_rowcdf, d_rowtot;
  if (int rc = d_img.alloc(n * 3 * sizeof(float))) return rc;
  if (int rc = d_sin.alloc(h * sizeof(float))) return rc;
  if (int rc = d_lum.alloc(n * sizeof(float))) return rc;
  if (int rc = d_cdf.alloc(size_t(h) * (w + 1) * sizeof(float))) return rc;
  if (int rc = d_rowint.alloc(h * sizeof(float))) return rc;
  if (int rc = d_rowcdf.alloc((size_t(h) + 1) * sizeof(float))) return rc;
  if (int rc = d_rowtot.alloc(sizeof(float))) return rc;
  HIP_TRY(hipMemcpyAsync(d_img.p, img, n * 3 * sizeof(float), hipMemcpyHostToDevice, g_stream));
  HIP_TRY(hipMemcpyAsync(d_sin.p, sin_elev.data(), h * sizeof(float), hipMemcpyHostToDevice, g_stream));
  enqueue_env_cdfs(d_img.as<float>(), w, h, EnvCdfScratch{d_sin.as<float>(), d_lum.as<float>(), d_rowint.as<float>(), d_rowtot.as<float>()},
                   d_rowcdf.as<float>(), d_cdf.as<float>(), g_stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(col_cdfs, d_cdf.p, size_t(h) * (w + 1) * sizeof(float), hipMemcpyDeviceToHost, g_stream));
  HIP_TRY(hipMemcpyAsync(row_cdf, d_rowcdf.p, (size_t(h) + 1) * sizeof(float), hipMemcpyDeviceToHost, g_stream));
  HIP_TRY(hipStreamSynchronize(g_stream));
  return VIMG_OK;
}

int vimg_hip_lut8_to_float(const uint8_t* in, uint64_t n, const float* lut256, float* out) {
  if (!in || !lut256 || !out) return fail(VIMG_E_INVALID, "lut8_to_float: bad arguments");
  if (n == 0) return VIMG_OK;
  if (int rc = pre_ready()) return rc;
  DevBuf d_in, d_lut, d_out;
  if (int rc = d_in.alloc(n)) return rc;
  if (int rc = d_lut.alloc(256 * sizeof(float))) return rc;
  if (int rc = d_out.alloc(n * sizeof(float))) return rc;
  HIP_TRY(hipMemcpyAsync(d_in.p, in, n, hipMemcpyHostToDevice, g_stream));
  HIP_TRY(hipMemcpyAsync(d_lut.p, lut256, 256 * sizeof(float), hipMemcpyHostToDevice, g_stream));
  hipLaunchKernelGGL(pre_lut8_kernel, dim3(pre_grid(n)), dim3(256), 0, g_stream, d_in.as<uint8_t>(), size_t(n),
                     d_lut.as<float>(), d_out.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, d_out.p, n * sizeof(float), hipMemcpyDeviceToHost, g_stream));
  HIP_TRY(hipStreamSynchronize(g_stream));
  return VIMG_OK;
}

int vimg_hip_rgb8_to_normal(const uint8_t* rgb8, uint64_t n_pixels, float scale, float* out) {
  if (!rgb8 || !out) return fail(VIMG_E_INVALID, "rgb8_to_normal: bad arguments");
  if (n_pixels == 0) return VIMG_OK;
  if (int rc = pre_ready()) return rc;
  DevBuf d_in, d_out;
  if (int rc = d_in.alloc(n_pixels * 3)) return rc;
  if (int rc = d_out.alloc(n_pixels * 3 * sizeof(float))) return rc;
  HIP_TRY(hipMemcpyAsync(d_in.p, rgb8, n_pixels * 3, hipMemcpyHostToDevice, g_stream));
  hipLaunchKernelGGL(pre_normal8_kernel, dim3(pre_grid(n_pixels)), dim3(256), 0, g_stream, d_in.as<uint8_t>(),
                     size_t(n_pixels), scale, d_out.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, d_out.p, n_pixels * 3 * sizeof(float), hipMemcpyDeviceToHost, g_stream));
  HIP_TRY(hipStreamSynchronize(g_stream));
  return VIMG_OK;
}

}  // extern "C"
