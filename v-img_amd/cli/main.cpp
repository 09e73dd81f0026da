// vimg-amd: the C++ host program around the GPU hot path — the counterpart of the reference's
// main (src/main.cpp:38-377) with its flags: -f scene.json, -t threads (ignored: the render runs
// on the GPU), -c tonemapper 0-3 (clamp, AgX, Reinhard, ACES; default AgX as main.cpp:97-114),
// -d "x y" single-pixel trace, -b 0 binned / 1 sweep BVH (default 0 as main.cpp:183-187),
// -m factor heatmap mode (BVH traversal cost, main.cpp:62-65,98-100,250-256), plus
// -s spp override, -p step progressive rendering (increments of `step` samples, the PNG rewritten
// after each; the last one is byte-identical to a plain run), -e target adaptive sampling on top of -p (increments
// only where the estimated relative error of a pixel is above `target`, -s the cap per pixel), -a prefix (the feature
// buffers of the frame beside the image: prefix_albedo.png, prefix_normal.png as (n + 1) / 2, prefix_depth.png
// divided by the image's largest depth, all through the clamp tonemapper), -n iterations (the picture written is the
// a-trous filtered frame: libvimg_filter on the frame and its albedo / normal / position / depth feature frames at the
// frame's sample count, with the library's other defaults; with -p every preview and the final file) and -o output path.  Scene loading, the SAH BVH build and PNG writing happen
// here on the host (libvimg_host); the render and the post chain go through the C ABI of
// libvimg_hip.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "vimg_filter.h"
#include "vimg_hip.h"
#include "vimg_host.h"

static double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv) {
  std::string scene_path, out_path = "v_img_amd.png", aux_prefix;
  int tonemapper = 0, bvh_type = VIMG_BVH_BINNED, px = -1, py = -1;   // clamp, as src/main.cpp:46
  long spp_override = -1, prog_step = 0, filter_iterations = 0;
  float heatmap_max = -1.f, err_target = -1.f;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : ""; };
    if (a == "-f") scene_path = next();
    else if (a == "-t") next();
    else if (a == "-c") {
      // an out-of-range value is ignored and the default kept (src/main.cpp:107-112)
      const int v = std::atoi(next());
      if (v >= 0 && v < 4) tonemapper = v;
    }
    else if (a == "-b") bvh_type = std::atoi(next()) == 1 ? VIMG_BVH_SWEEP : VIMG_BVH_BINNED;
    else if (a == "-s") spp_override = std::atol(next());
    else if (a == "-p") prog_step = std::atol(next());
    else if (a == "-e") err_target = static_cast<float>(std::atof(next()));
    else if (a == "-m") heatmap_max = static_cast<float>(std::atof(next()));
    else if (a == "-o") out_path = next();
    else if (a == "-a") aux_prefix = next();
    else if (a == "-n") {
      // 1..12 as the library has it: 0, a negative value or no number at all must not write the unfiltered frame
      char* end = nullptr;
      const char* v = next();
      filter_iterations = std::strtol(v, &end, 10);
      if (end == v || *end != '\0' || filter_iterations < 1 || filter_iterations > long(VIMG_ATROUS_MAX_ITERATIONS)) {
        std::fprintf(stderr, "-n iterations must be 1..%u, not \"%s\"\n", VIMG_ATROUS_MAX_ITERATIONS, v);
        return 2;
      }
    }
    else if (a == "-d") {
      if (std::sscanf(next(), "%d %d", &px, &py) != 2) {
        std::fprintf(stderr, "-d needs \"x y\"\n");
        return 2;
      }
    } else {
      std::fprintf(stderr, "usage: vimg-amd -f scene.json [-c 0..3] [-b 0|1] [-m factor] [-s spp] [-p step [-e target]] [-d \"x y\"] [-a prefix] [-n iterations] [-o out.png]\n");
      return 2;
    }
  }
  if (err_target >= 0.f && prog_step <= 0) {   // adaptive sampling is a loop of increments: it needs their size
    std::fprintf(stderr, "-e target needs -p step\nusage: vimg-amd -f scene.json [-c 0..3] [-b 0|1] [-m factor] [-s spp] [-p step [-e target]] [-d \"x y\"] [-a prefix] [-n iterations] [-o out.png]\n");
    return 2;
  }
  if (!aux_prefix.empty() && (heatmap_max >= 0.f || px >= 0)) {   // feature buffers go beside a rendered image only
    std::fprintf(stderr, "-a prefix goes with a rendered image: not with -m or -d\nusage: vimg-amd -f scene.json [-c 0..3] [-b 0|1] [-m factor] [-s spp] [-p step [-e target]] [-d \"x y\"] [-a prefix] [-n iterations] [-o out.png]\n");
    return 2;
  }
  if (filter_iterations != 0 && (heatmap_max >= 0.f || px >= 0)) {   // as -a: the filter needs a rendered image
    std::fprintf(stderr, "-n iterations goes with a rendered image: not with -m or -d\nusage: vimg-amd -f scene.json [-c 0..3] [-b 0|1] [-m factor] [-s spp] [-p step [-e target]] [-d \"x y\"] [-a prefix] [-n iterations] [-o out.png]\n");
    return 2;
  }
  if (scene_path.empty()) {
    std::fprintf(stderr, "No input file given\n");
    return 2;
  }
  double t0 = now_s();
  VimgHostScene* hs = nullptr;
  if (vimg_host_scene_from_json_file(scene_path.c_str(), &hs) != 0) {
    std::fprintf(stderr, "scene loading failed: %s\n", vimg_host_last_error());
    return 1;
  }
  double t1 = now_s();
  if (vimg_host_build_bvh(hs, bvh_type) != 0) {
    std::fprintf(stderr, "BVH build failed: %s\n", vimg_host_last_error());
    return 1;
  }
  const VimgScene* view = vimg_host_scene_view(hs);
  double t2 = now_s();
  std::printf("Number of lights loaded %u\nNumber of Surfaces loaded %u\nBVH max depth %u\n",
              view->num_lights, view->num_prims, view->bvh.max_depth);
  std::printf("scene loading %.3f s, BVH construction (%s) %.3f s\n", t1 - t0,
              bvh_type == VIMG_BVH_SWEEP ? "sweep" : "binned", t2 - t1);

  VimgRenderParams params;
  vimg_host_default_params(hs, &params);
  if (spp_override > 0) params.samples = static_cast<uint32_t>(spp_override);
  // main forces 4 spp and the clamp tonemapper for the normal integrators (src/main.cpp:220-237)
  // ... and for the heatmap (src/main.cpp:250-254)
  const bool heatmap = heatmap_max >= 0.f && px < 0;
  if (heatmap || params.integrator == VIMG_INTEGRATOR_S_NORMAL ||
      params.integrator == VIMG_INTEGRATOR_G_NORMAL) {
    params.samples = 4;   // unconditionally, -s or not: the reference overwrites the sample count here
    tonemapper = 0;
  }
  const int W = view->camera.res_x, H = view->camera.res_y;
  std::printf("Image resolution %dx%d, samples per pixel %u, max ray depth %u\n", W, H,
              params.samples, params.depth);

  VimgDeviceScene* dev = nullptr;
  if (vimg_hip_init(0) != VIMG_OK || vimg_hip_scene_upload(view, &dev) != VIMG_OK) {
    std::fprintf(stderr, "GPU set-up failed: %s\n", vimg_hip_last_error());
    return 1;
  }
  if (px >= 0) {
    float rgb[3];
    if (vimg_hip_trace_pixel(dev, &params, px, py, rgb) != VIMG_OK) {
      std::fprintf(stderr, "trace_pixel failed: %s\n", vimg_hip_last_error());
      return 1;
    }
    std::printf("Value of pixel in linear space is (%.9g, %.9g, %.9g)\n", rgb[0], rgb[1], rgb[2]);
    return 0;
  }
  float* d_rgb = nullptr;
  unsigned char* d_rgb8 = nullptr;
  const size_t n = size_t(W) * H;
  if (hipMalloc(reinterpret_cast<void**>(&d_rgb), n * 3 * sizeof(float)) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&d_rgb8), n * 3) != hipSuccess) {
    std::fprintf(stderr, "hipMalloc failed\n");
    return 1;
  }
  // -n: the guides of the frame, rendered once (they do not depend on the increments of -p), and the filter in
  // place on d_rgb.  The filter only enqueues on the null stream, so the frame is waited for before the post chain.
  float* d_guides[4] = {nullptr, nullptr, nullptr, nullptr};
  void* d_work = nullptr;
  auto denoise = [&]() -> bool {
    if (filter_iterations == 0) return true;
    static const uint32_t guide[4] = {VIMG_INTEGRATOR_ALBEDO, VIMG_INTEGRATOR_NORMAL, VIMG_INTEGRATOR_POSITION,
                                      VIMG_INTEGRATOR_DEPTH};
    const uint64_t work_bytes = vimg_filter_atrous_workspace(uint32_t(W), uint32_t(H));
    if (!d_work) {
      if (hipMalloc(&d_work, work_bytes) != hipSuccess) {
        std::fprintf(stderr, "hipMalloc failed\n");
        return false;
      }
      for (int g = 0; g < 4; ++g) {
        VimgRenderParams q = params;
        q.integrator = guide[g];
        if (hipMalloc(reinterpret_cast<void**>(&d_guides[g]), n * 3 * sizeof(float)) != hipSuccess ||
            vimg_hip_render(dev, &q, d_guides[g], nullptr, nullptr) != VIMG_OK) {
          std::fprintf(stderr, "feature render failed: %s\n", vimg_hip_last_error());
          return false;
        }
      }
    }
    VimgFilterFrames fr{};
    fr.struct_size = sizeof fr;
    fr.width = uint32_t(W);
    fr.height = uint32_t(H);
    fr.color = d_rgb;
    fr.albedo = d_guides[0];
    fr.normal = d_guides[1];
    fr.position = d_guides[2];
    fr.depth = d_guides[3];
    VimgAtrousParams ap;
    vimg_filter_atrous_defaults(&ap);
    ap.iterations = static_cast<uint32_t>(filter_iterations);
    if (vimg_filter_atrous(&fr, &ap, d_rgb, d_work, work_bytes, nullptr) != VIMG_OK) {
      std::fprintf(stderr, "filter failed: %s\n", vimg_filter_last_error());
      return false;
    }
    if (hipStreamSynchronize(nullptr) != hipSuccess) {
      std::fprintf(stderr, "filter failed on the device\n");
      return false;
    }
    return true;
  };
  VimgRenderStats st;
  double t3 = now_s();
  if (heatmap) {
    std::printf("Creating Heatmap for ray intersection\nHeatmap factor set to %g\n",
                heatmap_max <= 0 ? 20.0 : double(heatmap_max));
    if (vimg_hip_render_heatmap(dev, &params, heatmap_max, d_rgb, nullptr) != VIMG_OK) {
      std::fprintf(stderr, "heatmap failed: %s\n", vimg_hip_last_error());
      return 1;
    }
    std::printf("image rendering %.3f s\n", now_s() - t3);
  } else if (prog_step > 0) {
    // progressive: increments of prog_step samples (the last one may be shorter), each picture a valid preview
    VimgProgressive* acc = nullptr;
    if (vimg_hip_progressive_create(dev, &params, &acc) != VIMG_OK) {
      std::fprintf(stderr, "progressive set-up failed: %s\n", vimg_hip_last_error());
      return 1;
    }
    std::vector<uint8_t> rgb8(n * 3);
    // -e: two increments for everyone (the error needs two), then only the pixels vimg_hip_progressive_select
    // names - those all stand at `done`, so every step is one launch - until none is left or -s is reached
    const bool adaptive = err_target >= 0.f;
    uint8_t* d_mask = nullptr;
    if (adaptive && hipMalloc(reinterpret_cast<void**>(&d_mask), n) != hipSuccess) {
      std::fprintf(stderr, "hipMalloc failed\n");
      return 1;
    }
    uint32_t active = static_cast<uint32_t>(n);
    for (uint32_t done = 0; done < params.samples;) {
      const uint32_t k = static_cast<uint32_t>(std::min<long>(prog_step, long(params.samples - done)));
      const bool masked = adaptive && done >= 2u * static_cast<uint32_t>(prog_step);
      if (masked) {
        if (vimg_hip_progressive_select(acc, err_target, params.samples, d_mask, nullptr, &active) != VIMG_OK) {
          std::fprintf(stderr, "select failed: %s\n", vimg_hip_last_error());
          return 1;
        }
        if (active == 0) break;
      }
      if (vimg_hip_progressive_render_masked(dev, acc, k, masked ? d_mask : nullptr, d_rgb, nullptr, nullptr) != VIMG_OK) {
        std::fprintf(stderr, "render failed: %s\n", vimg_hip_last_error());
        return 1;
      }
      done += k;
      if (!denoise()) return 1;
      if (vimg_hip_post_rgb8(d_rgb, W, H, tonemapper, d_rgb8, nullptr) != VIMG_OK ||
          hipMemcpy(rgb8.data(), d_rgb8, n * 3, hipMemcpyDeviceToHost) != hipSuccess ||
          vimg_host_write_png(out_path.c_str(), rgb8.data(), W, H) != 0) {
        std::fprintf(stderr, "preview write failed: %s %s\n", vimg_hip_last_error(), vimg_host_last_error());
        return 1;
      }
      if (adaptive)
        std::printf("samples %u / %u, active pixels %u (%.3f s)\n", done, params.samples, active, now_s() - t3);
      else
        std::printf("samples %u / %u (%.3f s)\n", done, params.samples, now_s() - t3);
      std::fflush(stdout);
    }
    if (d_mask) (void)hipFree(d_mask);
    vimg_hip_progressive_free(acc);
    filter_iterations = 0;   // (d_rgb is the last preview: filtered already)
  } else {
    if (vimg_hip_render(dev, &params, d_rgb, nullptr, &st) != VIMG_OK) {
      std::fprintf(stderr, "render failed: %s\n", vimg_hip_last_error());
      return 1;
    }
    double t4 = now_s();
    const double rays = double(st.closest_rays + st.shadow_rays);
    std::printf("image rendering %.3f s: %.1f Mrays/s (%.4f rays per camera path), %llu NaN samples\n",
                t4 - t3, rays / (t4 - t3) / 1e6, rays / double(st.paths),
                static_cast<unsigned long long>(st.nan_samples));
  }
  if (!heatmap && !denoise()) return 1;
  if (vimg_hip_post_rgb8(d_rgb, W, H, tonemapper, d_rgb8, nullptr) != VIMG_OK) {
    std::fprintf(stderr, "post failed: %s\n", vimg_hip_last_error());
    return 1;
  }
  std::vector<uint8_t> rgb8(n * 3);
  if (hipMemcpy(rgb8.data(), d_rgb8, n * 3, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  if (vimg_host_write_png(out_path.c_str(), rgb8.data(), W, H) != 0) {
    std::fprintf(stderr, "PNG write failed: %s\n", vimg_host_last_error());
    return 1;
  }
  std::printf("output image written to %s\n", out_path.c_str());
  if (!aux_prefix.empty()) {
    // the first-hit feature integrators at the frame's sample count; the mapping to 8 bits is done here on the host
    static const struct { uint32_t integrator; const char* name; } aux[3] = {
        {VIMG_INTEGRATOR_ALBEDO, "albedo"}, {VIMG_INTEGRATOR_NORMAL, "normal"}, {VIMG_INTEGRATOR_DEPTH, "depth"}};
    std::vector<float> img(n * 3);
    for (const auto& f : aux) {
      VimgRenderParams q = params;
      q.integrator = f.integrator;
      if (vimg_hip_render(dev, &q, d_rgb, nullptr, nullptr) != VIMG_OK ||
          hipMemcpy(img.data(), d_rgb, n * 3 * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        std::fprintf(stderr, "%s render failed: %s\n", f.name, vimg_hip_last_error());
        return 1;
      }
      if (f.integrator == VIMG_INTEGRATOR_NORMAL)
        for (float& v : img) v = (v + 1.f) / 2.f;
      if (f.integrator == VIMG_INTEGRATOR_DEPTH) {
        const float deepest = *std::max_element(img.begin(), img.end());
        if (deepest > 0.f)
          for (float& v : img) v /= deepest;
      }
      const std::string path = aux_prefix + "_" + f.name + ".png";
      if (vimg_host_tonemap_to_rgb8(img.data(), W, H, 0, rgb8.data()) != 0 ||
          vimg_host_write_png(path.c_str(), rgb8.data(), W, H) != 0) {
        std::fprintf(stderr, "%s write failed: %s\n", f.name, vimg_host_last_error());
        return 1;
      }
      std::printf("%s written to %s\n", f.name, path.c_str());
    }
  }
  for (float* g : d_guides) (void)hipFree(g);
  (void)hipFree(d_work);
  (void)hipFree(d_rgb);
  (void)hipFree(d_rgb8);
  vimg_hip_scene_free(dev);
  vimg_host_scene_free(hs);
  return 0;
}
