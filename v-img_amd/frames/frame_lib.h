// The host skeleton of a frame library (libvimg_filter.so ... libvimg_rectify.so, twelve so far): the
// error slot, the argument checks a frame library is made of, the workspace check, the launch shape, the radius
// dispatch and the launch check.  Internal: not installed, not in include/.  A unit #defines FRAME_LIB ("atrous")
// before it includes this: it opens every sentence made here and in reproject.h, which the libraries that reproject a
// history include after it; guides.h holds the tap score of the spatial ones, tile.h the apron tile of the windowed ones.
// A unit writes its own kernels, its parameter ranges, the order of its checks and the sentences only it has; the
// sentences every library says - about its two structs, a missing frame, an alignment, an overlap - it gets from here.
// Everything is in an anonymous namespace: each library gets its own copy, and above all its own error slot.  One
// inline variable of default visibility would be one weak symbol in two libraries, which the dynamic linker may
// merge - vimg_filter_last_error() would then return the temporal library's message.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <span>
#include <type_traits>
#include <utility>

#include "vimg_hip.h"

#ifndef FRAME_LIB
#error "define FRAME_LIB, the prefix of the library's error sentences, before including frame_lib.h"
#endif

namespace vimg_frames {
namespace {

// ---- the error slot: the message of this thread's last failed call ------------------------------------------------
thread_local char g_error[256] = "";

__attribute__((format(printf, 2, 3))) int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
  return code;
}

// ---- argument checks: VIMG_OK, or VIMG_E_INVALID with the sentence set ---------------------------------------------
// What every frame library checks first, in this order, of its frames struct and the struct beside it, whose noun is
// `second` ("params"; motion's is "geometry"): both given, both of their size, the extent in range.
template <class Frames, class Second>
int check_structs(const Frames* f, const Second* a, const char* second, uint32_t max_extent) {
  static_assert(offsetof(Frames, struct_size) == 0 && offsetof(Frames, width) == 4 && offsetof(Frames, height) == 8,
                "a frames struct opens with struct_size, width, height");
  static_assert(offsetof(Second, struct_size) == 0, "a params struct opens with its struct_size");
  if (!f) return fail(VIMG_E_INVALID, FRAME_LIB ": null frames");
  if (!a) return fail(VIMG_E_INVALID, FRAME_LIB ": null %s", second);
  if (f->struct_size < sizeof(Frames))
    return fail(VIMG_E_INVALID, FRAME_LIB ": frames.struct_size %u is below the struct's %zu", f->struct_size, sizeof(Frames));
  if (a->struct_size < sizeof(Second))
    return fail(VIMG_E_INVALID, FRAME_LIB ": %s.struct_size %u is below the struct's %zu", second, a->struct_size, sizeof(Second));
  if (f->width == 0 || f->height == 0 || f->width > max_extent || f->height > max_extent)
    return fail(VIMG_E_INVALID, FRAME_LIB ": width and height must be 1..%u, not %u x %u", max_extent, f->width, f->height);
  return VIMG_OK;
}

// the pointers a call cannot do without, {pointer, name}: the first null one in the order given, as a `kind`
int check_present(std::initializer_list<std::pair<const void*, const char*>> needed, const char* kind = "frame") {
  for (const auto& [p, name] : needed)
    if (!p) return fail(VIMG_E_INVALID, FRAME_LIB ": null %s %s", name, kind);
  return VIMG_OK;
}

// The two over the four frames most libraries read (VimgFilterFrames, VimgTemporalFrames ...: offsets 0 .. 40, for
// which Python has one binding helper); a library whose frames struct holds other pointers calls the two itself.
template <class Frames, class Params>
int check_head(const Frames* f, const Params* a, uint32_t max_extent) {
  static_assert(offsetof(Frames, reserved) == 12 && offsetof(Frames, color) == 16 && offsetof(Frames, normal) == 24 &&
                    offsetof(Frames, position) == 32 && offsetof(Frames, depth) == 40,
                "a frame library's frames struct opens with the shared eight fields");
  if (const int rc = check_structs(f, a, "params", max_extent)) return rc;
  return check_present({{f->color, "color"}, {f->normal, "normal"}, {f->position, "position"}, {f->depth, "depth"}});
}

// a parameter field: above `low` (`strict`) or at least `low`, never NaN, finite unless `may_be_inf`
int check_float(const char* name, float v, float low, bool strict, bool may_be_inf) {
  if ((strict ? v > low : v >= low) && (may_be_inf || std::isfinite(v))) return VIMG_OK;
  return fail(VIMG_E_INVALID, FRAME_LIB ": %s must be %s %g%s, not %g", name, strict ? ">" : ">=", double(low),
              may_be_inf ? " (it may be +inf)" : " and finite", double(v));
}

bool misaligned(const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to != 0; }

bool overlaps(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + b_bytes && pb < pa + a_bytes;
}

// a buffer a call reads or writes, by the name its sentences give it; null or of no bytes: not there
struct Range {
  const void* p;
  uint64_t bytes;
  const char* name;
};

// the first of `among` that the `bytes` at `p` overlap, or null; the caller makes its own sentence of it
const Range* first_overlap(const void* p, uint64_t bytes, std::span<const Range> among) {
  for (const Range& r : among)
    if (r.p && r.bytes && overlaps(p, bytes, r.p, r.bytes)) return &r;
  return nullptr;
}

// the caller's workspace of `have` bytes, of which a w x h frame needs `need`
int check_workspace(const void* workspace, uint64_t have, uint64_t need, uint32_t w, uint32_t h) {
  if (!workspace) return fail(VIMG_E_INVALID, FRAME_LIB ": null workspace");
  if (have < need)
    return fail(VIMG_E_INVALID, FRAME_LIB ": the workspace has %llu bytes, %u x %u needs %llu", static_cast<unsigned long long>(have),
                w, h, static_cast<unsigned long long>(need));
  if (misaligned(workspace, 16)) return fail(VIMG_E_INVALID, FRAME_LIB ": the workspace must be 16-byte aligned");
  return VIMG_OK;
}

// ---- the launch shape: one lane per pixel, a wave is 64 consecutive pixels of one row, the tail is a bounds test ----
constexpr int WAVE_X = 64, ROWS = 4;    // blockDim: a wave per row segment, four rows per workgroup

__device__ inline bool pixel_of(uint32_t w, uint32_t h, int& x, int& y) {
  x = int(blockIdx.x * WAVE_X + threadIdx.x);
  y = int(blockIdx.y * ROWS + threadIdx.y);
  return uint32_t(x) < w && uint32_t(y) < h;
}

inline dim3 pixel_block() { return dim3(WAVE_X, ROWS); }
inline dim3 pixel_grid(uint32_t w, uint32_t h) { return dim3((w + WAVE_X - 1) / WAVE_X, (h + ROWS - 1) / ROWS); }

// ---- the radius dispatch: launch(R) with `radius` as a compile-time constant, std::integral_constant<int, 1..MAX>; a
// radius above MAX goes to MAX - its range was checked before.  For the kernels whose window is a template argument:
//   with_radius<3>(a->radius, [&](auto R) { clamp_kernel<R.value><<<grid, block, 0, s>>>(...); });
// It counts down from MAX; the kernels then stand in the device code as a switch over 1 .. MAX had them.
template <int MAX, class Launch>
void with_radius(uint32_t radius, Launch&& launch) {
  if constexpr (MAX > 1)
    if (radius < MAX) return with_radius<MAX - 1>(radius, launch);
  launch(std::integral_constant<int, MAX>{});
}

// ---- the launch check: a refusal is read right after the launch, so nothing is enqueued behind a stage that did not
// start; an error left by an earlier HIP call of this thread is not this call's and is cleared before the first launch
inline void clear_stale_error() { (void)hipGetLastError(); }

inline int launched(const char* stage = nullptr) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return VIMG_OK;
  return stage ? fail(VIMG_E_DEVICE, FRAME_LIB ": %s launch failed: %s", stage, hipGetErrorString(e))
               : fail(VIMG_E_DEVICE, FRAME_LIB ": launch failed: %s", hipGetErrorString(e));
}

}  // namespace
}  // namespace vimg_frames
