// How the host units report a HIP error (fail, HIP_TRY) and the two types that own what hipMalloc and
// hipEventCreate hand out.  Every device allocation and every event of the library belongs to one DevBuf /
// DevEvent - a local of the call, or a member of the scene, accumulator or tree it lives with - and is released
// by that owner's destructor: no return path frees by hand.  Not exported (hip_internal.h includes it).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>

#include "../../include/vimg_hip.h"

#pragma GCC visibility push(hidden)
namespace vimg {

int fail(int code, const std::string& msg);   // sets vimg_hip_last_error of this thread; returns code
#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(VIMG_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));        \
  } while (0)

// Device memory and its size in bytes.  Move-only: a move (or swap) hands the memory to another owner.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {   // what this owned is freed, `o` is left empty
    DevBuf(std::move(o)).swap(*this);
    return *this;
  }
  ~DevBuf() { if (p) (void)hipFree(p); }
  void swap(DevBuf& o) noexcept { std::swap(p, o.p), std::swap(bytes, o.bytes); }
  template <typename T> T* as() const { return static_cast<T*>(p); }
  // `need` bytes of new memory (one hipMalloc, nothing written to it); what the buffer held is freed first
  int alloc(size_t need) {
    if (p) HIP_TRY(hipFree(p));
    p = nullptr, bytes = 0;
    HIP_TRY(hipMalloc(&p, need));
    bytes = need;
    return VIMG_OK;
  }
  // at least `need` bytes: nothing happens when the buffer is large enough, the contents are lost when it grows
  int grow(size_t need) { return need <= bytes ? VIMG_OK : alloc(need); }
};

struct DevEvent {
  hipEvent_t e = nullptr;
  DevEvent() = default;
  DevEvent(DevEvent&& o) noexcept : e(std::exchange(o.e, nullptr)) {}
  DevEvent& operator=(DevEvent&& o) noexcept {
    DevEvent(std::move(o)).swap(*this);
    return *this;
  }
  ~DevEvent() { if (e) (void)hipEventDestroy(e); }
  void swap(DevEvent& o) noexcept { std::swap(e, o.e); }
  int create() {
    HIP_TRY(hipEventCreate(&e));
    return VIMG_OK;
  }
};

}  // namespace vimg
#pragma GCC visibility pop
