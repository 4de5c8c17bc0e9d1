// Host side of the C-ABI layer: HIP error reporting and the owners of device memory, streams and events.  Every device
// array, stream and event of a handle is a member of one of these types and is released with the handle.
#ifndef MFGPU_DEVICE_H
#define MFGPU_DEVICE_H

#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <utility>

#include "mfgpu_internal.h"

namespace mfgpu {

// 0, or the error code of a failed HIP call with "<what>: <HIP's message>" left for mfgpu_last_error()
inline int hip_check(hipError_t e, const char *what) {
  if (e == hipSuccess) return 0;
  set_error(std::string(what) + ": " + hipGetErrorString(e));
  return e == hipErrorOutOfMemory ? MFGPU_ENOMEM : MFGPU_EHIP;
}
#define HIP_TRY(expr)                                                        \
  do {                                                                       \
    if (const int rc_ = mfgpu::hip_check((expr), #expr)) return rc_;         \
  } while (0)

// MFGPU_EINVAL with msg left for mfgpu_last_error()
inline int einval(const char *msg) {
  set_error(msg);
  return MFGPU_EINVAL;
}

inline size_t esize(int number_type) { return number_type == MFGPU_F32 ? 4 : 8; }
inline bool valid_number_type(int number_type) { return number_type == MFGPU_F64 || number_type == MFGPU_F32; }

// One device allocation of n elements of T.  DeviceArray<void> counts in bytes and is read through as<Number>(): the
// arrays whose element is the operator's number type.  A DeviceArray<T> moves into a DeviceArray<void>.
template <typename T>
class DeviceArray {
  static constexpr size_t elem = sizeof(typename std::conditional<std::is_void<T>::value, char, T>::type);
  template <typename U>
  friend class DeviceArray;

 public:
  DeviceArray() = default;
  DeviceArray(DeviceArray &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
  template <typename U>
  DeviceArray(DeviceArray<U> &&o) noexcept : p_(o.p_), bytes_(o.bytes_) {
    o.p_ = nullptr, o.bytes_ = 0;
  }
  DeviceArray &operator=(DeviceArray &&o) noexcept {
    std::swap(p_, o.p_);
    std::swap(bytes_, o.bytes_);
    return *this;
  }
  ~DeviceArray() { hipFree(p_); }

  int alloc(size_t n, bool zero = false) {
    *this = DeviceArray();
    if (n == 0) return 0;
    HIP_TRY(hipMalloc((void **)&p_, n * elem));
    bytes_ = n * elem;
    if (zero) {
      // hipMemset on device memory may return before the fill has run; it is ordered on the null stream, which a
      // non-blocking stream does not wait for: complete it here (set-up time) so that the first kernel on any stream
      // reads zeros
      HIP_TRY(hipMemset(p_, 0, bytes_));
      HIP_TRY(hipStreamSynchronize(nullptr));
    }
    return 0;
  }
  int upload(const void *host, size_t n) {  // n = 0 leaves the array empty
    if (const int rc = alloc(n)) return rc;
    if (n) HIP_TRY(hipMemcpy(p_, host, bytes_, hipMemcpyHostToDevice));
    return 0;
  }
  T *get() const { return p_; }
  template <typename Number>
  Number *as() const {
    static_assert(std::is_void<T>::value, "typed arrays are read through get()");
    return static_cast<Number *>(p_);
  }
  size_t bytes() const { return bytes_; }

 private:
  T *p_ = nullptr;
  size_t bytes_ = 0;
};

class Stream {
 public:
  Stream() = default;
  Stream(Stream &&o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream &operator=(Stream &&o) noexcept {
    std::swap(s_, o.s_);
    return *this;
  }
  ~Stream() {
    if (s_) hipStreamDestroy(s_);
  }
  int create(unsigned flags, int priority) {
    HIP_TRY(hipStreamCreateWithPriority(&s_, flags, priority));
    return 0;
  }
  hipStream_t get() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

class Event {
 public:
  Event() = default;
  Event(Event &&o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event &operator=(Event &&o) noexcept {
    std::swap(e_, o.e_);
    return *this;
  }
  ~Event() {
    if (e_) hipEventDestroy(e_);
  }
  int create(unsigned flags) {
    HIP_TRY(hipEventCreateWithFlags(&e_, flags));
    return 0;
  }
  hipEvent_t get() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace mfgpu
#endif
