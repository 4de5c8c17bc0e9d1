// Host side of the C-ABI layer: HIP error reporting and the owners of device memory, streams and events.  Every device
// array, stream and event of a handle is a member of one of these types and is released with the handle.
#ifndef MFGPU_DEVICE_H
#define MFGPU_DEVICE_H

#include <hip/hip_runtime.h>

#include <atomic>
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

// Guard mode (mfgpu_debug_guard_*, mfgpu_guard.hip; off unless a caller switches it on): an allocation becomes
// [front guard | payload | back guard] with both guards and every unfilled floating-point payload set to 0xFF bytes
// (a NaN as double and as float), and is registered until it is freed.  The payload begins 256-byte aligned, as a bare
// hipMalloc's does.
extern std::atomic<size_t> g_guard_bytes;  // 0: the mode is off
// the padded allocation of `bytes` payload bytes: *payload and its distance *front (> 0) from the hipMalloc'ed base
int guard_alloc(void **payload, size_t *front, size_t bytes, size_t guard, bool zero, bool poison);
void guard_free(void *payload, size_t front);

// One device allocation of n elements of T.  DeviceArray<void> counts in bytes and is read through as<Number>(): the
// arrays whose element is the operator's number type.  A DeviceArray<T> moves into a DeviceArray<void>.
template <typename T>
class DeviceArray {
  static constexpr size_t elem = sizeof(typename std::conditional<std::is_void<T>::value, char, T>::type);
  template <typename U>
  friend class DeviceArray;

 public:
  DeviceArray() = default;
  DeviceArray(DeviceArray &&o) noexcept : p_(o.p_), bytes_(o.bytes_), front_(o.front_) {
    o.p_ = nullptr, o.bytes_ = 0, o.front_ = 0;
  }
  template <typename U>
  DeviceArray(DeviceArray<U> &&o) noexcept : p_(o.p_), bytes_(o.bytes_), front_(o.front_) {
    o.p_ = nullptr, o.bytes_ = 0, o.front_ = 0;
  }
  DeviceArray &operator=(DeviceArray &&o) noexcept {
    std::swap(p_, o.p_);
    std::swap(bytes_, o.bytes_);
    std::swap(front_, o.front_);
    return *this;
  }
  ~DeviceArray() {
    if (front_)
      guard_free(p_, front_);
    else
      hipFree(p_);
  }

  // without `zero` the payload is unspecified (guard mode: 0xFF bytes where T is a floating-point type or void, the
  // Number arrays; integer arrays are left alone, an all-ones index would be a wild address)
  int alloc(size_t n, bool zero = false) { return alloc_(n, zero, floating); }
  int upload(const void *host, size_t n) {  // n = 0 leaves the array empty
    if (const int rc = alloc_(n, false, false)) return rc;
    if (n) HIP_TRY(hipMemcpy(p_, host, bytes_, hipMemcpyHostToDevice));
    return 0;
  }
  T *get() const { return p_; }
  template <typename Number>
  Number *as() const {
    static_assert(std::is_void<T>::value, "typed arrays are read through get()");
    return static_cast<Number *>(p_);
  }
  size_t bytes() const { return bytes_; }  // of the payload

 private:
  static constexpr bool floating = std::is_void<T>::value || std::is_floating_point<T>::value;

  int alloc_(size_t n, bool zero, bool poison) {
    *this = DeviceArray();
    if (n == 0) return 0;
    if (const size_t guard = g_guard_bytes.load(std::memory_order_relaxed)) {
      if (const int rc = guard_alloc((void **)&p_, &front_, n * elem, guard, zero, poison)) return rc;
      bytes_ = n * elem;
      return 0;
    }
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

  T *p_ = nullptr;
  size_t bytes_ = 0;
  size_t front_ = 0;  // guard mode: bytes between the hipMalloc'ed base and p_
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
