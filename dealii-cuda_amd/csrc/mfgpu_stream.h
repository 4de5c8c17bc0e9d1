// What every streaming vector kernel shares ("Streaming kernels"): the 16-byte access per lane, the
// chunk-and-tail loop, the fixed-order block reduction, the grid rule and the choice of a template instantiation from
// run-time flags.  Included by .hip files only.
// Contract of a kernel on the skeleton: ONE body states the element formula, for a chunk and for a tail element alike;
// every element is read and written by one lane; sums go through block_sum / resum and so have one fixed order.
#ifndef MFGPU_STREAM_H
#define MFGPU_STREAM_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace mfgpu {

constexpr unsigned kStreamBlocks = 2048;  // 256 CUs x 8 resident blocks of 256 threads, grid-stride

template <typename T>
constexpr int lanes16() {
  return 16 / (int)sizeof(T);
}

template <typename T>
__device__ __forceinline__ void ld16(const T *p, T (&v)[lanes16<T>()]) {
  if constexpr (sizeof(T) == 8) {
    const double2 a = *reinterpret_cast<const double2 *>(p);
    v[0] = a.x;
    v[1] = a.y;
  } else {
    const float4 a = *reinterpret_cast<const float4 *>(p);
    v[0] = a.x;
    v[1] = a.y;
    v[2] = a.z;
    v[3] = a.w;
  }
}

template <typename T>
__device__ __forceinline__ void st16(T *p, const T (&v)[lanes16<T>()]) {
  if constexpr (sizeof(T) == 8) {
    *reinterpret_cast<double2 *>(p) = make_double2(v[0], v[1]);
  } else {
    *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// four elements per chunk: one 16-byte access on the float side, two on the double side
template <typename T>
__device__ __forceinline__ void ld4(const T *p, T (&v)[4]) {
  if constexpr (sizeof(T) == 8) {
    T a[2], b[2];
    ld16<T>(p, a);
    ld16<T>(p + 2, b);
    v[0] = a[0], v[1] = a[1], v[2] = b[0], v[3] = b[1];
  } else {
    ld16<T>(p, v);
  }
}
template <typename T>
__device__ __forceinline__ void st4(T *p, const T (&v)[4]) {
  if constexpr (sizeof(T) == 8) {
    const T a[2] = {v[0], v[1]}, b[2] = {v[2], v[3]};
    st16<T>(p, a);
    st16<T>(p + 2, b);
  } else {
    st16<T>(p, v);
  }
}

// W elements at p: W == 1 a scalar access, W == lanes16<T>() the 16-byte access, W == 4 the conversion's chunk
template <int W, typename T>
__device__ __forceinline__ void ldw(const T *p, T (&v)[W]) {
  static_assert(W == 1 || W == lanes16<T>() || W == 4, "a scalar, a 16-byte chunk or four elements");
  if constexpr (W == 1)
    v[0] = *p;
  else if constexpr (W == lanes16<T>())
    ld16<T>(p, v);
  else
    ld4<T>(p, v);
}
template <int W, typename T>
__device__ __forceinline__ void stw(T *p, const T (&v)[W]) {
  static_assert(W == 1 || W == lanes16<T>() || W == 4, "a scalar, a 16-byte chunk or four elements");
  if constexpr (W == 1)
    *p = v[0];
  else if constexpr (W == lanes16<T>())
    st16<T>(p, v);
  else
    st4<T>(p, v);
}

// The skeleton: body(o, width) once per chunk of W elements at offset o = c W (grid-stride over the n / W chunks), then
// once per element of the tail, with width = std::integral_constant<int, W> resp. <int, 1>, so that the body declares
// its `T v[width]` arrays, loads with ldw, applies its element function for k < width and stores with stw, once.
// VEC = false (vectors not 16-byte aligned): the tail loop runs from 0.  tid and stride are the kernel's
// (size_t)blockIdx.x * blockDim.x + threadIdx.x and (size_t)gridDim.x * blockDim.x: formed here, blockDim.x is fetched
// through the generic implicit-argument path and the stride lives in VGPRs (profiles/r12_notes.md).
template <int W, bool VEC, typename Body>
__device__ __forceinline__ void stream_chunks(size_t tid, size_t stride, size_t n, Body &&body) {
  size_t done = 0;
  if (VEC) {
    const size_t nc = n / W;
    for (size_t c = tid; c < nc; c += stride) body(c * W, std::integral_constant<int, W>{});
    done = nc * W;
  }
  for (size_t i = done + tid; i < n; i += stride) body(i, std::integral_constant<int, 1>{});
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

// the block's sum of acc over its 256 threads (wave sums, then the four waves in a fixed order), on every thread, with
// red free for the next sum on return.  ALL = false, for a kernel that ends with the sum: thread 0 alone holds it and
// the second barrier is left out.
template <bool ALL = true>
__device__ __forceinline__ double block_sum(double acc, double *red) {
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (!ALL && threadIdx.x != 0) return 0.0;
  const double s = (red[0] + red[1]) + (red[2] + red[3]);
  if (ALL) __syncthreads();
  return s;
}

// sum of np partials by one block of 256 threads.  vec_reduce_final (mfgpu_aux.hip) is this function, so every block
// that re-sums the same partials holds the bits of that reduction.
template <bool ALL = true>
__device__ __forceinline__ double resum(const double *__restrict__ partial, unsigned np, double *red) {
  double acc = 0.0;
  for (unsigned i = threadIdx.x; i < np; i += 256) acc += partial[i];
  return block_sum<ALL>(acc, red);
}

// blocks of 256 threads for n elements in chunks of W: one thread per chunk and per tail element, grid-stride above
// kStreamBlocks
inline unsigned stream_grid(size_t n, size_t W, bool vec) {
  const size_t work = vec ? n / W + n % W : n, blocks = (work + 255) / 256;
  return (unsigned)(blocks == 0 ? 1 : blocks > kStreamBlocks ? kStreamBlocks : blocks);
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }  // a null (absent) vector counts as aligned

// Run-time flags to template arguments: dispatch(f, a, b, ...) calls f(A, B, ...) with std::true_type / std::false_type
// for a bool and std::integral_constant<int, i> for a OneOf3{i}, i in {0, 1, 2}; in f, `A()` is the constant.
struct OneOf3 {
  int i;
};
template <typename F>
void dispatch(F &&f) {
  f();
}
template <typename F, typename... Rest>
void dispatch(F &&f, OneOf3 v, Rest... rest);
template <typename F, typename... Rest>
void dispatch(F &&f, bool b, Rest... rest) {
  if (b)
    dispatch([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else
    dispatch([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
template <typename F, typename... Rest>
void dispatch(F &&f, OneOf3 v, Rest... rest) {
  if (v.i == 0)
    dispatch([&](auto... c) { f(std::integral_constant<int, 0>{}, c...); }, rest...);
  else if (v.i == 1)
    dispatch([&](auto... c) { f(std::integral_constant<int, 1>{}, c...); }, rest...);
  else
    dispatch([&](auto... c) { f(std::integral_constant<int, 2>{}, c...); }, rest...);
}

}  // namespace mfgpu
#endif
