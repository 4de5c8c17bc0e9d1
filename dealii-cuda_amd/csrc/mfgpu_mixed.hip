// Mixed-precision multigrid and the fused Chebyshev smoother (mixed precision).
//   mfgpu_vec_convert            dst = (dst type) src between double and float vectors: the OtherNumber side of
//                                deal.II's copy_to_mg / copy_from_mg (a float V-cycle under a double CG,
//                                level_number in the reference's bmop_mg.cu:58-59 and poisson_mg.cu:51)
//   mfgpu_vec_chebyshev_start    the vector updates of one PreconditionChebyshev sweep (host/mfgpu_shim_mg.h) in ONE
//   mfgpu_vec_chebyshev_update   launch each instead of the BLAS-1 sequence r.add, t.equ, t.scale, upd.sadd, x.add
//   mfgpu_vec_residual           t = b - t or t = b - (t + e) in one launch instead of add + sadd (the V-cycle's residual)
//   mfgpu_vec_chebyshev_start_dev, mfgpu_vec_chebyshev_update_dev   the two sweep launches with their scalars read from
//                                device memory when the stream gets there (mfgpu_vcycle_refresh)
// All kernels stream: grid-stride over 16-byte chunks per lane (2 doubles or 4 floats; 4 elements for the conversion),
// single elements for the tail (and for vectors that are not 16-byte aligned), no atomics, no LDS, every element
// computed by one lane in a fixed order (deterministic).  All but cheb_update_kernel are one body on the skeleton of
// mfgpu_stream.h.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mfgpu_device.h"
#include "mfgpu_stream.h"

using namespace mfgpu;

namespace {

// dst[i] = (D) src[i]; double -> float rounds to nearest even (overflow gives +-inf), float -> double is exact
template <typename D, typename S, bool VEC>
__global__ void __launch_bounds__(256) convert_kernel(D *__restrict__ dst, const S *__restrict__ src, size_t n) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  stream_chunks<4, VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    S a[W];
    D b[W];
    ldw<W>(src + o, a);
#pragma unroll
    for (int k = 0; k < W; ++k) b[k] = (D)a[k];
    stw<W>(dst + o, b);
  });
}

// r = b - t (t == nullptr: r = b); upd = (f r) dinv; x = upd (ZERO) or x += upd.  The operations and their order are
// those of the BLAS-1 sequence r.equ(1, b), r.add(-1, t), upd.equ(f, r), upd.scale(dinv), x.equ / x.add(1, upd).
template <typename T, bool HAS_T, bool ZERO>
__device__ __forceinline__ void cheb_start_elem(T &x, T &u, T &r, T b, T t, T d, T f) {
  r = HAS_T ? b - t : b;
  u = (f * r) * d;
  x = ZERO ? u : x + u;
}

template <typename T, bool VEC, bool HAS_T, bool ZERO>
__global__ void __launch_bounds__(256)
cheb_start_kernel(T *__restrict__ x, T *__restrict__ upd, T *__restrict__ r, const T *__restrict__ b,
                  const T *__restrict__ t, const T *__restrict__ dinv, T f, size_t n) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T xv[W], uv[W], rv[W], bv[W], tv[W], dv[W];
    ldw<W>(b + o, bv);
    if (HAS_T) ldw<W>(t + o, tv);
    ldw<W>(dinv + o, dv);
    if (!ZERO) ldw<W>(x + o, xv);
#pragma unroll
    for (int k = 0; k < W; ++k) cheb_start_elem<T, HAS_T, ZERO>(xv[k], uv[k], rv[k], bv[k], HAS_T ? tv[k] : T(0), dv[k], f);
    stw<W>(r + o, rv);
    stw<W>(upd + o, uv);
    stw<W>(x + o, xv);
  });
}

// r -= t; upd = f1 upd + (f2 r) dinv; x += upd  (r.add(-1, t), t.equ(f2, r), t.scale(dinv), upd.sadd(f1, 1, t),
// x.add(1, upd) without the store and reload of t)
template <typename T>
__device__ __forceinline__ void cheb_update_elem(T &x, T &u, T &r, T t, T d, T f1, T f2) {
  r = r - t;
  u = f1 * u + (f2 * r) * d;
  x = x + u;
}

// Not on stream_chunks: f1 upd + (f2 r) dinv has two products that the optimiser may contract into the sum, and it
// fuses f1 upd here (in the float tail neither) but (f2 r) dinv in a body called from the skeleton, which changes the
// last bit of upd and x (profiles/r12_notes.md).  Whoever changes the formula changes it in both loops.
template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
cheb_update_kernel(T *__restrict__ x, T *__restrict__ upd, T *__restrict__ r, const T *__restrict__ t,
                   const T *__restrict__ dinv, T f1, T f2, size_t n) {
  constexpr int W = lanes16<T>();
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  size_t done = 0;
  if (VEC) {
    const size_t nc = n / W;
    for (size_t c = tid; c < nc; c += stride) {
      const size_t o = c * W;
      T xv[W], uv[W], rv[W], tv[W], dv[W];
      ld16<T>(r + o, rv);
      ld16<T>(t + o, tv);
      ld16<T>(dinv + o, dv);
      ld16<T>(upd + o, uv);
      ld16<T>(x + o, xv);
#pragma unroll
      for (int k = 0; k < W; ++k) cheb_update_elem<T>(xv[k], uv[k], rv[k], tv[k], dv[k], f1, f2);
      st16<T>(r + o, rv);
      st16<T>(upd + o, uv);
      st16<T>(x + o, xv);
    }
    done = nc * W;
  }
  for (size_t i = done + tid; i < n; i += stride) {
    T xi = x[i], ui = upd[i], ri = r[i];
    cheb_update_elem<T>(xi, ui, ri, t[i], dinv[i], f1, f2);
    r[i] = ri;
    upd[i] = ui;
    x[i] = xi;
  }
}

// (T) f for a double f that is the same on every lane, in scalar registers, where a kernel argument lives: with the
// scalars in vector registers the optimiser pairs and contracts the products of cheb_update_elem differently (a packed
// multiply and a fused multiply-add in the float tail), which changes the last bit of upd and x
template <typename T>
__device__ __forceinline__ T uniform_scalar(double f) {
  if constexpr (sizeof(T) == 8) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(f)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(f));
    return __hiloint2double(hi, lo);
  } else {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int((float)f)));
  }
}

// The two kernels above with the scalars in device memory: f_dev holds doubles, every thread reads them and rounds them
// to T as the by-value entry points round theirs on the host (round to nearest even), then runs the same loop.  The
// bodies are copies, not calls, for the reason given at cheb_update_kernel: the by-value kernels keep their code, and
// tests/test_gpu_refresh.py holds the two forms to equal bits.
template <typename T, bool VEC, bool HAS_T, bool ZERO>
__global__ void __launch_bounds__(256)
cheb_start_dev_kernel(T *__restrict__ x, T *__restrict__ upd, T *__restrict__ r, const T *__restrict__ b,
                      const T *__restrict__ t, const T *__restrict__ dinv, const double *__restrict__ f_dev, size_t n) {
  const T f = uniform_scalar<T>(f_dev[0]);
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T xv[W], uv[W], rv[W], bv[W], tv[W], dv[W];
    ldw<W>(b + o, bv);
    if (HAS_T) ldw<W>(t + o, tv);
    ldw<W>(dinv + o, dv);
    if (!ZERO) ldw<W>(x + o, xv);
#pragma unroll
    for (int k = 0; k < W; ++k) cheb_start_elem<T, HAS_T, ZERO>(xv[k], uv[k], rv[k], bv[k], HAS_T ? tv[k] : T(0), dv[k], f);
    stw<W>(r + o, rv);
    stw<W>(upd + o, uv);
    stw<W>(x + o, xv);
  });
}

// cheb_update_elem with the contraction written out instead of left to the optimiser, which decides it differently once
// the scalars come from memory.  What cheb_update_kernel compiles to, and therefore what this states: f1 upd is fused
// into the sum everywhere (FUSE) but in the float tail, where both products are rounded; (f2 r) dinv is two rounded
// products everywhere.
template <typename T, bool FUSE>
__device__ __forceinline__ void cheb_update_elem_dev(T &x, T &u, T &r, T t, T d, T f1, T f2) {
#pragma clang fp contract(off)
  r = r - t;
  const T p = (f2 * r) * d;
  if constexpr (!FUSE)
    u = f1 * u + p;
  else if constexpr (sizeof(T) == 8)
    u = __builtin_fma(f1, u, p);
  else
    u = __builtin_fmaf(f1, u, p);
  x = x + u;
}

template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
cheb_update_dev_kernel(T *__restrict__ x, T *__restrict__ upd, T *__restrict__ r, const T *__restrict__ t,
                       const T *__restrict__ dinv, const double *__restrict__ f12_dev, size_t n) {
  constexpr int W = lanes16<T>();
  const T f1 = uniform_scalar<T>(f12_dev[0]), f2 = uniform_scalar<T>(f12_dev[1]);
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  size_t done = 0;
  if (VEC) {
    const size_t nc = n / W;
    for (size_t c = tid; c < nc; c += stride) {
      const size_t o = c * W;
      T xv[W], uv[W], rv[W], tv[W], dv[W];
      ld16<T>(r + o, rv);
      ld16<T>(t + o, tv);
      ld16<T>(dinv + o, dv);
      ld16<T>(upd + o, uv);
      ld16<T>(x + o, xv);
#pragma unroll
      for (int k = 0; k < W; ++k) cheb_update_elem_dev<T, true>(xv[k], uv[k], rv[k], tv[k], dv[k], f1, f2);
      st16<T>(r + o, rv);
      st16<T>(upd + o, uv);
      st16<T>(x + o, xv);
    }
    done = nc * W;
  }
  for (size_t i = done + tid; i < n; i += stride) {
    T xi = x[i], ui = upd[i], ri = r[i];
    cheb_update_elem_dev<T, sizeof(T) == 8>(xi, ui, ri, t[i], dinv[i], f1, f2);
    r[i] = ri;
    upd[i] = ui;
    x[i] = xi;
  }
}

// t = b - t (HAS_E: t = b - (t + e)): the V-cycle's residual after t = A x, the edge rows e = down x included -- the
// operations and their order of t.add(1, e), t.sadd(-1, 1, b)
template <typename T, bool VEC, bool HAS_E>
__global__ void __launch_bounds__(256)
residual_kernel(T *__restrict__ t, const T *__restrict__ b, const T *__restrict__ e, size_t n) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T tv[W], bv[W], ev[W];
    ldw<W>(t + o, tv);
    ldw<W>(b + o, bv);
    if (HAS_E) ldw<W>(e + o, ev);
#pragma unroll
    for (int k = 0; k < W; ++k) tv[k] = HAS_E ? bv[k] - (tv[k] + ev[k]) : bv[k] - tv[k];
    stw<W>(t + o, tv);
  });
}

template <typename D, typename S>
void convert_launch(D *dst, const S *src, size_t n, hipStream_t st) {
  const bool vec = aligned16(dst) && aligned16(src);
  dispatch([&](auto VEC) {
    hipLaunchKernelGGL((convert_kernel<D, S, VEC()>), dim3(stream_grid(n, 4, vec)), dim3(256), 0, st, dst, src, n);
  }, vec);
}

template <typename T>
void cheb_start_launch(T *x, T *upd, T *r, const T *b, const T *t, const T *dinv, T f, bool zero, size_t n,
                       hipStream_t st) {
  const bool vec = aligned16(x) && aligned16(upd) && aligned16(r) && aligned16(b) && aligned16(t) && aligned16(dinv);
  dispatch([&](auto VEC, auto HAS_T, auto ZERO) {
    hipLaunchKernelGGL((cheb_start_kernel<T, VEC(), HAS_T(), ZERO()>), dim3(stream_grid(n, lanes16<T>(), vec)),
                       dim3(256), 0, st, x, upd, r, b, t, dinv, f, n);
  }, vec, t != nullptr, zero);
}

template <typename T>
void cheb_update_launch(T *x, T *upd, T *r, const T *t, const T *dinv, T f1, T f2, size_t n, hipStream_t st) {
  const bool vec = aligned16(x) && aligned16(upd) && aligned16(r) && aligned16(t) && aligned16(dinv);
  dispatch([&](auto VEC) {
    hipLaunchKernelGGL((cheb_update_kernel<T, VEC()>), dim3(stream_grid(n, lanes16<T>(), vec)), dim3(256), 0, st, x,
                       upd, r, t, dinv, f1, f2, n);
  }, vec);
}

template <typename T>
void cheb_start_dev_launch(T *x, T *upd, T *r, const T *b, const T *t, const T *dinv, const double *f_dev, bool zero,
                           size_t n, hipStream_t st) {
  const bool vec = aligned16(x) && aligned16(upd) && aligned16(r) && aligned16(b) && aligned16(t) && aligned16(dinv);
  dispatch([&](auto VEC, auto HAS_T, auto ZERO) {
    hipLaunchKernelGGL((cheb_start_dev_kernel<T, VEC(), HAS_T(), ZERO()>), dim3(stream_grid(n, lanes16<T>(), vec)),
                       dim3(256), 0, st, x, upd, r, b, t, dinv, f_dev, n);
  }, vec, t != nullptr, zero);
}

template <typename T>
void cheb_update_dev_launch(T *x, T *upd, T *r, const T *t, const T *dinv, const double *f12_dev, size_t n,
                            hipStream_t st) {
  const bool vec = aligned16(x) && aligned16(upd) && aligned16(r) && aligned16(t) && aligned16(dinv);
  dispatch([&](auto VEC) {
    hipLaunchKernelGGL((cheb_update_dev_kernel<T, VEC()>), dim3(stream_grid(n, lanes16<T>(), vec)), dim3(256), 0, st, x,
                       upd, r, t, dinv, f12_dev, n);
  }, vec);
}

template <typename T>
void residual_launch(T *t, const T *b, const T *e, size_t n, hipStream_t st) {
  const bool vec = aligned16(t) && aligned16(b) && aligned16(e);
  dispatch([&](auto VEC, auto HAS_E) {
    hipLaunchKernelGGL((residual_kernel<T, VEC(), HAS_E()>), dim3(stream_grid(n, lanes16<T>(), vec)), dim3(256), 0, st,
                       t, b, e, n);
  }, vec, e != nullptr);
}

// the three written vectors must be distinct and must not be one of the read ones
bool outputs_alias(const void *x, const void *upd, const void *r, const void *a, const void *b, const void *c) {
  const void *out[3] = {x, upd, r}, *in[3] = {a, b, c};
  for (int i = 0; i < 3; ++i) {
    for (int j = i + 1; j < 3; ++j)
      if (out[i] == out[j]) return true;
    for (int j = 0; j < 3; ++j)
      if (in[j] && out[i] == in[j]) return true;
  }
  return false;
}

}  // namespace

extern "C" {

int mfgpu_vec_convert(void *dst, int dst_type, const void *src, int src_type, size_t n, void *stream) {
  if (!mfgpu::valid_number_type(dst_type) || !mfgpu::valid_number_type(src_type)) return einval("mfgpu_vec_convert: number type must be MFGPU_F64 or MFGPU_F32");
  if (n == 0) return MFGPU_OK;
  if (!dst || !src) return einval("mfgpu_vec_convert: null vector");
  const hipStream_t st = (hipStream_t)stream;
  if (dst_type == src_type) {
    if (dst == src) return MFGPU_OK;
    return mfgpu::hip_check(hipMemcpyAsync(dst, src, n * mfgpu::esize(dst_type), hipMemcpyDeviceToDevice, st),
                            "mfgpu_vec_convert");
  }
  if (dst == src) return einval("mfgpu_vec_convert: dst and src must not alias");
  if (dst_type == MFGPU_F32)
    convert_launch<float, double>((float *)dst, (const double *)src, n, st);
  else
    convert_launch<double, float>((double *)dst, (const float *)src, n, st);
  return mfgpu::hip_check(hipGetLastError(), "mfgpu_vec_convert");
}

int mfgpu_vec_residual(void *t, const void *b, const void *e, size_t n, int number_type, void *stream) {
  if (!mfgpu::valid_number_type(number_type)) return einval("mfgpu_vec_residual: number type must be MFGPU_F64 or MFGPU_F32");
  if (n == 0) return MFGPU_OK;
  if (!t || !b) return einval("mfgpu_vec_residual: null vector");
  const uintptr_t bytes = n * mfgpu::esize(number_type), t0 = (uintptr_t)t;
  for (const void *in : {b, e}) {  // ranges, as mfgpu_cg_begin: the kernel reads b and e through __restrict__ pointers
    const uintptr_t i0 = (uintptr_t)in;
    if (in && t0 < i0 + bytes && i0 < t0 + bytes) return einval("mfgpu_vec_residual: t must not overlap b or e");
  }
  const hipStream_t st = (hipStream_t)stream;
  if (number_type == MFGPU_F64)
    residual_launch<double>((double *)t, (const double *)b, (const double *)e, n, st);
  else
    residual_launch<float>((float *)t, (const float *)b, (const float *)e, n, st);
  return mfgpu::hip_check(hipGetLastError(), "mfgpu_vec_residual");
}

int mfgpu_vec_chebyshev_start(void *x, void *upd, void *r, const void *b, const void *t, const void *dinv, double f,
                              int zero_start, size_t n, int number_type, void *stream) {
  if (!mfgpu::valid_number_type(number_type)) return einval("mfgpu_vec_chebyshev_start: number type must be MFGPU_F64 or MFGPU_F32");
  if (n == 0) return MFGPU_OK;
  if (!x || !upd || !r || !b || !dinv) return einval("mfgpu_vec_chebyshev_start: null vector");
  if (outputs_alias(x, upd, r, b, t, dinv)) return einval("mfgpu_vec_chebyshev_start: x, upd and r must not alias each other or an input");
  const hipStream_t st = (hipStream_t)stream;
  if (number_type == MFGPU_F64)
    cheb_start_launch<double>((double *)x, (double *)upd, (double *)r, (const double *)b, (const double *)t,
                              (const double *)dinv, f, zero_start != 0, n, st);
  else
    cheb_start_launch<float>((float *)x, (float *)upd, (float *)r, (const float *)b, (const float *)t,
                             (const float *)dinv, (float)f, zero_start != 0, n, st);
  return mfgpu::hip_check(hipGetLastError(), "mfgpu_vec_chebyshev_start");
}

int mfgpu_vec_chebyshev_update(void *x, void *upd, void *r, const void *t, const void *dinv, double f1, double f2,
                               size_t n, int number_type, void *stream) {
  if (!mfgpu::valid_number_type(number_type)) return einval("mfgpu_vec_chebyshev_update: number type must be MFGPU_F64 or MFGPU_F32");
  if (n == 0) return MFGPU_OK;
  if (!x || !upd || !r || !t || !dinv) return einval("mfgpu_vec_chebyshev_update: null vector");
  if (outputs_alias(x, upd, r, t, dinv, nullptr)) return einval("mfgpu_vec_chebyshev_update: x, upd and r must not alias each other or an input");
  const hipStream_t st = (hipStream_t)stream;
  if (number_type == MFGPU_F64)
    cheb_update_launch<double>((double *)x, (double *)upd, (double *)r, (const double *)t, (const double *)dinv, f1, f2,
                               n, st);
  else
    cheb_update_launch<float>((float *)x, (float *)upd, (float *)r, (const float *)t, (const float *)dinv, (float)f1,
                              (float)f2, n, st);
  return mfgpu::hip_check(hipGetLastError(), "mfgpu_vec_chebyshev_update");
}

int mfgpu_vec_chebyshev_start_dev(void *x, void *upd, void *r, const void *b, const void *t, const void *dinv,
                                  const double *f_dev, int zero_start, size_t n, int number_type, void *stream) {
  if (!mfgpu::valid_number_type(number_type)) return einval("mfgpu_vec_chebyshev_start_dev: number type must be MFGPU_F64 or MFGPU_F32");
  if (!f_dev || ((uintptr_t)f_dev & 7u)) return einval("mfgpu_vec_chebyshev_start_dev: f_dev must be a device address of doubles");
  if (n == 0) return MFGPU_OK;
  if (!x || !upd || !r || !b || !dinv) return einval("mfgpu_vec_chebyshev_start_dev: null vector");
  if (outputs_alias(x, upd, r, b, t, dinv)) return einval("mfgpu_vec_chebyshev_start_dev: x, upd and r must not alias each other or an input");
  const hipStream_t st = (hipStream_t)stream;
  if (number_type == MFGPU_F64)
    cheb_start_dev_launch<double>((double *)x, (double *)upd, (double *)r, (const double *)b, (const double *)t,
                                  (const double *)dinv, f_dev, zero_start != 0, n, st);
  else
    cheb_start_dev_launch<float>((float *)x, (float *)upd, (float *)r, (const float *)b, (const float *)t,
                                 (const float *)dinv, f_dev, zero_start != 0, n, st);
  return mfgpu::hip_check(hipGetLastError(), "mfgpu_vec_chebyshev_start_dev");
}

int mfgpu_vec_chebyshev_update_dev(void *x, void *upd, void *r, const void *t, const void *dinv, const double *f12_dev,
                                   size_t n, int number_type, void *stream) {
  if (!mfgpu::valid_number_type(number_type)) return einval("mfgpu_vec_chebyshev_update_dev: number type must be MFGPU_F64 or MFGPU_F32");
  if (!f12_dev || ((uintptr_t)f12_dev & 7u)) return einval("mfgpu_vec_chebyshev_update_dev: f12_dev must be a device address of doubles");
  if (n == 0) return MFGPU_OK;
  if (!x || !upd || !r || !t || !dinv) return einval("mfgpu_vec_chebyshev_update_dev: null vector");
  if (outputs_alias(x, upd, r, t, dinv, nullptr)) return einval("mfgpu_vec_chebyshev_update_dev: x, upd and r must not alias each other or an input");
  const hipStream_t st = (hipStream_t)stream;
  if (number_type == MFGPU_F64)
    cheb_update_dev_launch<double>((double *)x, (double *)upd, (double *)r, (const double *)t, (const double *)dinv,
                                   f12_dev, n, st);
  else
    cheb_update_dev_launch<float>((float *)x, (float *)upd, (float *)r, (const float *)t, (const float *)dinv, f12_dev, n,
                                  st);
  return mfgpu::hip_check(hipGetLastError(), "mfgpu_vec_chebyshev_update_dev");
}

}  // extern "C"
