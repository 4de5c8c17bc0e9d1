// Device-resident BiCGStab: SolverBicgstab::solve of host/mfgpu_shim_qop.h -- right-preconditioned, zero
// start, r0 = b, a half-step exit on |s| <= tolerance after x += alpha y, a full-step exit on |r| <= tolerance -- with
// every scalar kept in a device state block, so that begin / iterate only enqueue work (no allocation, no synchronisation,
// no host read-back) and can be captured in a graph.  The operator is a callback (a handle's mfgpu_vmult, a
// mfgpu_qop_vmult or the caller's function), so the non-symmetric operators of mfgpu_qop are solved here.
//   bicg_init_kernel       begin: x = 0, r = r0 = b, partial sums of r.r (= r0.r); resets the state
//   bicg_direction_kernel  (1) sums the r.r / r0.r partials; count, residual, status; beta = (rho_new / rho)(alpha / omega);
//                              p = r + beta (p - omega v) (first launch: p = r); JACOBI: y = dinv p
//   bicg_dot_kernel        (2) partial sums of r0.v after v = A y
//   bicg_half_kernel       (3) alpha = rho / (r0.v); x += alpha y, r -= alpha v (s lives in r); partial sums of s.s;
//                              JACOBI: z = dinv s
//   bicg_dot2_kernel       (4) partial sums of t.s and t.t in one pass after t = A z
//   bicg_full_kernel       (5) sums s.s: |s| <= tolerance is the half-step exit, recorded as a flag, nothing else written;
//                              else omega = t.s / t.t, x += omega z, r -= omega t, partial sums of r.r and r0.r
// y and z are p and r themselves for NONE, vectors for JACOBI (written by (1) and (3)) and CALLBACK (y = M^-1 p and
// z = M^-1 s by the callback, after (1) and (3)).
// Streaming kernels on the skeleton of mfgpu_stream.h, under the rules of mfgpu_cg.hip: double accumulation in a fixed
// order, one partial per block, EVERY block of the consuming kernel re-sums the <= kStreamBlocks partials (resum), so all
// blocks hold the same bits of alpha, omega and beta; the scalars are rounded to T before any element-wise use.  No
// atomics, no counters, no grid barrier.
// State block rule: no kernel reads a field that the same kernel writes.  Four groups:
//   begin      written by bicg_init_kernel (which reads none and also resets count and status)
//   direction  written by (1), which reads begin, half and full
//   half       written by (3), which reads direction
//   full       written by (5), which reads begin, direction (the tolerance only) and half
// (2) and (4) read the status and write no field.  What a kernel reads was written by an earlier launch and is uniform
// over its grid, which makes every early return uniform per block.  tolerance_abs (begin_relative) is a direction field
// that the FIRST launch of (1) writes without reading and the later launches read without writing, as in mfgpu_cg.hip.
// The half-step exit needs no host visit: (3) has already moved x and r when |s| is known, which is what the host loop
// does at that exit; (5) sees |s| <= tolerance, sets F_HALF_EXIT in its own group and moves nothing; the next (1) turns
// the flag into status 1 with residual |s| and the count of that iteration.  The A z and (4) in between write t and
// partials only.  Breakdown (r0.v or t.t zero or not finite: flags of (3) and (5); rho: seen by (1) itself) ends with
// status 3 and x at the last complete update.  Once the status has left 0, (2) and (4) return at once, (3) sets F_FROZEN,
// (5) passes it on and (1) returns on it: no vector and no direction field is written again.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>

#include "mfgpu_device.h"
#include "mfgpu_stream.h"

using namespace mfgpu;

namespace {

enum : uint32_t { F_FROZEN = 1u, F_BREAKDOWN = 2u, F_HALF_EXIT = 4u };

struct BicgState {
  // begin: written by bicg_init_kernel
  double tolerance;  // begin_relative: the relative tolerance, see tolerance_abs
  uint32_t max_iterations, relative;
  // direction: written by bicg_direction_kernel (status and iterations also reset by bicg_init_kernel)
  double rho, rr, beta, initial_residual;
  double tolerance_abs;  // begin_relative only: written by the first launch of a solve, read by the later ones
  uint32_t iterations, status;
  // half: written by bicg_half_kernel
  double r0v, alpha, rho_h;  // rho_h, it_h: the direction fields handed on, so that (1) does not read what it writes
  uint32_t it_h, flags_h;
  // full: written by bicg_full_kernel
  double ss, tt, omega;
  uint32_t flags_f, pad;
};
static_assert(sizeof(BicgState) == 128, "the state block is 128 bytes (mfgpu_bicgstab_memory_consumption, include/mfgpu.h)");

enum Prec { P_NONE = 0, P_JACOBI = 1, P_STORED = 2 };  // P_STORED: y and z come from the callback
enum { PART_RR, PART_R0R, PART_R0V, PART_SS, PART_TS, PART_TT, N_PARTIALS };

__device__ __forceinline__ bool usable(double d) { return d != 0.0 && fabs(d) < INFINITY; }  // false for NaN

// begin: x = 0, r = r0 = b; partials of r.r
template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
bicg_init_kernel(BicgState *__restrict__ s, T *__restrict__ x, T *__restrict__ r, T *__restrict__ r0,
                 const T *__restrict__ b, double *__restrict__ prr, double tolerance, uint32_t relative,
                 uint32_t max_iterations, size_t n) {
  __shared__ double red[4];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  double arr = 0.0;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T bv[W], zero[W];
    ldw<W>(b + o, bv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      zero[k] = T(0);
      arr += (double)bv[k] * (double)bv[k];
    }
    stw<W>(x + o, zero);
    stw<W>(r + o, bv);
    stw<W>(r0 + o, bv);
  });
  arr = block_sum<false>(arr, red);
  if (threadIdx.x == 0) {
    prr[blockIdx.x] = arr;
    if (blockIdx.x == 0) {
      s->tolerance = tolerance;
      s->relative = relative;
      s->max_iterations = max_iterations;
      s->iterations = 0;
      s->status = 0;
    }
  }
}

// (1): r.r and r0.r from the partials (first launch: r0 = r, one sum); count, residual, status; beta; p = r + beta (p -
// omega v), first launch p = r; JACOBI: y = dinv p.  p is left alone once the solve has ended.
template <typename T, bool VEC, int PREC>
__global__ void __launch_bounds__(256)
bicg_direction_kernel(BicgState *__restrict__ s, T *__restrict__ p, T *__restrict__ y, const T *__restrict__ r,
                      const T *__restrict__ v, const T *__restrict__ dinv, const double *__restrict__ prr,
                      const double *__restrict__ pr0r, unsigned np, int first, size_t n) {
  __shared__ double red[4];
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  const bool is_first = first != 0;  // a local: the parameter itself, captured by reference, changes the code below
  uint32_t it = 0;
  if (!is_first) {
    const uint32_t flags = s->flags_f;
    if (flags & F_FROZEN) return;
    if (flags & F_BREAKDOWN) {  // r0.v or t.t was not usable: (3) resp. (5) wrote no vector
      if (writer) s->status = 3;
      return;
    }
    it = s->it_h + 1u;
    if (flags & F_HALF_EXIT) {  // |s| <= tolerance: (3) has moved x and r, (5) nothing
      if (writer) {
        s->rr = s->ss;
        s->iterations = it;
        s->status = 1;
      }
      return;
    }
  }
  const double rr = resum(prr, np, red);
  const double rho_new = is_first ? rr : resum(pr0r, np, red);
  const double res = sqrt(rr);
  // relative: the first launch forms the absolute tolerance from the start residual, the later ones read it back
  const bool relative = s->relative != 0;
  const double tolerance = !relative ? s->tolerance : is_first ? s->tolerance * res : s->tolerance_abs;
  const uint32_t status = res <= tolerance ? 1u : it >= s->max_iterations ? 2u : !usable(rho_new) ? 3u : 0u;
  const double omega_d = is_first ? 1.0 : s->omega;
  const double beta_d = is_first ? 0.0 : (rho_new / s->rho_h) * (s->alpha / omega_d);
  const T beta = (T)beta_d, omega = (T)omega_d;
  if (writer) {
    s->rr = rr;
    s->rho = rho_new;
    s->beta = beta_d;
    s->iterations = it;
    s->status = status;
    if (is_first) s->initial_residual = res;
    if (is_first && relative) s->tolerance_abs = tolerance;
  }
  if (status != 0) return;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T pv[W], rv[W], vv[W], dv[W];
    ldw<W>(r + o, rv);
    if (is_first) {
#pragma unroll
      for (int k = 0; k < W; ++k) pv[k] = rv[k];
    } else {
      ldw<W>(p + o, pv);
      ldw<W>(v + o, vv);
#pragma unroll
      for (int k = 0; k < W; ++k) pv[k] = rv[k] + beta * (pv[k] - omega * vv[k]);
    }
    stw<W>(p + o, pv);
    if (PREC == P_JACOBI) {
      ldw<W>(dinv + o, dv);
#pragma unroll
      for (int k = 0; k < W; ++k) dv[k] = dv[k] * pv[k];
      stw<W>(y + o, dv);
    }
  });
}

// (2): partials of a.b; nothing once the solve has ended
template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
bicg_dot_kernel(const BicgState *__restrict__ s, double *__restrict__ partial, const T *__restrict__ a,
                const T *__restrict__ b, size_t n) {
  __shared__ double red[4];
  if (s->status != 0) return;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T av[W], bv[W];
    ldw<W>(a + o, av);
    ldw<W>(b + o, bv);
#pragma unroll
    for (int k = 0; k < W; ++k) acc += (double)av[k] * (double)bv[k];
  });
  acc = block_sum<false>(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// (4): partials of t.s and t.t in one pass; nothing once the solve has ended
template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
bicg_dot2_kernel(const BicgState *__restrict__ s, double *__restrict__ pts, double *__restrict__ ptt,
                 const T *__restrict__ t, const T *__restrict__ sv, size_t n) {
  __shared__ double red[4];
  if (s->status != 0) return;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  double ats = 0.0, att = 0.0;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T tv[W], rv[W];
    ldw<W>(t + o, tv);
    ldw<W>(sv + o, rv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      ats += (double)tv[k] * (double)rv[k];
      att += (double)tv[k] * (double)tv[k];
    }
  });
  ats = block_sum(ats, red);
  att = block_sum<false>(att, red);
  if (threadIdx.x == 0) {
    pts[blockIdx.x] = ats;
    ptt[blockIdx.x] = att;
  }
}

// (3): alpha = rho / (r0.v) from the partials of (2); x += alpha y; r -= alpha v; partials of s.s; JACOBI: z = dinv s
template <typename T, bool VEC, int PREC>
__global__ void __launch_bounds__(256)
bicg_half_kernel(BicgState *__restrict__ s, T *__restrict__ x, T *__restrict__ r, T *__restrict__ z,
                 const T *__restrict__ y, const T *__restrict__ v, const T *__restrict__ dinv,
                 const double *__restrict__ pr0v, double *__restrict__ pss, unsigned np, size_t n) {
  __shared__ double red[4];
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (s->status != 0) {  // frozen: tell (5) and through it (1), write nothing else
    if (writer) s->flags_h = F_FROZEN;
    return;
  }
  const double r0v = resum(pr0v, np, red), rho = s->rho;
  const bool ok = usable(r0v);
  const double alpha_d = rho / r0v;
  const T alpha = (T)alpha_d;
  if (writer) {
    s->flags_h = ok ? 0u : F_BREAKDOWN;
    s->r0v = r0v;
    s->alpha = alpha_d;
    s->rho_h = rho;
    s->it_h = s->iterations;
  }
  if (!ok) return;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  double ass = 0.0;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T xv[W], rv[W], yv[W], vv[W], dv[W];
    ldw<W>(x + o, xv);
    ldw<W>(r + o, rv);
    ldw<W>(y + o, yv);
    ldw<W>(v + o, vv);
    if (PREC == P_JACOBI) ldw<W>(dinv + o, dv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      xv[k] = xv[k] + alpha * yv[k];
      rv[k] = rv[k] - alpha * vv[k];
      ass += (double)rv[k] * (double)rv[k];
      if (PREC == P_JACOBI) dv[k] = dv[k] * rv[k];
    }
    stw<W>(x + o, xv);
    stw<W>(r + o, rv);
    if (PREC == P_JACOBI) stw<W>(z + o, dv);
  });
  ass = block_sum<false>(ass, red);
  if (threadIdx.x == 0) pss[blockIdx.x] = ass;
}

// (5): s.s from the partials of (3): the half-step exit; else omega = t.s / t.t from the partials of (4); x += omega z;
// r -= omega t; partials of r.r and r0.r.  NONE: z is s, the r this kernel reads.
template <typename T, bool VEC, int PREC>
__global__ void __launch_bounds__(256)
bicg_full_kernel(BicgState *__restrict__ s, T *__restrict__ x, T *__restrict__ r, const T *__restrict__ z,
                 const T *__restrict__ t, const T *__restrict__ r0, const double *__restrict__ pss,
                 const double *__restrict__ pts, const double *__restrict__ ptt, double *__restrict__ prr,
                 double *__restrict__ pr0r, unsigned np, size_t n) {
  __shared__ double red[4];
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  const uint32_t flags_h = s->flags_h;
  if (flags_h != 0) {  // frozen, or r0.v not usable: handed on to (1)
    if (writer) s->flags_f = flags_h;
    return;
  }
  const double ss = resum(pss, np, red);
  const double tolerance = s->relative != 0 ? s->tolerance_abs : s->tolerance;
  const bool half_exit = sqrt(ss) <= tolerance;
  const double ts = resum(pts, np, red), tt = resum(ptt, np, red);
  const bool ok = usable(tt);
  const double omega_d = ts / tt;
  const T omega = (T)omega_d;
  if (writer) {
    s->flags_f = half_exit ? F_HALF_EXIT : ok ? 0u : F_BREAKDOWN;
    s->ss = ss;
    s->tt = tt;
    s->omega = omega_d;
  }
  if (half_exit || !ok) return;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  double arr = 0.0, ar0r = 0.0;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T xv[W], rv[W], zv[W], tv[W], qv[W];
    ldw<W>(x + o, xv);
    ldw<W>(r + o, rv);
    if (PREC != P_NONE) ldw<W>(z + o, zv);
    ldw<W>(t + o, tv);
    ldw<W>(r0 + o, qv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      xv[k] = xv[k] + omega * (PREC != P_NONE ? zv[k] : rv[k]);
      rv[k] = rv[k] - omega * tv[k];
      arr += (double)rv[k] * (double)rv[k];
      ar0r += (double)qv[k] * (double)rv[k];
    }
    stw<W>(x + o, xv);
    stw<W>(r + o, rv);
  });
  arr = block_sum(arr, red);
  ar0r = block_sum<false>(ar0r, red);
  if (threadIdx.x == 0) {
    prr[blockIdx.x] = arr;
    pr0r[blockIdx.x] = ar0r;
  }
}

}  // namespace

struct mfgpu_bicgstab {
  int prec = MFGPU_CG_NONE, number_type = MFGPU_F64;
  size_t n = 0;
  const void *dinv = nullptr;
  mfgpu::DeviceArray<void> r, r0, p, v, t, y, z;  // y, z: JACOBI and CALLBACK only
  mfgpu::DeviceArray<double> partials;            // N_PARTIALS x kStreamBlocks
  mfgpu::DeviceArray<BicgState> state;
  BicgState *mirror = nullptr;  // pinned
  // the operator: dst = A src
  int (*apply)(void *, void *, const void *, void *) = nullptr;
  void *apply_ctx = nullptr;
  mfgpu_handle *handle = nullptr;  // set_operator_handle
  mfgpu_qop *qop = nullptr;        // set_operator_qop
  uint32_t qop_flags = 0;
  // the preconditioner callback: z = M^-1 r
  int (*fn)(void *, void *, const void *, void *) = nullptr;
  void *ctx = nullptr;
  // the solve in progress
  void *x = nullptr;
  const void *b = nullptr;
  bool begun = false, vec = false;
  unsigned grid = 1;
  size_t device_bytes = 0;
  ~mfgpu_bicgstab() {
    if (mirror) hipHostFree(mirror);
  }
};

namespace {

int kernel_prec(const mfgpu_bicgstab *s) {
  return s->prec == MFGPU_CG_NONE ? P_NONE : s->prec == MFGPU_CG_JACOBI ? P_JACOBI : P_STORED;
}
double *partial(const mfgpu_bicgstab *s, int which) { return s->partials.get() + (size_t)which * kStreamBlocks; }
// y = M^-1 p and z = M^-1 s: p and r themselves without a preconditioner
void *y_of(const mfgpu_bicgstab *s) { return s->prec == MFGPU_CG_NONE ? s->p.get() : s->y.get(); }
void *z_of(const mfgpu_bicgstab *s) { return s->prec == MFGPU_CG_NONE ? s->r.get() : s->z.get(); }

template <typename F>
void with_vec_prec(const mfgpu_bicgstab *s, F &&f) {
  static_assert(P_NONE == 0 && P_JACOBI == 1 && P_STORED == 2, "OneOf3 carries the Prec");
  dispatch(f, s->vec, OneOf3{kernel_prec(s)});
}

int handle_apply(void *ctx, void *dst, const void *src, void *stream) {
  return mfgpu_vmult(static_cast<mfgpu_bicgstab *>(ctx)->handle, dst, src, stream);
}
int qop_apply(void *ctx, void *dst, const void *src, void *stream) {
  mfgpu_bicgstab *s = static_cast<mfgpu_bicgstab *>(ctx);
  return mfgpu_qop_vmult(s->qop, dst, src, s->qop_flags, stream);
}
int vqop_apply(void *ctx, void *dst, const void *src, void *stream) {
  return mfgpu_vqop_vmult(static_cast<mfgpu_vqop *>(ctx), dst, src, stream);
}
int vcycle_callback(void *ctx, void *z_dev, const void *r_dev, void *stream) {
  return mfgpu_vcycle_apply(static_cast<mfgpu_vcycle *>(ctx), z_dev, r_dev, stream);
}

int apply_operator(mfgpu_bicgstab *s, void *dst, const void *src, hipStream_t st) {
  const int rc = s->apply(s->apply_ctx, dst, src, (void *)st);
  if (rc && s->apply != handle_apply && s->apply != qop_apply && s->apply != vqop_apply) mfgpu::set_error("mfgpu_bicgstab: the operator callback failed");
  return rc;
}
int precondition(mfgpu_bicgstab *s, void *dst, const void *src, hipStream_t st) {
  if (s->prec != MFGPU_CG_CALLBACK) return 0;
  const int rc = s->fn(s->ctx, dst, src, (void *)st);
  if (rc && s->fn != vcycle_callback) mfgpu::set_error("mfgpu_bicgstab: the preconditioner callback failed");
  return rc;
}

template <typename T>
int direction_launch(mfgpu_bicgstab *s, int first, hipStream_t st) {
  with_vec_prec(s, [&](auto VEC, auto PREC) {
    hipLaunchKernelGGL((bicg_direction_kernel<T, VEC(), PREC()>), dim3(s->grid), dim3(256), 0, st, s->state.get(),
                       (T *)s->p.get(), (T *)s->y.get(), (const T *)s->r.get(), (const T *)s->v.get(),
                       (const T *)s->dinv, (const double *)partial(s, PART_RR), (const double *)partial(s, PART_R0R),
                       s->grid, first, s->n);
  });
  if (const int rc = mfgpu::hip_check(hipGetLastError(), "mfgpu_bicgstab: direction update")) return rc;
  return precondition(s, s->y.get(), s->p.get(), st);
}

template <typename T>
int begin_typed(mfgpu_bicgstab *s, double tolerance, uint32_t relative, uint32_t max_iterations, hipStream_t st) {
  dispatch([&](auto VEC) {
    hipLaunchKernelGGL((bicg_init_kernel<T, VEC()>), dim3(s->grid), dim3(256), 0, st, s->state.get(), (T *)s->x,
                       (T *)s->r.get(), (T *)s->r0.get(), (const T *)s->b, partial(s, PART_RR), tolerance, relative,
                       max_iterations, s->n);
  }, s->vec);
  if (const int rc = mfgpu::hip_check(hipGetLastError(), "mfgpu_bicgstab_begin")) return rc;
  return direction_launch<T>(s, 1, st);
}

template <typename T>
int iterate_typed(mfgpu_bicgstab *s, uint32_t n_iterations, hipStream_t st) {
  BicgState *state = s->state.get();
  const T *r = (const T *)s->r.get(), *r0 = (const T *)s->r0.get(), *v = (const T *)s->v.get(), *t = (const T *)s->t.get();
  for (uint32_t it = 0; it < n_iterations; ++it) {
    if (const int rc = apply_operator(s, s->v.get(), y_of(s), st)) return rc;
    dispatch([&](auto VEC) {
      hipLaunchKernelGGL((bicg_dot_kernel<T, VEC()>), dim3(s->grid), dim3(256), 0, st, (const BicgState *)state,
                         partial(s, PART_R0V), r0, v, s->n);
    }, s->vec);
    with_vec_prec(s, [&](auto VEC, auto PREC) {
      hipLaunchKernelGGL((bicg_half_kernel<T, VEC(), PREC()>), dim3(s->grid), dim3(256), 0, st, state, (T *)s->x,
                         (T *)s->r.get(), (T *)s->z.get(), (const T *)y_of(s), v, (const T *)s->dinv,
                         (const double *)partial(s, PART_R0V), partial(s, PART_SS), s->grid, s->n);
    });
    if (const int rc = mfgpu::hip_check(hipGetLastError(), "mfgpu_bicgstab_iterate")) return rc;
    if (const int rc = precondition(s, s->z.get(), s->r.get(), st)) return rc;
    if (const int rc = apply_operator(s, s->t.get(), z_of(s), st)) return rc;
    dispatch([&](auto VEC) {
      hipLaunchKernelGGL((bicg_dot2_kernel<T, VEC()>), dim3(s->grid), dim3(256), 0, st, (const BicgState *)state,
                         partial(s, PART_TS), partial(s, PART_TT), t, r, s->n);
    }, s->vec);
    with_vec_prec(s, [&](auto VEC, auto PREC) {
      hipLaunchKernelGGL((bicg_full_kernel<T, VEC(), PREC()>), dim3(s->grid), dim3(256), 0, st, state, (T *)s->x,
                         (T *)s->r.get(), (const T *)s->z.get(), t, r0, (const double *)partial(s, PART_SS),
                         (const double *)partial(s, PART_TS), (const double *)partial(s, PART_TT), partial(s, PART_RR),
                         partial(s, PART_R0R), s->grid, s->n);
    });
    if (const int rc = mfgpu::hip_check(hipGetLastError(), "mfgpu_bicgstab_iterate")) return rc;
    if (const int rc = direction_launch<T>(s, 0, st)) return rc;
  }
  return 0;
}

int begin_common(mfgpu_bicgstab *s, void *x_dev, const void *b_dev, double tolerance, uint32_t relative,
                 uint32_t max_iterations, void *stream) {
  if (!s || !x_dev || !b_dev) return einval("mfgpu_bicgstab_begin: null argument");
  if (!s->apply) return einval("mfgpu_bicgstab_begin: no operator set (mfgpu_bicgstab_set_operator*)");
  if (s->prec == MFGPU_CG_CALLBACK && !s->fn) return einval("mfgpu_bicgstab_begin: no callback set (mfgpu_bicgstab_set_callback)");
  const size_t vbytes = s->n * mfgpu::esize(s->number_type);
  const uintptr_t x0 = (uintptr_t)x_dev, b0 = (uintptr_t)b_dev;
  if (x0 < b0 + vbytes && b0 < x0 + vbytes) return einval("mfgpu_bicgstab_begin: x and b must not overlap");
  s->x = x_dev;
  s->b = b_dev;
  s->vec = aligned16(x_dev) && aligned16(b_dev) && aligned16(s->dinv);
  s->grid = stream_grid(s->n, 16 / mfgpu::esize(s->number_type), s->vec);
  s->begun = true;
  return s->number_type == MFGPU_F64 ? begin_typed<double>(s, tolerance, relative, max_iterations, (hipStream_t)stream)
                                     : begin_typed<float>(s, tolerance, relative, max_iterations, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int mfgpu_bicgstab_create(size_t n_dofs, int number_type, int preconditioner, const void *inv_diag_dev,
                          mfgpu_bicgstab **out) {
  if (!out) return einval("mfgpu_bicgstab_create: null argument");
  if (n_dofs == 0) return einval("mfgpu_bicgstab_create: n_dofs must be positive");
  if (!mfgpu::valid_number_type(number_type)) return einval("mfgpu_bicgstab_create: unknown number type");
  if (preconditioner != MFGPU_CG_NONE && preconditioner != MFGPU_CG_JACOBI && preconditioner != MFGPU_CG_CALLBACK)
    return einval("mfgpu_bicgstab_create: the preconditioner is MFGPU_CG_NONE, MFGPU_CG_JACOBI or MFGPU_CG_CALLBACK");
  if (preconditioner == MFGPU_CG_JACOBI && !inv_diag_dev) return einval("mfgpu_bicgstab_create: JACOBI needs inv_diag_dev");
  mfgpu_bicgstab *s = new (std::nothrow) mfgpu_bicgstab;
  if (!s) return MFGPU_ENOMEM;
  s->prec = preconditioner;
  s->number_type = number_type;
  s->n = n_dofs;
  s->dinv = preconditioner == MFGPU_CG_JACOBI ? inv_diag_dev : nullptr;
  const size_t vbytes = s->n * mfgpu::esize(number_type);
  mfgpu::DeviceArray<void> *vectors[7] = {&s->r, &s->r0, &s->p, &s->v, &s->t, &s->y, &s->z};
  const int n_vectors = preconditioner == MFGPU_CG_NONE ? 5 : 7;
  int rc = 0;
  for (int k = 0; k < n_vectors && !rc; ++k) rc = vectors[k]->alloc(vbytes, true);
  if (!rc) rc = s->partials.alloc((size_t)N_PARTIALS * kStreamBlocks, true);
  if (!rc) rc = s->state.alloc(1, true);
  if (!rc) rc = mfgpu::hip_check(hipHostMalloc((void **)&s->mirror, sizeof(BicgState), hipHostMallocDefault), "mfgpu_bicgstab_create");
  if (rc) {
    delete s;
    return rc;
  }
  s->device_bytes = n_vectors * vbytes + s->partials.bytes() + s->state.bytes();
  *out = s;
  return MFGPU_OK;
}

int mfgpu_bicgstab_set_operator(mfgpu_bicgstab *s, int (*apply)(void *ctx, void *dst_dev, const void *src_dev, void *stream),
                                void *ctx) {
  if (!s || !apply) return einval("mfgpu_bicgstab_set_operator: null argument");
  s->apply = apply;
  s->apply_ctx = ctx;
  return MFGPU_OK;
}

int mfgpu_bicgstab_set_operator_handle(mfgpu_bicgstab *s, mfgpu_handle *A) {
  if (!s || !A) return einval("mfgpu_bicgstab_set_operator_handle: null argument");
  if (mfgpu::handle_number_type(A) != s->number_type || mfgpu_n_dofs(A) != s->n)
    return einval("mfgpu_bicgstab_set_operator_handle: the handle's vectors are not the solver's (type or length)");
  s->handle = A;
  s->apply = handle_apply;
  s->apply_ctx = s;
  return MFGPU_OK;
}

int mfgpu_bicgstab_set_operator_qop(mfgpu_bicgstab *s, mfgpu_qop *q, uint32_t flags) {
  if (!s || !q) return einval("mfgpu_bicgstab_set_operator_qop: null argument");
  if (flags & ~(uint32_t)MFGPU_QOP_TRANSPOSE) return einval("mfgpu_bicgstab_set_operator_qop: unknown flag");
  if (s->number_type != MFGPU_F64 || mfgpu::qop_n_dofs(q) != s->n)
    return einval("mfgpu_bicgstab_set_operator_qop: needs an MFGPU_F64 solver of the operator's length");
  s->qop = q;
  s->qop_flags = flags;
  s->apply = qop_apply;
  s->apply_ctx = s;
  return MFGPU_OK;
}

int mfgpu_bicgstab_set_operator_vqop(mfgpu_bicgstab *s, mfgpu_vqop *q) {
  if (!s || !q) return einval("mfgpu_bicgstab_set_operator_vqop: null argument");
  if (s->number_type != MFGPU_F64 || mfgpu::vqop_length(q) != s->n)
    return einval("mfgpu_bicgstab_set_operator_vqop: needs an MFGPU_F64 solver of the operator's length dim * n_dofs");
  s->apply = vqop_apply;
  s->apply_ctx = q;
  return MFGPU_OK;
}

int mfgpu_bicgstab_set_callback(mfgpu_bicgstab *s, int (*fn)(void *ctx, void *z_dev, const void *r_dev, void *stream),
                                void *ctx) {
  if (!s || !fn) return einval("mfgpu_bicgstab_set_callback: null argument");
  if (s->prec != MFGPU_CG_CALLBACK)
    return einval("mfgpu_bicgstab_set_callback: the solver was not created with MFGPU_CG_CALLBACK");
  s->fn = fn;
  s->ctx = ctx;
  return MFGPU_OK;
}

int mfgpu_bicgstab_set_vcycle(mfgpu_bicgstab *s, mfgpu_vcycle *v) {
  if (!s || !v) return einval("mfgpu_bicgstab_set_vcycle: null argument");
  if (s->prec != MFGPU_CG_CALLBACK) return einval("mfgpu_bicgstab_set_vcycle: the solver was not created with MFGPU_CG_CALLBACK");
  int active_type = 0;
  uint32_t n_active = 0;
  mfgpu::vcycle_active(v, &active_type, &n_active);
  if (active_type != s->number_type || n_active != s->n)
    return einval("mfgpu_bicgstab_set_vcycle: the V-cycle's active vectors are not the solver's (type or length)");
  s->fn = vcycle_callback;
  s->ctx = v;
  return MFGPU_OK;
}

int mfgpu_bicgstab_begin(mfgpu_bicgstab *s, void *x_dev, const void *b_dev, double tolerance, uint32_t max_iterations,
                         void *stream) {
  return begin_common(s, x_dev, b_dev, tolerance, 0, max_iterations, stream);
}

int mfgpu_bicgstab_begin_relative(mfgpu_bicgstab *s, void *x_dev, const void *b_dev, double relative_tolerance,
                                  uint32_t max_iterations, void *stream) {
  if (!(relative_tolerance >= 0.0) || !std::isfinite(relative_tolerance))
    return einval("mfgpu_bicgstab_begin_relative: the relative tolerance must be a finite number >= 0");
  return begin_common(s, x_dev, b_dev, relative_tolerance, 1, max_iterations, stream);
}

int mfgpu_bicgstab_iterate(mfgpu_bicgstab *s, uint32_t n_iterations, void *stream) {
  if (!s) return einval("mfgpu_bicgstab_iterate: null argument");
  if (!s->begun) return einval("mfgpu_bicgstab_iterate: call mfgpu_bicgstab_begin first");
  return s->number_type == MFGPU_F64 ? iterate_typed<double>(s, n_iterations, (hipStream_t)stream)
                                     : iterate_typed<float>(s, n_iterations, (hipStream_t)stream);
}

int mfgpu_bicgstab_status(mfgpu_bicgstab *s, void *stream, mfgpu_cg_info *info) {
  if (!s || !info) return einval("mfgpu_bicgstab_status: null argument");
  if (!s->begun) return einval("mfgpu_bicgstab_status: call mfgpu_bicgstab_begin first");
  HIP_TRY(hipMemcpyAsync(s->mirror, s->state.get(), sizeof(BicgState), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  info->iterations = s->mirror->iterations;
  info->status = s->mirror->status;
  info->residual = std::sqrt(s->mirror->rr);
  info->initial_residual = s->mirror->initial_residual;
  return MFGPU_OK;
}

int mfgpu_bicgstab_solve(mfgpu_bicgstab *s, void *x_dev, const void *b_dev, double tolerance, uint32_t max_iterations,
                         uint32_t check_every, void *stream, mfgpu_cg_info *info) {
  if (!s || !info) return einval("mfgpu_bicgstab_solve: null argument");
  if (check_every == 0) return einval("mfgpu_bicgstab_solve: check_every must be at least 1");
  if (const int rc = mfgpu_bicgstab_begin(s, x_dev, b_dev, tolerance, max_iterations, stream)) return rc;
  do {  // ends: the count reaches max_iterations on the device at the latest
    if (const int rc = mfgpu_bicgstab_iterate(s, check_every, stream)) return rc;
    if (const int rc = mfgpu_bicgstab_status(s, stream, info)) return rc;
  } while (info->status == 0);
  return MFGPU_OK;
}

size_t mfgpu_bicgstab_memory_consumption(const mfgpu_bicgstab *s) { return s ? s->device_bytes : 0; }

void mfgpu_bicgstab_destroy(mfgpu_bicgstab *s) { delete s; }

}  // extern "C"
