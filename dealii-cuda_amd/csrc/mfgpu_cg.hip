// Device-resident conjugate gradients: SolverCG::solve of host/mfgpu_shim_poisson.h with every scalar
// (rz, pq, rr, alpha, beta, tolerance, iteration count, status) kept in a device state block, so that begin / iterate
// only enqueue work -- no allocation, no synchronisation, no host read-back -- and can be captured in a graph.
//   cg_init_kernel       begin:  x = 0, r = b, partial sums of r.r (and of r.z for NONE / JACOBI); resets the state
//   cg_dot_kernel        (a) partial sums of p.q; for CHEBYSHEV / CALLBACK also of r.z after the preconditioner
//   cg_update_kernel     (b) sums the p.q partials, alpha = rz / pq, x += alpha p, r -= alpha q, partial sums of r.r
//                            (and of r.z for NONE / JACOBI)
//   cg_direction_kernel  (c) sums the r.r / r.z partials, updates count and status, beta = rz_new / rz, p = z + beta p
// Streaming kernels on the skeleton of mfgpu_stream.h: grid-stride over 16-byte chunks per lane, the same body on single
// elements for the tail and for unaligned vectors, at most kStreamBlocks blocks of 256 threads.  Reductions with its
// block_sum / resum: double accumulation, one partial per block, fixed order; EVERY block of the consuming kernel
// re-sums the <= kStreamBlocks partials with the code of vec_reduce_final (mfgpu_aux.hip), so all blocks hold the same
// bits of alpha and beta.  No atomics, no counters, no grid barrier.
// State block rule: no kernel reads a field that the same kernel writes (another block could see either value).
// cg_init_kernel writes the `begin` and `direction` fields and reads none; cg_update_kernel reads the `direction`
// fields and writes the `update` fields; cg_direction_kernel reads the `begin` and `update` fields and writes the
// `direction` fields; cg_dot_kernel only reads.  What a kernel reads was therefore written by an earlier launch and is
// uniform over its grid, which also makes the early returns below uniform per block.  The absolute tolerance of a solve
// begun with a relative one (mfgpu_cg_begin_relative) is a `direction` field that the first launch of
// cg_direction_kernel writes and only the later launches read.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "mfgpu_device.h"
#include "mfgpu_stream.h"

using namespace mfgpu;

namespace {

struct CgState {
  // begin: written by cg_init_kernel
  double tolerance;  // begin_relative: the relative tolerance, see tolerance_abs
  uint32_t max_iterations, relative;
  // direction: written by cg_direction_kernel (status and iterations also reset by cg_init_kernel)
  double rz, rr, beta, initial_residual;
  uint32_t iterations, status;
  // update: written by cg_update_kernel
  double pq, alpha, rz_old;
  uint32_t it_old, frozen, breakdown, pad1;
  // direction, mfgpu_cg_begin_relative only: tolerance * sqrt(r.r) of the start, written by the FIRST launch of
  // cg_direction_kernel of a solve (which does not read it) and read by the later ones (which do not write it)
  double tolerance_abs;
  double pad2[3];
};
static_assert(sizeof(CgState) == 128, "the state block is 128 bytes (mfgpu_cg_memory_consumption, include/mfgpu.h)");

enum Prec { P_NONE = MFGPU_CG_NONE, P_JACOBI = MFGPU_CG_JACOBI, P_STORED = 2 };  // P_STORED: z is a vector (CHEBYSHEV, CALLBACK)

// begin: x = 0, r = b; partials of r.r and, for JACOBI, of r.(dinv r)
template <typename T, bool VEC, int PREC>
__global__ void __launch_bounds__(256)
cg_init_kernel(CgState *__restrict__ s, T *__restrict__ x, T *__restrict__ r, const T *__restrict__ b,
               const T *__restrict__ dinv, double *__restrict__ prr, double *__restrict__ prz, double tolerance,
               uint32_t relative, uint32_t max_iterations, size_t n) {
  __shared__ double red[4];
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  double arr = 0.0, arz = 0.0;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T bv[W], dv[W], zero[W];
    ldw<W>(b + o, bv);
    if (PREC == P_JACOBI) ldw<W>(dinv + o, dv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      zero[k] = T(0);
      arr += (double)bv[k] * (double)bv[k];
      if (PREC == P_JACOBI) arz += (double)bv[k] * (double)(dv[k] * bv[k]);
    }
    stw<W>(x + o, zero);
    stw<W>(r + o, bv);
  });
  arr = block_sum(arr, red);
  if (PREC == P_JACOBI) arz = block_sum(arz, red);
  if (threadIdx.x == 0) {
    prr[blockIdx.x] = arr;
    if (PREC == P_JACOBI) prz[blockIdx.x] = arz;
    if (blockIdx.x == 0) {
      s->tolerance = tolerance;
      s->relative = relative;
      s->max_iterations = max_iterations;
      s->iterations = 0;
      s->status = 0;
    }
  }
}

// partials of v.w; nothing once the solve has ended
template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
cg_dot_kernel(const CgState *__restrict__ s, double *__restrict__ partial, const T *__restrict__ v,
              const T *__restrict__ w, size_t n) {
  __shared__ double red[4];
  if (s->status != 0) return;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  double acc = 0.0;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T a[W], b[W];
    ldw<W>(v + o, a);
    ldw<W>(w + o, b);
#pragma unroll
    for (int k = 0; k < W; ++k) acc += (double)a[k] * (double)b[k];
  });
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

template <typename T, int PREC>
__device__ __forceinline__ void update_elem(T &x, T &r, T p, T q, T d, T alpha, double &arr, double &arz) {
  x = x + alpha * p;
  r = r - alpha * q;
  arr += (double)r * (double)r;
  if (PREC == P_JACOBI) arz += (double)r * (double)(d * r);
}

// (b): alpha = rz / (p.q) from the partials of (a); x += alpha p; r -= alpha q; partials of r.r (JACOBI: and r.z)
template <typename T, bool VEC, int PREC>
__global__ void __launch_bounds__(256)
cg_update_kernel(CgState *__restrict__ s, T *__restrict__ x, T *__restrict__ r, const T *__restrict__ p,
                 const T *__restrict__ q, const T *__restrict__ dinv, const double *__restrict__ ppq,
                 double *__restrict__ prr, double *__restrict__ prz, unsigned np, size_t n) {
  __shared__ double red[4];
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (s->status != 0) {  // frozen: tell (c), write nothing else
    if (writer) s->frozen = 1;
    return;
  }
  const double pq = resum(ppq, np, red), rz = s->rz;
  const bool ok = pq > 0.0 && pq < INFINITY;  // false for NaN
  const double alpha_d = rz / pq;
  const T alpha = (T)alpha_d;
  if (writer) {
    s->frozen = 0;
    s->breakdown = ok ? 0 : 1;
    s->pq = pq;
    s->alpha = alpha_d;
    s->rz_old = rz;
    s->it_old = s->iterations;
  }
  if (!ok) return;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  double arr = 0.0, arz = 0.0;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T xv[W], rv[W], pv[W], qv[W], dv[W];
    ldw<W>(x + o, xv);
    ldw<W>(r + o, rv);
    ldw<W>(p + o, pv);
    ldw<W>(q + o, qv);
    if (PREC == P_JACOBI) ldw<W>(dinv + o, dv);
#pragma unroll
    for (int k = 0; k < W; ++k)
      update_elem<T, PREC>(xv[k], rv[k], pv[k], qv[k], PREC == P_JACOBI ? dv[k] : T(0), alpha, arr, arz);
    stw<W>(x + o, xv);
    stw<W>(r + o, rv);
  });
  arr = block_sum(arr, red);
  if (PREC == P_JACOBI) arz = block_sum(arz, red);
  if (threadIdx.x == 0) {
    prr[blockIdx.x] = arr;
    if (PREC == P_JACOBI) prz[blockIdx.x] = arz;
  }
}

// (c): rr and rz from the partials; count, residual and status; beta = rz / rz_old; p = z + beta p (first: p = z) with
// z = r (NONE), dinv r (JACOBI) or the stored vector.  p is left alone once the solve has ended, as SolverCG returns
// before its p.sadd.
template <typename T, bool VEC, int PREC>
__global__ void __launch_bounds__(256)
cg_direction_kernel(CgState *__restrict__ s, T *__restrict__ p, const T *__restrict__ r, const T *__restrict__ z,
                    const T *__restrict__ dinv, const double *__restrict__ prr, const double *__restrict__ prz,
                    unsigned np, int first, size_t n) {
  __shared__ double red[4];
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (!first) {
    if (s->frozen) return;
    if (s->breakdown) {  // p.q was not a positive finite number: (b) wrote nothing
      if (writer) s->status = 3;
      return;
    }
  }
  const double rr = resum(prr, np, red);
  const double rz = PREC == P_NONE ? rr : resum(prz, np, red);
  const uint32_t it = first ? 0u : s->it_old + 1u;
  const double res = sqrt(rr);
  // relative: the first launch forms the absolute tolerance from the start residual, the later ones read it back
  const bool relative = s->relative != 0;
  const double tolerance = !relative ? s->tolerance : first ? s->tolerance * res : s->tolerance_abs;
  const uint32_t status = res <= tolerance ? 1u : it >= s->max_iterations ? 2u : 0u;
  const double beta_d = first ? 0.0 : rz / s->rz_old;
  const T beta = (T)beta_d;
  if (writer) {
    s->rr = rr;
    s->rz = rz;
    s->beta = beta_d;
    s->iterations = it;
    s->status = status;
    if (first) s->initial_residual = res;
    if (first && relative) s->tolerance_abs = tolerance;
  }
  if (status != 0) return;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  const bool is_first = first != 0;  // a local: the parameter itself, captured by reference, changes the code above
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T pv[W], zv[W], dv[W];
    ldw<W>((PREC == P_STORED ? z : r) + o, zv);
    if (PREC == P_JACOBI) {
      ldw<W>(dinv + o, dv);
#pragma unroll
      for (int k = 0; k < W; ++k) zv[k] = dv[k] * zv[k];
    }
    if (is_first) {
      stw<W>(p + o, zv);
    } else {
      ldw<W>(p + o, pv);
#pragma unroll
      for (int k = 0; k < W; ++k) pv[k] = beta * pv[k] + zv[k];
      stw<W>(p + o, pv);
    }
  });
}

}  // namespace

struct mfgpu_cg {
  mfgpu_handle *A = nullptr;
  int prec = MFGPU_CG_NONE, number_type = MFGPU_F64;
  size_t n = 0;
  const void *dinv = nullptr;
  std::vector<double> cheb;  // mfgpu_cg_chebyshev_scalars
  uint32_t degree = 0;
  mfgpu::DeviceArray<void> r, p, q, z, cheb_r, cheb_upd, cheb_t;
  mfgpu::DeviceArray<double> partials;  // p.q | r.r | r.z, kStreamBlocks each
  mfgpu::DeviceArray<CgState> state;
  CgState *mirror = nullptr;  // pinned
  int (*fn)(void *, void *, const void *, void *) = nullptr;
  void *ctx = nullptr;
  // the solve in progress
  void *x = nullptr;
  const void *b = nullptr;
  bool begun = false, vec = false;
  unsigned grid = 1;
  size_t device_bytes = 0;
  ~mfgpu_cg() {
    if (mirror) hipHostFree(mirror);
  }
};

namespace {

int kernel_prec(const mfgpu_cg *s) { return s->prec == MFGPU_CG_NONE ? P_NONE : s->prec == MFGPU_CG_JACOBI ? P_JACOBI : P_STORED; }

// f(VEC, PREC) with the solver's (vec, prec) as constants: one launch of a kernel<T, VEC(), PREC()>
template <typename F>
void with_vec_prec(const mfgpu_cg *s, F &&f) {
  static_assert(P_NONE == 0 && P_JACOBI == 1 && P_STORED == 2, "OneOf3 carries the Prec");
  dispatch(f, s->vec, OneOf3{kernel_prec(s)});
}

template <typename T>
int dot_launch(mfgpu_cg *s, double *partial, const void *v, const void *w, hipStream_t st) {
  dispatch([&](auto VEC) {
    hipLaunchKernelGGL((cg_dot_kernel<T, VEC()>), dim3(s->grid), dim3(256), 0, st, s->state.get(), partial,
                       (const T *)v, (const T *)w, s->n);
  }, s->vec);
  return mfgpu::hip_check(hipGetLastError(), "mfgpu_cg: dot");
}

// z = M^-1 r for the preconditioners that store z, then the partials of r.z
template <typename T>
int precondition(mfgpu_cg *s, hipStream_t st) {
  if (kernel_prec(s) != P_STORED) return 0;
  void *z = s->z.get();
  const void *r = s->r.get();
  if (s->prec == MFGPU_CG_CALLBACK) {
    if (const int rc = s->fn(s->ctx, z, r, (void *)st)) {
      mfgpu::set_error("mfgpu_cg: the preconditioner callback failed");
      return rc;
    }
  } else {  // PreconditionChebyshev::run_fused, zero start (host/mfgpu_shim_mg.h)
    if (const int rc = mfgpu_vec_chebyshev_start(z, s->cheb_upd.get(), s->cheb_r.get(), r, nullptr, s->dinv, s->cheb[0], 1,
                                                 s->n, s->number_type, (void *)st))
      return rc;
    for (uint32_t k = 1; k < s->degree; ++k) {
      if (const int rc = mfgpu_vmult(s->A, s->cheb_t.get(), s->cheb_upd.get(), (void *)st)) return rc;
      if (const int rc = mfgpu_vec_chebyshev_update(z, s->cheb_upd.get(), s->cheb_r.get(), s->cheb_t.get(), s->dinv,
                                                    s->cheb[2 * k - 1], s->cheb[2 * k], s->n, s->number_type, (void *)st))
        return rc;
    }
  }
  return dot_launch<T>(s, s->partials.get() + 2 * kStreamBlocks, r, z, st);
}

template <typename T>
int direction_launch(mfgpu_cg *s, int first, hipStream_t st) {
  double *prr = s->partials.get() + kStreamBlocks, *prz = prr + kStreamBlocks;
  with_vec_prec(s, [&](auto VEC, auto PREC) {
    hipLaunchKernelGGL((cg_direction_kernel<T, VEC(), PREC()>), dim3(s->grid), dim3(256), 0, st, s->state.get(),
                       (T *)s->p.get(), (const T *)s->r.get(), (const T *)s->z.get(), (const T *)s->dinv,
                       (const double *)prr, (const double *)prz, s->grid, first, s->n);
  });
  return mfgpu::hip_check(hipGetLastError(), "mfgpu_cg: direction update");
}

template <typename T>
int begin_typed(mfgpu_cg *s, double tolerance, uint32_t relative, uint32_t max_iterations, hipStream_t st) {
  double *prr = s->partials.get() + kStreamBlocks, *prz = prr + kStreamBlocks;
  with_vec_prec(s, [&](auto VEC, auto PREC) {
    hipLaunchKernelGGL((cg_init_kernel<T, VEC(), PREC()>), dim3(s->grid), dim3(256), 0, st, s->state.get(), (T *)s->x,
                       (T *)s->r.get(), (const T *)s->b, (const T *)s->dinv, prr, prz, tolerance, relative,
                       max_iterations, s->n);
  });
  if (const int rc = mfgpu::hip_check(hipGetLastError(), "mfgpu_cg_begin")) return rc;
  if (const int rc = precondition<T>(s, st)) return rc;
  return direction_launch<T>(s, 1, st);
}

template <typename T>
int iterate_typed(mfgpu_cg *s, uint32_t n_iterations, hipStream_t st) {
  double *ppq = s->partials.get(), *prr = ppq + kStreamBlocks, *prz = prr + kStreamBlocks;
  for (uint32_t it = 0; it < n_iterations; ++it) {
    if (const int rc = mfgpu_vmult(s->A, s->q.get(), s->p.get(), (void *)st)) return rc;
    if (const int rc = dot_launch<T>(s, ppq, s->p.get(), s->q.get(), st)) return rc;
    with_vec_prec(s, [&](auto VEC, auto PREC) {
      hipLaunchKernelGGL((cg_update_kernel<T, VEC(), PREC()>), dim3(s->grid), dim3(256), 0, st, s->state.get(),
                         (T *)s->x, (T *)s->r.get(), (const T *)s->p.get(), (const T *)s->q.get(), (const T *)s->dinv,
                         (const double *)ppq, prr, prz, s->grid, s->n);
    });
    if (const int rc = mfgpu::hip_check(hipGetLastError(), "mfgpu_cg_iterate")) return rc;
    if (const int rc = precondition<T>(s, st)) return rc;
    if (const int rc = direction_launch<T>(s, 0, st)) return rc;
  }
  return 0;
}

bool chebyshev_arguments_ok(uint32_t degree, double lambda_max, double smoothing_range) {
  return degree >= 1 && lambda_max > 0.0 && smoothing_range > 1.0 && std::isfinite(lambda_max) &&
         std::isfinite(smoothing_range);
}

}  // namespace

extern "C" {

int mfgpu_cg_chebyshev_scalars(uint32_t degree, double lambda_max, double smoothing_range, double *f) {
  if (!f) return einval("mfgpu_cg_chebyshev_scalars: null output");
  if (!chebyshev_arguments_ok(degree, lambda_max, smoothing_range))
    return einval("mfgpu_cg_chebyshev_scalars: need degree >= 1, lambda_max > 0 and smoothing_range > 1");
  // PreconditionChebyshev::run / run_fused (host/mfgpu_shim_mg.h)
  const double lambda_min = lambda_max / smoothing_range;
  const double theta = 0.5 * (lambda_max + lambda_min), delta = 0.5 * (lambda_max - lambda_min);
  const double sigma = theta / delta;
  double rho = 1.0 / sigma;
  f[0] = 1.0 / theta;
  for (uint32_t k = 1; k < degree; ++k) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    f[2 * k - 1] = rho_new * rho;
    f[2 * k] = 2.0 * rho_new / delta;
    rho = rho_new;
  }
  return MFGPU_OK;
}

int mfgpu_cg_create(mfgpu_handle *A, int preconditioner, const void *inv_diag_dev, uint32_t chebyshev_degree,
                    double lambda_max, double smoothing_range, mfgpu_cg **out) {
  if (!A || !out) return einval("mfgpu_cg_create: null argument");
  if (preconditioner < MFGPU_CG_NONE || preconditioner > MFGPU_CG_CALLBACK)
    return einval("mfgpu_cg_create: unknown preconditioner");
  const bool needs_diag = preconditioner == MFGPU_CG_JACOBI || preconditioner == MFGPU_CG_CHEBYSHEV;
  if (needs_diag && !inv_diag_dev) return einval("mfgpu_cg_create: JACOBI and CHEBYSHEV need inv_diag_dev");
  if (preconditioner == MFGPU_CG_CHEBYSHEV && !chebyshev_arguments_ok(chebyshev_degree, lambda_max, smoothing_range))
    return einval("mfgpu_cg_create: CHEBYSHEV needs degree >= 1, lambda_max > 0 and smoothing_range > 1");
  mfgpu_cg *s = new (std::nothrow) mfgpu_cg;
  if (!s) return MFGPU_ENOMEM;
  s->A = A;
  s->prec = preconditioner;
  s->number_type = mfgpu::handle_number_type(A);
  s->n = mfgpu_n_dofs(A);
  s->dinv = needs_diag ? inv_diag_dev : nullptr;
  const size_t vbytes = s->n * mfgpu::esize(s->number_type);
  int rc = 0;
  if (preconditioner == MFGPU_CG_CHEBYSHEV) {
    s->degree = chebyshev_degree;
    s->cheb.resize(2 * chebyshev_degree - 1);
    rc = mfgpu_cg_chebyshev_scalars(chebyshev_degree, lambda_max, smoothing_range, s->cheb.data());
  }
  mfgpu::DeviceArray<void> *vectors[7] = {&s->r, &s->p, &s->q, &s->z, &s->cheb_r, &s->cheb_upd, &s->cheb_t};
  const int n_vectors = preconditioner == MFGPU_CG_CHEBYSHEV ? 7 : preconditioner == MFGPU_CG_CALLBACK ? 4 : 3;
  for (int v = 0; v < n_vectors && !rc; ++v) rc = vectors[v]->alloc(vbytes, true);
  if (!rc) rc = s->partials.alloc(3 * kStreamBlocks, true);
  if (!rc) rc = s->state.alloc(1, true);
  if (!rc) rc = mfgpu::hip_check(hipHostMalloc((void **)&s->mirror, sizeof(CgState), hipHostMallocDefault), "mfgpu_cg_create");
  if (rc) {
    delete s;
    return rc;
  }
  s->device_bytes = n_vectors * vbytes + s->partials.bytes() + s->state.bytes();
  *out = s;
  return MFGPU_OK;
}

int mfgpu_cg_set_callback(mfgpu_cg *s, int (*fn)(void *ctx, void *z_dev, const void *r_dev, void *stream), void *ctx) {
  if (!s || !fn) return einval("mfgpu_cg_set_callback: null argument");
  if (s->prec != MFGPU_CG_CALLBACK) return einval("mfgpu_cg_set_callback: the solver was not created with MFGPU_CG_CALLBACK");
  s->fn = fn;
  s->ctx = ctx;
  return MFGPU_OK;
}

namespace {
int begin_common(mfgpu_cg *s, void *x_dev, const void *b_dev, double tolerance, uint32_t relative, uint32_t max_iterations,
                 void *stream) {
  if (!s || !x_dev || !b_dev) return einval("mfgpu_cg_begin: null argument");
  if (s->prec == MFGPU_CG_CALLBACK && !s->fn) return einval("mfgpu_cg_begin: no callback set (mfgpu_cg_set_callback)");
  const size_t vbytes = s->n * mfgpu::esize(s->number_type);
  const uintptr_t x0 = (uintptr_t)x_dev, b0 = (uintptr_t)b_dev;
  if (x0 < b0 + vbytes && b0 < x0 + vbytes) return einval("mfgpu_cg_begin: x and b must not overlap");
  s->x = x_dev;
  s->b = b_dev;
  s->vec = aligned16(x_dev) && aligned16(b_dev) && aligned16(s->dinv);
  s->grid = stream_grid(s->n, 16 / mfgpu::esize(s->number_type), s->vec);
  s->begun = true;
  return s->number_type == MFGPU_F64 ? begin_typed<double>(s, tolerance, relative, max_iterations, (hipStream_t)stream)
                                     : begin_typed<float>(s, tolerance, relative, max_iterations, (hipStream_t)stream);
}
}  // namespace

int mfgpu_cg_begin(mfgpu_cg *s, void *x_dev, const void *b_dev, double tolerance, uint32_t max_iterations, void *stream) {
  return begin_common(s, x_dev, b_dev, tolerance, 0, max_iterations, stream);
}

int mfgpu_cg_begin_relative(mfgpu_cg *s, void *x_dev, const void *b_dev, double relative_tolerance,
                            uint32_t max_iterations, void *stream) {
  if (!(relative_tolerance >= 0.0) || !std::isfinite(relative_tolerance))
    return einval("mfgpu_cg_begin_relative: the relative tolerance must be a finite number >= 0");
  return begin_common(s, x_dev, b_dev, relative_tolerance, 1, max_iterations, stream);
}

// the library's own callback: z = M^-1 r is one mfgpu_vcycle_apply
static int vcycle_callback(void *ctx, void *z_dev, const void *r_dev, void *stream) {
  return mfgpu_vcycle_apply(static_cast<mfgpu_vcycle *>(ctx), z_dev, r_dev, stream);
}

int mfgpu_cg_set_vcycle(mfgpu_cg *s, mfgpu_vcycle *v) {
  if (!s || !v) return einval("mfgpu_cg_set_vcycle: null argument");
  if (s->prec != MFGPU_CG_CALLBACK) return einval("mfgpu_cg_set_vcycle: the solver was not created with MFGPU_CG_CALLBACK");
  int active_type = 0;
  uint32_t n_active = 0;
  mfgpu::vcycle_active(v, &active_type, &n_active);
  if (active_type != s->number_type || n_active != s->n)
    return einval("mfgpu_cg_set_vcycle: the V-cycle's active vectors are not the solver's (type or length)");
  s->fn = vcycle_callback;
  s->ctx = v;
  return MFGPU_OK;
}

int mfgpu_cg_iterate(mfgpu_cg *s, uint32_t n_iterations, void *stream) {
  if (!s) return einval("mfgpu_cg_iterate: null argument");
  if (!s->begun) return einval("mfgpu_cg_iterate: call mfgpu_cg_begin first");
  return s->number_type == MFGPU_F64 ? iterate_typed<double>(s, n_iterations, (hipStream_t)stream)
                                     : iterate_typed<float>(s, n_iterations, (hipStream_t)stream);
}

int mfgpu_cg_status(mfgpu_cg *s, void *stream, mfgpu_cg_info *info) {
  if (!s || !info) return einval("mfgpu_cg_status: null argument");
  if (!s->begun) return einval("mfgpu_cg_status: call mfgpu_cg_begin first");
  HIP_TRY(hipMemcpyAsync(s->mirror, s->state.get(), sizeof(CgState), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  info->iterations = s->mirror->iterations;
  info->status = s->mirror->status;
  info->residual = std::sqrt(s->mirror->rr);
  info->initial_residual = s->mirror->initial_residual;
  return MFGPU_OK;
}

int mfgpu_cg_solve(mfgpu_cg *s, void *x_dev, const void *b_dev, double tolerance, uint32_t max_iterations,
                   uint32_t check_every, void *stream, mfgpu_cg_info *info) {
  if (!s || !info) return einval("mfgpu_cg_solve: null argument");
  if (check_every == 0) return einval("mfgpu_cg_solve: check_every must be at least 1");
  if (const int rc = mfgpu_cg_begin(s, x_dev, b_dev, tolerance, max_iterations, stream)) return rc;
  do {  // ends: the count reaches max_iterations on the device at the latest
    if (const int rc = mfgpu_cg_iterate(s, check_every, stream)) return rc;
    if (const int rc = mfgpu_cg_status(s, stream, info)) return rc;
  } while (info->status == 0);
  return MFGPU_OK;
}

size_t mfgpu_cg_memory_consumption(const mfgpu_cg *s) { return s ? s->device_bytes : 0; }

void mfgpu_cg_destroy(mfgpu_cg *s) { delete s; }

}  // extern "C"
