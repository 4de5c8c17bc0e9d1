// What a V-cycle needs recomputed after a coefficient update, as calls that only enqueue: the set-up
// pieces of mfgpu_vcycle.hip -- the eigenvalue estimate, the Chebyshev scalars, the dense SPD inverse -- with every
// scalar and every intermediate in device memory, so that mfgpu_vcycle_refresh neither stops the host nor breaks a graph.
//   mfgpu_cg_chebyshev_scalars_dev        one thread: the recurrence of mfgpu_cg_chebyshev_scalars on a device lambda_max
//   mfgpu_estimate_lambda_max_enqueue     the power iteration of mfgpu_estimate_lambda_max, per step one mfgpu_vmult and
//     eig_scale_kernel      w = dinv w, partial sums of w.w and v.v; copies the fields the next kernel may not read itself
//     eig_normalise_kernel  sums the partials, estimate = |w| / |v|, count, status, v = w / |w|
//   mfgpu_spd_inverse_enqueue             the three stages of mfgpu_spd_inverse, the matrix in global memory (L2)
//     spd_factor_kernel     ONE workgroup: right-looking Cholesky, the pivot column in LDS, __syncthreads only
//     spd_invert_kernel     one wave per column of L^-1 (forward substitution; the columns are independent)
//     spd_product_kernel    one workgroup per row of inv = L^-T L^-1
// The streaming kernels are on the skeleton of mfgpu_stream.h; the reductions are those of mfgpu_cg.hip (double, one
// partial per block, every block of the consumer re-sums them in the order of vec_reduce_final; no atomics).  No kernel
// waits on another workgroup: order comes from the stream.
// State block rule (mfgpu_cg.hip): no kernel reads a field that the same kernel writes.  eig_start_kernel writes the
// `result` fields and reads none; eig_scale_kernel reads the `result` fields and writes the `scale` fields;
// eig_normalise_kernel reads the `scale` fields and writes the `result` fields.  spd_factor_kernel writes the status
// word and does not read it; the two kernels after it only read it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "mfgpu_device.h"
#include "mfgpu_refresh.h"
#include "mfgpu_stream.h"

using namespace mfgpu;

namespace {

static_assert(sizeof(mfgpu_eig_result) == 24, "the result is the head of the state block");
static_assert(sizeof(EigState) == kEigStateBytes, "the state block is 64 bytes (mfgpu_eig_workspace_bytes, include/mfgpu.h)");

// ---- Chebyshev scalars

// mfgpu_cg_chebyshev_scalars (mfgpu_cg.hip) operation for operation; contraction off, so that the device rounds where the
// host does
__global__ void chebyshev_scalars_kernel(uint32_t degree, const double *__restrict__ lambda_max_dev, double smoothing_range,
                                         double *__restrict__ f) {
#pragma clang fp contract(off)
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double lambda_max = *lambda_max_dev;
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
}

// ---- power iteration

// v[i] = sin(0.7 i) + 0.3, the start vector of mfgpu_estimate_lambda_max; resets the result fields but lambda_max, which
// keeps the last value until a later step replaces it
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) eig_start_kernel(EigState *__restrict__ s, T *__restrict__ v, size_t n) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T vv[W];
#pragma unroll
    for (int k = 0; k < W; ++k) vv[k] = (T)(sin(0.7 * (double)(uint32_t)(o + k)) + 0.3);
    stw<W>(v + o, vv);
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    s->result.estimate = 0.0;
    s->result.steps = 0;
    s->result.status = 0;
  }
}

// w = dinv w (mfgpu_vec_scale); partials of w.w and v.v.  Frozen: tells eig_normalise_kernel and writes nothing else.
template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
eig_scale_kernel(EigState *__restrict__ s, T *__restrict__ w, const T *__restrict__ dinv, const T *__restrict__ v,
                 double *__restrict__ pw, double *__restrict__ pv, size_t n) {
  __shared__ double red[4];
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (s->result.status != 0) {
    if (writer) s->frozen = 1;
    return;
  }
  if (writer) {
    s->frozen = 0;
    s->prev = s->result.estimate;
    s->steps_old = s->result.steps;
  }
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  double aw = 0.0, av = 0.0;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T wv[W], dv[W], vv[W];
    ldw<W>(w + o, wv);
    ldw<W>(dinv + o, dv);
    ldw<W>(v + o, vv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      wv[k] = wv[k] * dv[k];
      aw += (double)wv[k] * (double)wv[k];
      av += (double)vv[k] * (double)vv[k];
    }
    stw<W>(w + o, wv);
  });
  aw = block_sum(aw, red);
  av = block_sum(av, red);
  if (threadIdx.x == 0) {
    pw[blockIdx.x] = aw;
    pv[blockIdx.x] = av;
  }
}

// |w| and |v| from the partials; the estimate |w| / |v|, the count and the status of mfgpu_estimate_lambda_max's loop;
// v = (1 / |w|) w with the factor rounded to T (mfgpu_vec_equ).  `last`: this is step n_steps of the call.
template <typename T, bool VEC>
__global__ void __launch_bounds__(256)
eig_normalise_kernel(EigState *__restrict__ s, T *__restrict__ v, const T *__restrict__ w, const double *__restrict__ pw,
                     const double *__restrict__ pv, unsigned np, uint32_t min_steps, int last, size_t n) {
  __shared__ double red[4];
  if (s->frozen) return;
  const double nw = sqrt(resum(pw, np, red)), nv = sqrt(resum(pv, np, red));
  const bool ok = nw > 0.0 && nv > 0.0 && nw < INFINITY;  // false for NaN
  const double lam = nw / nv;
  const uint32_t steps = s->steps_old + 1u;
  const bool stop = steps >= min_steps && fabs(lam - s->prev) <= 0.01 * lam;
  const uint32_t status = !ok ? 3u : stop ? 1u : last ? 2u : 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    s->result.steps = steps;
    s->result.status = status;
    if (ok) s->result.estimate = lam;
    if (status == 1u || status == 2u) s->result.lambda_max = 1.2 * lam;
  }
  if (!ok) return;
  const T scale = (T)(1.0 / nw);
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, n, [&](size_t o, auto width) {
    constexpr int W = width;
    T wv[W];
    ldw<W>(w + o, wv);
#pragma unroll
    for (int k = 0; k < W; ++k) wv[k] = scale * wv[k];
    stw<W>(v + o, wv);
  });
}

template <typename T>
int eig_enqueue_typed(mfgpu_handle *op, const T *dinv, uint32_t min_steps, uint32_t n_steps, EigState *s, double *partials,
                      T *v, T *w, size_t n, hipStream_t st) {
  const bool vec = aligned16(v) && aligned16(w) && aligned16(dinv);
  const unsigned grid = stream_grid(n, lanes16<T>(), vec);
  double *pw = partials, *pv = partials + kStreamBlocks;
  dispatch([&](auto VEC) { hipLaunchKernelGGL((eig_start_kernel<T, VEC()>), dim3(grid), dim3(256), 0, st, s, v, n); }, vec);
  if (const int rc = hip_check(hipGetLastError(), "mfgpu_estimate_lambda_max_enqueue: start vector")) return rc;
  for (uint32_t k = 0; k < n_steps; ++k) {
    if (const int rc = mfgpu_vmult(op, w, v, (void *)st)) return rc;
    dispatch([&](auto VEC) {
      hipLaunchKernelGGL((eig_scale_kernel<T, VEC()>), dim3(grid), dim3(256), 0, st, s, w, dinv, (const T *)v, pw, pv, n);
      hipLaunchKernelGGL((eig_normalise_kernel<T, VEC()>), dim3(grid), dim3(256), 0, st, s, v, (const T *)w,
                         (const double *)pw, (const double *)pv, grid, min_steps, k + 1 == n_steps ? 1 : 0, n);
    }, vec);
    if (const int rc = hip_check(hipGetLastError(), "mfgpu_estimate_lambda_max_enqueue: step")) return rc;
  }
  return 0;
}

// ---- dense SPD inverse

constexpr int kFactorThreads = 1024;

// a = L L^T by the right-looking Cholesky, one workgroup.  S holds the working matrix by columns of the lower triangle:
// S[k n + i] = a[i][k], k <= i, so that a column is contiguous; step j scales column j into L's (S[j n + i] = L[i][j],
// also kept in LDS) and subtracts its outer product from the columns after it, which visits every entry in the order
// k = 0, 1, ... of mfgpu_spd_inverse's sums.  The diagonal of L waits in LDS until the end, since every thread reads the
// pivot S[j n + j] at the start of step j.  A pivot that is not a positive finite number ends the kernel with *status = 1
// (uniform: every thread reads the same pivot after the barrier).
__global__ void __launch_bounds__(kFactorThreads)
spd_factor_kernel(uint32_t n, const double *__restrict__ a, uint32_t lda, double *__restrict__ S, uint32_t *__restrict__ status) {
  __shared__ double col[MFGPU_SPD_INVERSE_DEVICE_MAX], diag[MFGPU_SPD_INVERSE_DEVICE_MAX];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  for (uint32_t e = tid; e < n * n; e += kFactorThreads) {
    const uint32_t i = e / n, k = e % n;
    if (k <= i) S[(size_t)k * n + i] = a[(size_t)i * lda + k];
  }
  __syncthreads();
  bool fail = false;
  for (uint32_t j = 0; j < n; ++j) {
    double *Sj = S + (size_t)j * n;
    const double d = Sj[j];
    if (!(d > 0.0) || !(d < INFINITY)) {
      fail = true;
      break;
    }
    const double ljj = sqrt(d);
    for (uint32_t i = j + 1u + tid; i < n; i += kFactorThreads) {
      const double l = Sj[i] / ljj;
      col[i] = l;
      Sj[i] = l;
    }
    if (tid == 0) diag[j] = ljj;
    __syncthreads();
    for (uint32_t k = j + 1u + wave; k < n; k += kFactorThreads / 64) {
      double *Sk = S + (size_t)k * n;
      const double ck = col[k];
      for (uint32_t i = k + lane; i < n; i += 64u) Sk[i] -= col[i] * ck;
    }
    __syncthreads();
  }
  if (!fail)
    for (uint32_t j = tid; j < n; j += kFactorThreads) S[(size_t)j * n + j] = diag[j];
  if (tid == 0) *status = fail ? 1u : 0u;
}

// Column c of M = L^-1 by forward substitution, one wave per column: x = e_c; for k = c, c + 1, ...: M[k][c] = x[k] /
// L[k][k], x[i] -= L[i][k] M[k][c] for i > k -- column k of L is contiguous in S.  Mt[c n + k] = M[k][c], k >= c; the
// entries k < c are never written and never read.
__global__ void __launch_bounds__(64)
spd_invert_kernel(uint32_t n, const double *__restrict__ S, double *__restrict__ Mt, const uint32_t *__restrict__ status) {
  __shared__ double x[MFGPU_SPD_INVERSE_DEVICE_MAX], diag[MFGPU_SPD_INVERSE_DEVICE_MAX];
  if (*status != 0) return;
  const uint32_t c = blockIdx.x, lane = threadIdx.x;
  for (uint32_t i = lane; i < n; i += 64u) {
    x[i] = i == c ? 1.0 : 0.0;
    diag[i] = S[(size_t)i * n + i];
  }
  __syncthreads();
  for (uint32_t k = c; k < n; ++k) {
    const double mk = x[k] / diag[k];
    const double *Sk = S + (size_t)k * n;
    for (uint32_t i = k + 1u + lane; i < n; i += 64u) x[i] -= Sk[i] * mk;
    if (lane == 0) Mt[(size_t)c * n + k] = mk;
    __syncthreads();  // the lane that owns x[i] changes with k
  }
}

// Row i of inv = M^T M: inv[i][j] = sum_{k >= i} M[k][i] M[k][j] for j <= i, both factors contiguous in Mt; one wave per
// entry, the lanes stride k, the 64 sums added in the order of wave_sum; the entry is stored on both sides of the
// diagonal.  The columns n .. ld - 1 of the row get zeros (the padding dense_solve_kernel reads).
__global__ void __launch_bounds__(256)
spd_product_kernel(uint32_t n, const double *__restrict__ Mt, double *__restrict__ inv, uint32_t ld,
                   const uint32_t *__restrict__ status) {
  __shared__ double row[MFGPU_SPD_INVERSE_DEVICE_MAX];
  if (*status != 0) return;
  const uint32_t i = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  for (uint32_t k = i + tid; k < n; k += 256u) row[k] = Mt[(size_t)i * n + k];
  __syncthreads();
  for (uint32_t j = wave; j <= i; j += 4u) {
    const double *Mj = Mt + (size_t)j * n;
    double acc = 0.0;
    for (uint32_t k = i + lane; k < n; k += 64u) acc += Mj[k] * row[k];
    acc = wave_sum(acc);
    if (lane == 0) {
      inv[(size_t)i * ld + j] = acc;
      inv[(size_t)j * ld + i] = acc;
    }
  }
  for (uint32_t c = n + tid; c < ld; c += 256u) inv[(size_t)i * ld + c] = 0.0;
}

size_t round16(size_t b) { return (b + 15u) & ~(size_t)15u; }

}  // namespace

namespace mfgpu {

int eig_enqueue(mfgpu_handle *op, const void *dinv, uint32_t min_iterations, uint32_t n_steps, EigState *state,
                double *partials, void *v, void *w, void *stream) {
  const size_t n = mfgpu_n_dofs(op);
  const uint32_t min_steps = min_iterations > 5u ? min_iterations : 5u;
  return handle_number_type(op) == MFGPU_F64
             ? eig_enqueue_typed<double>(op, (const double *)dinv, min_steps, n_steps, state, partials, (double *)v,
                                         (double *)w, n, (hipStream_t)stream)
             : eig_enqueue_typed<float>(op, (const float *)dinv, min_steps, n_steps, state, partials, (float *)v, (float *)w,
                                        n, (hipStream_t)stream);
}

}  // namespace mfgpu

extern "C" {

int mfgpu_cg_chebyshev_scalars_dev(uint32_t degree, const double *lambda_max_dev, double smoothing_range, double *f_dev,
                                   void *stream) {
  if (!lambda_max_dev || !f_dev) return einval("mfgpu_cg_chebyshev_scalars_dev: null argument");
  if (degree < 1 || !(smoothing_range > 1.0) || !std::isfinite(smoothing_range))
    return einval("mfgpu_cg_chebyshev_scalars_dev: need degree >= 1 and smoothing_range > 1");
  hipLaunchKernelGGL(chebyshev_scalars_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, degree, lambda_max_dev,
                     smoothing_range, f_dev);
  return hip_check(hipGetLastError(), "mfgpu_cg_chebyshev_scalars_dev");
}

size_t mfgpu_eig_workspace_bytes(uint32_t n_dofs, int number_type) {
  if (!valid_number_type(number_type)) return 0;
  return kEigStateBytes + 2 * kStreamBlocks * sizeof(double) + 2 * round16((size_t)n_dofs * esize(number_type));
}

int mfgpu_estimate_lambda_max_enqueue(mfgpu_handle *op, const void *inv_diag_dev, uint32_t min_iterations, uint32_t n_steps,
                                      void *workspace_dev, void *stream) {
  if (!op || !inv_diag_dev || !workspace_dev) return einval("mfgpu_estimate_lambda_max_enqueue: null argument");
  if (!aligned16(workspace_dev)) return einval("mfgpu_estimate_lambda_max_enqueue: the workspace must be 16-byte aligned");
  if (n_steps == 0) return einval("mfgpu_estimate_lambda_max_enqueue: n_steps must be at least 1");
  const uint32_t n = mfgpu_n_dofs(op);
  if (n == 0) return einval("mfgpu_estimate_lambda_max_enqueue: an operator without dofs");
  char *base = static_cast<char *>(workspace_dev);
  double *partials = reinterpret_cast<double *>(base + kEigStateBytes);
  char *v = base + kEigStateBytes + 2 * kStreamBlocks * sizeof(double);
  char *w = v + round16((size_t)n * esize(handle_number_type(op)));
  return eig_enqueue(op, inv_diag_dev, min_iterations, n_steps, reinterpret_cast<EigState *>(base), partials, v, w, stream);
}

size_t mfgpu_spd_inverse_workspace_bytes(uint32_t n) { return 2 * (size_t)n * n * sizeof(double); }

int mfgpu_spd_inverse_enqueue(uint32_t n, const double *a_dev, uint32_t lda, double *inv_dev, uint32_t ld,
                              void *workspace_dev, uint32_t *status_dev, void *stream) {
  if (n == 0 || n > MFGPU_SPD_INVERSE_DEVICE_MAX)
    return einval("mfgpu_spd_inverse_enqueue: n must be in [1, MFGPU_SPD_INVERSE_DEVICE_MAX]");
  if (!a_dev || !inv_dev || !workspace_dev || !status_dev) return einval("mfgpu_spd_inverse_enqueue: null argument");
  if (lda < n || ld < n) return einval("mfgpu_spd_inverse_enqueue: lda and ld must be at least n");
  if (((uintptr_t)workspace_dev & 7u) || ((uintptr_t)status_dev & 3u))
    return einval("mfgpu_spd_inverse_enqueue: misaligned workspace or status");
  const uintptr_t a0 = (uintptr_t)a_dev, a1 = a0 + ((size_t)(n - 1) * lda + n) * sizeof(double);
  const uintptr_t i0 = (uintptr_t)inv_dev, i1 = i0 + (size_t)n * ld * sizeof(double);
  const uintptr_t w0 = (uintptr_t)workspace_dev, w1 = w0 + mfgpu_spd_inverse_workspace_bytes(n);
  if ((a0 < i1 && i0 < a1) || (a0 < w1 && w0 < a1) || (i0 < w1 && w0 < i1))
    return einval("mfgpu_spd_inverse_enqueue: a, inv and the workspace must not overlap");
  const hipStream_t st = (hipStream_t)stream;
  double *S = static_cast<double *>(workspace_dev), *Mt = S + (size_t)n * n;
  hipLaunchKernelGGL(spd_factor_kernel, dim3(1), dim3(kFactorThreads), 0, st, n, a_dev, lda, S, status_dev);
  hipLaunchKernelGGL(spd_invert_kernel, dim3(n), dim3(64), 0, st, n, (const double *)S, Mt, (const uint32_t *)status_dev);
  hipLaunchKernelGGL(spd_product_kernel, dim3(n), dim3(256), 0, st, n, (const double *)Mt, inv_dev, ld,
                     (const uint32_t *)status_dev);
  return hip_check(hipGetLastError(), "mfgpu_spd_inverse_enqueue");
}

}  // extern "C"
