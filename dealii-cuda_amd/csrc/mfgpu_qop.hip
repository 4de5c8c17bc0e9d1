// The submit / integrate half of the integrator and the fused quadrature-point operator (include/mfgpu.h,
// "mfgpu_integrator_integrate" and "mfgpu_qop").  Double only, as the integrator.
//
//   integrate: dst_i = sum_cells sum_q JxW_q [phi_i(x_q) v_q + grad_x phi_i(x_q) . g_q] -- the transpose of
//              mfgpu_integrator_evaluate (submit_value / submit_gradient / integrate / distribute_local_to_global of
//              FEEvaluationGpu, fee_gpu.cuh:283-352, for caller-given point data).
//   qop:       (A u)_i = sum_cells sum_q JxW_q [grad phi_i . (D grad u + gamma u) + phi_i (beta . grad u + c u)] in one
//              cell kernel.  The coefficients are folded once per mfgpu_qop_set_coefficients into reference form
//              (JxW J^-1 D J^-T, JxW J^-1 gamma, JxW J^-1 beta, JxW c), so an apply reads neither inv_jac nor JxW.
//
// Structure, as mfgpu_integrate.hip: one wave64 workgroup per cell, sum factorisation in LDS (tensor<>), hn_resolve on
// LDS pencils, per-cell local vectors in the integrator's scratch, then the per-dof gather over the integrator's
// host-built CSR (ascending (cell, local index) order).  No atomics: bitwise repeatable.  Everything only enqueues.
// Folded arrays are component-major inside a cell ([cell][component][q]), so a wave reads each component contiguously.
#include <hip/hip_runtime.h>

#include <memory>

#include "mfgpu_device.h"
#include "mfgpu_integrate_cell.h"
#include "mfgpu_points.h"

using namespace mfgpu;

namespace {

struct QopArgs {
  const uint32_t *loc2glob;  // [n_cells * N^dim]
  const uint32_t *cmask;     // [n_cells] or nullptr
  const uint8_t *con;        // [n_dofs]
  const double *tab;         // Tab<N>
  double *local;             // [n_cells * N^dim]
  // integrate
  const double *v, *g;       // [n_cells * N^dim], [n_cells * N^dim * dim]; either may be nullptr
  const double *jxw, *jinv;  // as IntegratorView
  int general;
  // qop: folded terms, nullptr = term absent (transpose: conv and flux arrive swapped)
  const double *src;
  const double *diff;  // diff_scalar: [cell][q]; else [cell][e * dim + f][q]
  const double *conv;  // [cell][e][q]
  const double *flux;  // [cell][e][q]
  const double *reac;  // [cell][q]
  int diff_scalar, transpose;
};

// LOC (nodal, before the transposed hanging-node resolution) = integral of the point values in V (if has_v) against
// phi_i plus the reference fluxes in G[e] (if has_g) against d phi_i / d xi_e.  Thread t owns LOC[t], LOC[t + 64], ... in
// the zero fill and in every accumulation, so those need no barrier of their own; tensor<> begins and ends with one.
template <int dim, int N>
__device__ __forceinline__ void integrate_local(const double *tab, bool has_v, bool has_g, const double *V, const double *G,
                                                double *LOC, double *TO, double *T1, double *T2) {
  constexpr int ND = cpow(N, dim);
  using TB = Tab<N>;
  const double *SI = tab + TB::SI, *GI = tab + TB::GI;
  if (has_v) {
    tensor<dim, N, N>(V, LOC, SI, SI, SI, T1, T2);
  } else {
    for (int i = threadIdx.x; i < ND; i += 64) LOC[i] = 0;
  }
  if (has_g) {
#pragma unroll
    for (int e = 0; e < dim; ++e) {
      tensor<dim, N, N>(G + e * ND, TO, e == 0 ? GI : SI, e == 1 ? GI : SI, e == 2 ? GI : SI, T1, T2);
      for (int i = threadIdx.x; i < ND; i += 64) LOC[i] += TO[i];
    }
  }
}

template <int dim, int N>
__global__ void __launch_bounds__(64) integrate_cell_kernel(QopArgs a) {
  constexpr int ND = cpow(N, dim);
  using TB = Tab<N>;
  __shared__ double tab[TB::size], V[ND], G[dim * ND], LOC[ND], TO[ND], T1[ND], T2[ND];
  const uint32_t c = blockIdx.x;
  const size_t c0 = (size_t)c * ND;
  load_tab<N>(tab, a.tab);
  const unsigned mask = a.cmask ? a.cmask[c] : 0u;
  const double j0 = (a.g && !a.general) ? a.jinv[c] : 0.0;
  for (int q = threadIdx.x; q < ND; q += 64) {
    const double w = a.jxw[c0 + q];
    if (a.v) V[q] = w * a.v[c0 + q];
    if (a.g) {
      double g[dim];
#pragma unroll
      for (int k = 0; k < dim; ++k) g[k] = a.g[(c0 + q) * dim + k];
      if (!a.general) {
#pragma unroll
        for (int e = 0; e < dim; ++e) G[e * ND + q] = w * j0 * g[e];
      } else {
        const double *J = a.jinv + (c0 + q) * (dim * dim);  // J^-1[e][k] = d xi_e / d x_k
#pragma unroll
        for (int e = 0; e < dim; ++e) {
          double s = 0;
#pragma unroll
          for (int k = 0; k < dim; ++k) s = fma(J[e * dim + k], g[k], s);
          G[e * ND + q] = w * s;
        }
      }
    }
  }
  integrate_local<dim, N>(tab, a.v != nullptr, a.g != nullptr, V, G, LOC, TO, T1, T2);
  if (mask) hn_resolve<dim, N, true>(LOC, mask, tab + TB::W);
  __syncthreads();
  for (int i = threadIdx.x; i < ND; i += 64) a.local[c0 + i] = LOC[i];
}

// The cell operator on the nodal values in A (already hanging-node resolved); the result overwrites A (LOC is A: the
// nodal values are dead once the point values exist).
template <int dim, int N>
__device__ __forceinline__ void qop_cell_apply(const QopArgs &a, size_t c0, const double *tab, double *A, double *U,
                                               double *G, double *TO, double *T1, double *T2) {
  constexpr int ND = cpow(N, dim);
  using TB = Tab<N>;
  const double *S = tab + TB::SE, *D = tab + TB::GE;
  const bool in_val = a.flux || a.reac, in_grad = a.diff || a.conv;
  const bool out_val = a.conv || a.reac, out_grad = a.diff || a.flux;
  if (in_val) tensor<dim, N, N>(A, U, S, S, S, T1, T2);
  if (in_grad) {
#pragma unroll
    for (int e = 0; e < dim; ++e) tensor<dim, N, N>(A, G + e * ND, e == 0 ? D : S, e == 1 ? D : S, e == 2 ? D : S, T1, T2);
  }
  for (int q = threadIdx.x; q < ND; q += 64) {  // the thread owns point q: in place
    double g[dim], fl[dim], vo = 0;
    const double u = in_val ? U[q] : 0.0;
#pragma unroll
    for (int e = 0; e < dim; ++e) {
      g[e] = in_grad ? G[e * ND + q] : 0.0;
      fl[e] = 0;
    }
    if (a.diff) {
      if (a.diff_scalar) {
        const double m = a.diff[c0 + q];
#pragma unroll
        for (int e = 0; e < dim; ++e) fl[e] = m * g[e];
      } else {
        const double *M = a.diff + c0 * (dim * dim) + q;
#pragma unroll
        for (int e = 0; e < dim; ++e)
#pragma unroll
          for (int f = 0; f < dim; ++f) {
            const double m = a.transpose ? M[(f * dim + e) * ND] : M[(e * dim + f) * ND];
            fl[e] = fma(m, g[f], fl[e]);
          }
      }
    }
    if (a.flux) {
#pragma unroll
      for (int e = 0; e < dim; ++e) fl[e] = fma(a.flux[c0 * dim + e * ND + q], u, fl[e]);
    }
    if (a.conv) {
#pragma unroll
      for (int e = 0; e < dim; ++e) vo = fma(a.conv[c0 * dim + e * ND + q], g[e], vo);
    }
    if (a.reac) vo = fma(a.reac[c0 + q], u, vo);
    if (out_val) U[q] = vo;
    if (out_grad) {
#pragma unroll
      for (int e = 0; e < dim; ++e) G[e * ND + q] = fl[e];
    }
  }
  integrate_local<dim, N>(tab, out_val, out_grad, U, G, A, TO, T1, T2);
}

template <int dim, int N>
__global__ void __launch_bounds__(64) qop_cell_kernel(QopArgs a) {
  constexpr int ND = cpow(N, dim);
  using TB = Tab<N>;
  __shared__ double tab[TB::size], A[ND], U[ND], G[dim * ND], TO[ND], T1[ND], T2[ND];
  const uint32_t c = blockIdx.x;
  const size_t c0 = (size_t)c * ND;
  load_tab<N>(tab, a.tab);
  const unsigned mask = a.cmask ? a.cmask[c] : 0u;
  for (int i = threadIdx.x; i < ND; i += 64) {  // constrained entries of src are read as 0
    const uint32_t gi = a.loc2glob[c0 + i];
    const double s = a.src[gi];
    A[i] = a.con[gi] ? 0.0 : s;
  }
  if (mask) hn_resolve<dim, N, false>(A, mask, tab + TB::W);
  qop_cell_apply<dim, N>(a, c0, tab, A, U, G, TO, T1, T2);
  if (mask) hn_resolve<dim, N, true>(A, mask, tab + TB::W);
  __syncthreads();
  for (int i = threadIdx.x; i < ND; i += 64) a.local[c0 + i] = A[i];
}

// local[cell][i] = (C^T K C)_ii of the cell: the cell operator with both hanging-node resolutions applied to the local
// unit vector e_i, entry i.  Set-up work: N^dim applies per cell.
template <int dim, int N>
__global__ void __launch_bounds__(64) qop_diag_kernel(QopArgs a) {
  constexpr int ND = cpow(N, dim);
  using TB = Tab<N>;
  __shared__ double tab[TB::size], A[ND], U[ND], G[dim * ND], TO[ND], T1[ND], T2[ND];
  const uint32_t c = blockIdx.x;
  const size_t c0 = (size_t)c * ND;
  load_tab<N>(tab, a.tab);
  const unsigned mask = a.cmask ? a.cmask[c] : 0u;
  for (int i = 0; i < ND; ++i) {
    for (int j = threadIdx.x; j < ND; j += 64) A[j] = j == i ? 1.0 : 0.0;
    if (mask) hn_resolve<dim, N, false>(A, mask, tab + TB::W);
    qop_cell_apply<dim, N>(a, c0, tab, A, U, G, TO, T1, T2);
    if (mask) hn_resolve<dim, N, true>(A, mask, tab + TB::W);
    __syncthreads();
    if ((int)threadIdx.x == (i & 63)) a.local[c0 + i] = A[i];
    __syncthreads();
  }
}

// dst[dof] = sum of the dof's local entries in ascending (cell, local index) order, as rhs_gather_kernel; with src the
// constrained rows are identity rows.  dst may be src (a thread reads src[i] before it writes dst[i]): no __restrict__
// on the two.
__global__ void __launch_bounds__(256) qop_gather_kernel(double *dst, const double *src,
                                                         const double *__restrict__ local,
                                                         const uint32_t *__restrict__ off,
                                                         const uint32_t *__restrict__ idx,
                                                         const uint8_t *__restrict__ con, uint32_t n_dofs) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_dofs) return;
  double s = 0;
  for (uint32_t j = off[i]; j < off[i + 1]; ++j) s += local[idx[j]];
  dst[i] = (src && con[i]) ? src[i] : s;
}

// inv_diag[dof] = 1 / (sum of the dof's local diagonals); 1 on constrained and unreferenced dofs
__global__ void __launch_bounds__(256) qop_inv_diag_kernel(double *__restrict__ inv_diag, const double *__restrict__ local,
                                                           const uint32_t *__restrict__ off,
                                                           const uint32_t *__restrict__ idx, uint32_t n_dofs) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_dofs) return;
  const uint32_t b = off[i], e = off[i + 1];
  double s = 0;
  for (uint32_t j = b; j < e; ++j) s += local[idx[j]];
  inv_diag[i] = e > b ? 1.0 / s : 1.0;
}

// The folds of mfgpu_qop_set_coefficients, one thread per point; nullptr = leave that term alone.
struct FoldArgs {
  const double *jxw, *jinv;  // jinv nullptr: no gradient term (reaction only)
  const double *diff, *conv, *flux, *reac;  // the caller's real-space arrays
  double *o_diff, *o_conv, *o_flux, *o_reac;
  int general, diff_scalar_in, diff_scalar_out;
  uint32_t n_cells, nd;
};

template <int dim>
__global__ void __launch_bounds__(256) qop_fold_kernel(FoldArgs a) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)a.n_cells * a.nd) return;
  const uint32_t c = (uint32_t)(p / a.nd), q = (uint32_t)(p - (size_t)c * a.nd);
  const size_t c0 = (size_t)c * a.nd, nd = a.nd;
  const double w = a.jxw[p];
  if (a.reac) a.o_reac[p] = w * a.reac[p];
  if (!a.diff && !a.conv && !a.flux) return;
  double J[dim][dim];  // J^-1[e][k] = d xi_e / d x_k
#pragma unroll
  for (int e = 0; e < dim; ++e)
#pragma unroll
    for (int k = 0; k < dim; ++k)
      J[e][k] = a.general ? a.jinv[p * (dim * dim) + e * dim + k] : (e == k ? a.jinv[c] : 0.0);
  if (a.diff) {
    if (a.diff_scalar_out) {  // scalar a on uniform-J0: a J0^2 JxW
      a.o_diff[p] = w * J[0][0] * J[0][0] * a.diff[p];
    } else {
      double D[dim][dim];
#pragma unroll
      for (int k = 0; k < dim; ++k)
#pragma unroll
        for (int l = 0; l < dim; ++l)
          D[k][l] = a.diff_scalar_in ? (k == l ? a.diff[p] : 0.0) : a.diff[p * (dim * dim) + k * dim + l];
#pragma unroll
      for (int e = 0; e < dim; ++e) {
        double t[dim];  // (J^-1 D)[e][l]
#pragma unroll
        for (int l = 0; l < dim; ++l) {
          double s = 0;
#pragma unroll
          for (int k = 0; k < dim; ++k) s = fma(J[e][k], D[k][l], s);
          t[l] = s;
        }
#pragma unroll
        for (int f = 0; f < dim; ++f) {
          double s = 0;
#pragma unroll
          for (int l = 0; l < dim; ++l) s = fma(t[l], J[f][l], s);
          a.o_diff[c0 * (dim * dim) + (size_t)(e * dim + f) * nd + q] = w * s;
        }
      }
    }
  }
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const double *in = which ? a.flux : a.conv;
    double *out = which ? a.o_flux : a.o_conv;
    if (!in) continue;
    double b[dim];
#pragma unroll
    for (int k = 0; k < dim; ++k) b[k] = in[p * dim + k];
#pragma unroll
    for (int e = 0; e < dim; ++e) {
      double s = 0;
#pragma unroll
      for (int k = 0; k < dim; ++k) s = fma(J[e][k], b[k], s);
      out[c0 * dim + (size_t)e * nd + q] = w * s;
    }
  }
}

enum Which { INTEGRATE, APPLY, DIAG };

template <int dim, int N>
hipError_t launch_dn(Which w, const QopArgs &a, uint32_t n_cells, hipStream_t st) {
  const dim3 grid(n_cells), block(64);
  if (w == INTEGRATE) hipLaunchKernelGGL((integrate_cell_kernel<dim, N>), grid, block, 0, st, a);
  if (w == APPLY) hipLaunchKernelGGL((qop_cell_kernel<dim, N>), grid, block, 0, st, a);
  if (w == DIAG) hipLaunchKernelGGL((qop_diag_kernel<dim, N>), grid, block, 0, st, a);
  return hipGetLastError();
}

hipError_t launch(int dim, int n, Which w, const QopArgs &a, uint32_t n_cells, hipStream_t st) {
#define CASE(N)                                                                      \
  case N:                                                                            \
    return dim == 2 ? launch_dn<2, N>(w, a, n_cells, st) : launch_dn<3, N>(w, a, n_cells, st);
  switch (n) {
    CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7)
    default: return hipErrorInvalidValue;
  }
#undef CASE
}

QopArgs base_args(const IntegratorView &iv) {
  QopArgs a{};
  a.loc2glob = iv.loc2glob;
  a.cmask = iv.cmask;
  a.con = iv.con;
  a.tab = iv.tab;
  a.local = iv.local;
  a.jxw = iv.jxw;
  a.jinv = iv.jinv;
  a.general = iv.general ? 1 : 0;
  return a;
}

constexpr uint32_t kAllTerms = MFGPU_QOP_DIFFUSION_SCALAR | MFGPU_QOP_DIFFUSION_TENSOR | MFGPU_QOP_CONVECTION |
                               MFGPU_QOP_FLUX | MFGPU_QOP_REACTION;
constexpr uint32_t kDiffusion = MFGPU_QOP_DIFFUSION_SCALAR | MFGPU_QOP_DIFFUSION_TENSOR;

}  // namespace

int mfgpu_integrator_integrate(mfgpu_integrator *it, void *dst, const void *values_qp, const void *gradients_qp,
                               void *stream) {
  if (!it || !dst) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  if (!values_qp && !gradients_qp) return einval("mfgpu_integrator_integrate: values_qp and gradients_qp are both NULL");
  const IntegratorView iv = integrator_view(it);
  if (gradients_qp && !iv.updatable)
    return einval("mfgpu_integrator_integrate: gradients need inv_jac on the device; create the integrator with "
                  "MFGPU_UPDATABLE_COEFFICIENTS");
  hipStream_t st = (hipStream_t)stream;
  QopArgs a = base_args(iv);
  a.v = (const double *)values_qp;
  a.g = (const double *)gradients_qp;
  HIP_TRY(launch(iv.dim, iv.n, INTEGRATE, a, iv.n_cells, st));
  hipLaunchKernelGGL(qop_gather_kernel, dim3((iv.n_dofs + 255) / 256), dim3(256), 0, st, (double *)dst,
                     (const double *)nullptr, (const double *)iv.local, iv.rhs_off, iv.rhs_idx, iv.con, iv.n_dofs);
  HIP_TRY(hipGetLastError());
  return 0;
}

struct mfgpu_qop {
  IntegratorView iv{};
  uint32_t terms = 0, set = 0;  // MFGPU_QOP_* bits: requested, and given to set_coefficients at least once
  bool diff_scalar = false;     // the folded diffusion is one value per point (scalar a on uniform-J0)
  DeviceArray<double> d_diff, d_conv, d_flux, d_reac;
};

int mfgpu_qop_create(mfgpu_integrator *it, uint32_t terms, mfgpu_qop **out) {
  if (!it || !out) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  *out = nullptr;
  if (terms == 0 || (terms & ~kAllTerms)) return einval("mfgpu_qop_create: terms must be a non-empty set of MFGPU_QOP_* bits");
  if ((terms & kDiffusion) == kDiffusion)
    return einval("mfgpu_qop_create: MFGPU_QOP_DIFFUSION_SCALAR and MFGPU_QOP_DIFFUSION_TENSOR exclude each other");
  const IntegratorView iv = integrator_view(it);
  if ((terms & ~(uint32_t)MFGPU_QOP_REACTION) && !iv.updatable)
    return einval("mfgpu_qop_create: terms with a gradient need inv_jac on the device; create the integrator with "
                  "MFGPU_UPDATABLE_COEFFICIENTS");
  std::unique_ptr<mfgpu_qop> q(new mfgpu_qop());
  q->iv = iv;
  q->terms = terms;
  q->diff_scalar = (terms & MFGPU_QOP_DIFFUSION_SCALAR) && !iv.general;
  const size_t np = (size_t)iv.n_cells * (size_t)ipow(iv.n, iv.dim), dim = (size_t)iv.dim;
  int rc;
  if ((terms & kDiffusion) && (rc = q->d_diff.alloc(q->diff_scalar ? np : np * dim * dim))) return rc;
  if ((terms & MFGPU_QOP_CONVECTION) && (rc = q->d_conv.alloc(np * dim))) return rc;
  if ((terms & MFGPU_QOP_FLUX) && (rc = q->d_flux.alloc(np * dim))) return rc;
  if ((terms & MFGPU_QOP_REACTION) && (rc = q->d_reac.alloc(np))) return rc;
  *out = q.release();
  return 0;
}

int mfgpu_qop_set_coefficients(mfgpu_qop *q, const mfgpu_qop_coefficients *c, void *stream) {
  if (!q || !c) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  uint32_t given = 0;
  if (c->diffusion) given |= q->terms & kDiffusion ? q->terms & kDiffusion : kDiffusion;
  if (c->convection) given |= MFGPU_QOP_CONVECTION;
  if (c->flux) given |= MFGPU_QOP_FLUX;
  if (c->reaction) given |= MFGPU_QOP_REACTION;
  if (given & ~q->terms) return einval("mfgpu_qop_set_coefficients: a coefficient was given for a term the operator was created without");
  if (!given) return einval("mfgpu_qop_set_coefficients: every coefficient is NULL");
  const IntegratorView &iv = q->iv;
  FoldArgs a{};
  a.jxw = iv.jxw;
  a.jinv = iv.jinv;
  a.diff = (const double *)c->diffusion;
  a.conv = (const double *)c->convection;
  a.flux = (const double *)c->flux;
  a.reac = (const double *)c->reaction;
  a.o_diff = q->d_diff.get();
  a.o_conv = q->d_conv.get();
  a.o_flux = q->d_flux.get();
  a.o_reac = q->d_reac.get();
  a.general = iv.general ? 1 : 0;
  a.diff_scalar_in = (q->terms & MFGPU_QOP_DIFFUSION_SCALAR) ? 1 : 0;
  a.diff_scalar_out = q->diff_scalar ? 1 : 0;
  a.n_cells = iv.n_cells;
  a.nd = (uint32_t)ipow(iv.n, iv.dim);
  const size_t np = (size_t)a.n_cells * a.nd;
  const dim3 grid((unsigned)((np + 255) / 256)), block(256);
  if (iv.dim == 2) hipLaunchKernelGGL(qop_fold_kernel<2>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(qop_fold_kernel<3>, grid, block, 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  q->set |= given;
  return 0;
}

static int qop_args(const mfgpu_qop *q, const char *who, bool transpose, QopArgs &a) {
  if (q->set != q->terms) {
    set_error(std::string(who) + ": mfgpu_qop_set_coefficients has not set every term yet");
    return MFGPU_EINVAL;
  }
  a = base_args(q->iv);
  a.diff = q->d_diff.get();
  a.conv = transpose ? q->d_flux.get() : q->d_conv.get();
  a.flux = transpose ? q->d_conv.get() : q->d_flux.get();
  a.reac = q->d_reac.get();
  a.diff_scalar = q->diff_scalar ? 1 : 0;
  a.transpose = transpose ? 1 : 0;
  return 0;
}

int mfgpu_qop_vmult(mfgpu_qop *q, void *dst, const void *src, uint32_t flags, void *stream) {
  if (!q || !dst || !src) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  if (flags & ~(uint32_t)MFGPU_QOP_TRANSPOSE) return einval("mfgpu_qop_vmult: unknown flag");
  QopArgs a;
  if (const int rc = qop_args(q, "mfgpu_qop_vmult", (flags & MFGPU_QOP_TRANSPOSE) != 0, a)) return rc;
  a.src = (const double *)src;
  const IntegratorView &iv = q->iv;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(launch(iv.dim, iv.n, APPLY, a, iv.n_cells, st));
  hipLaunchKernelGGL(qop_gather_kernel, dim3((iv.n_dofs + 255) / 256), dim3(256), 0, st, (double *)dst,
                     (const double *)src, (const double *)iv.local, iv.rhs_off, iv.rhs_idx, iv.con, iv.n_dofs);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mfgpu_qop_compute_inverse_diagonal(mfgpu_qop *q, void *inv_diag, void *stream) {
  if (!q || !inv_diag) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  QopArgs a;
  if (const int rc = qop_args(q, "mfgpu_qop_compute_inverse_diagonal", false, a)) return rc;
  const IntegratorView &iv = q->iv;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(launch(iv.dim, iv.n, DIAG, a, iv.n_cells, st));
  hipLaunchKernelGGL(qop_inv_diag_kernel, dim3((iv.n_dofs + 255) / 256), dim3(256), 0, st, (double *)inv_diag,
                     (const double *)iv.local, iv.rhs_off, iv.rhs_idx, iv.n_dofs);
  HIP_TRY(hipGetLastError());
  return 0;
}

size_t mfgpu_qop_memory_consumption(const mfgpu_qop *q) {
  return q ? q->d_diff.bytes() + q->d_conv.bytes() + q->d_flux.bytes() + q->d_reac.bytes() : 0;
}

void mfgpu_qop_destroy(mfgpu_qop *q) { delete q; }

namespace mfgpu {
uint32_t qop_n_dofs(const mfgpu_qop *q) { return q->iv.n_dofs; }
}  // namespace mfgpu
