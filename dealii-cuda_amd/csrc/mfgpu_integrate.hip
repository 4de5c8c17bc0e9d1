// Cell integrals of a Poisson solve (include/mfgpu.h, "integrator"): the load vector with the Dirichlet lift of
// poisson.cu:182-221 and the L2 error of VectorTools::integrate_difference(..., QGauss(p+2), L2_norm),
// poisson.cu:277-292.  Double only (the reference's poisson uses `typedef double number`).  With a mass term in the
// description (mfgpu_desc.mass_coefficient) the lift also subtracts int c phi_i u_b.
//
// Structure: one wave64 workgroup per cell; every per-point array is cell-major, so a wave reads its cell contiguously.
// Inside the cell all tensor work is sum-factorised in LDS (tpass: one 1D contraction along one direction; a thread owns
// output entries).  Hanging-node resolution is the 1D pencil pass of mfgpu_cell.h (hn_pencil / hn_flag2 / hn_flag3) on
// LDS pencils, in the order of oracle/mf_oracle.py hn_resolve.
//   rhs:   cell kernel -> per-cell local vectors (scratch) -> per-dof gather over a host-built CSR (dof -> cell-major
//          local index, ascending), constrained and unreferenced dofs 0.  No atomics: bitwise repeatable.
//   error: cell kernel -> squared cell errors -> the two-stage fixed-order reduction of mfgpu_vec_dot.
//   evaluate: cell kernel -> values and real-space gradients of a field at the quadrature points, cell-major.
//   recovery indicator: nodal kernel (cell gradients as nodal coefficients, times |K|, to per-cell local buffers) ->
//          per-dof gather over a second CSR (unconstrained positions, Dirichlet dofs included), divided by the resident
//          denominator -> cell kernel (recovered minus cell gradient, integrated).  No atomics either.
// Geometry at the (p+2)^dim error points is interpolated from the description's QGauss(p+1) points with the 1D Lagrange
// basis on those points (values and derivatives): exact for mappings of degree <= p per direction (affine cells,
// MappingQ1, i.e. all mesh stand-ins).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mfgpu_integrate_cell.h"
#include "mfgpu_points.h"
#include "mfgpu_stream.h"
#include "mfgpu_transfer_build.h"

using namespace mfgpu;

namespace {

struct IntArgs {
  const uint32_t *loc2glob;  // [n_cells * N^dim]
  const uint32_t *cmask;     // [n_cells] or nullptr
  const double *tab;         // Tab<N>
  const double *qpts;        // [n_cells * N^dim * dim]
  const double *jxw;         // [n_cells * N^dim]
  const double *metric;      // uniform: [cell][q] a J0^2 JxW; general: [cell][e][q] symmetric a JxW J^-1 J^-T
  const double *mass;        // [cell][q] c JxW, or nullptr (no mass term)
  int general;
  // rhs
  const double *f_qp, *u_b;
  double *local;  // [n_cells * N^dim]
  // error
  const double *u, *exact;
  double *per_cell;
  double *points;  // error_points
  // evaluate
  const double *jinv;     // uniform: [n_cells] J0^-1; general: [n_cells * N^dim * dim * dim] row-major J^-1 per point
  double *values, *grads;  // [n_cells * N^dim], [n_cells * N^dim * dim]; either may be nullptr
  uint32_t n_cells;
};

// ---- Solution<dim> (poisson_common.cc:5-175) and RightHandSide<dim> (poisson_common.h:277-296), in double
template <int dim>
__device__ __forceinline__ double center(int i, int d) {
  if (dim == 2) {
    constexpr double c[3][2] = {{-0.5, +0.5}, {-0.5, -0.5}, {+0.5, -0.5}};
    return c[i][d];
  }
  constexpr double c[3][3] = {{-0.5, +0.5, 0.25}, {-0.6, -0.5, -0.125}, {+0.5, -0.5, 0.5}};
  return c[i][d];
}

template <int dim>
__device__ __forceinline__ double sol_norm() {
  const double s = sqrt(2 * M_PI) * (1. / 3.);
  return dim == 2 ? s * s : s * s * s;
}

template <int dim>
__device__ double solution_value(const double (&x)[dim]) {
  const double w = 1. / 3.;
  double r = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double n2 = 0;
#pragma unroll
    for (int d = 0; d < dim; ++d) {
      const double t = x[d] - center<dim>(i, d);
      n2 += t * t;
    }
    r += exp(-n2 / (w * w));
  }
  return r / sol_norm<dim>();
}

template <int dim>
__device__ double rhs_value(const double (&x)[dim]) {
  const double w = 1. / 3.;
  double lap = 0, grad[dim], xx = 0;
#pragma unroll
  for (int d = 0; d < dim; ++d) {
    grad[d] = 0;
    xx += x[d] * x[d];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double t[dim], n2 = 0;
#pragma unroll
    for (int d = 0; d < dim; ++d) {
      t[d] = x[d] - center<dim>(i, d);
      n2 += t[d] * t[d];
    }
    const double e = exp(-n2 / (w * w));
    lap += (-2 * dim + 4 * n2 / (w * w)) / (w * w) * e;
#pragma unroll
    for (int d = 0; d < dim; ++d) grad[d] += -2 / (w * w) * e * t[d];
  }
  lap /= sol_norm<dim>();
  // Coefficient<dim>::value / ::gradient (poisson_common.h:146-170)
  const double a = 1. / (0.05 + 2. * xx);
  const double den = 0.05 + 2. * xx;
  double ga_gu = 0;
#pragma unroll
  for (int d = 0; d < dim; ++d) ga_gu += (4. / (den * den)) * (-x[d]) * (grad[d] / sol_norm<dim>());
  return -(lap * a + ga_gu);
}


// rhs_i = int phi_i f - int grad phi_i . a grad u_b [- int c phi_i u_b]  (poisson.cu:198-214), hanging-node TRANSPOSE,
// to a.local
template <int dim, int N>
__global__ void __launch_bounds__(64) rhs_cell_kernel(IntArgs a) {
  constexpr int ND = cpow(N, dim);
  using TB = Tab<N>;
  __shared__ double tab[TB::size], A[ND], G[dim * ND], F[ND], LOC[ND], TO[ND], T1[ND], T2[ND];
  const uint32_t c = blockIdx.x;
  const size_t c0 = (size_t)c * ND;
  load_tab<N>(tab, a.tab);
  const unsigned mask = a.cmask ? a.cmask[c] : 0u;
  for (int q = threadIdx.x; q < ND; q += 64) {
    double f;
    if (a.f_qp) {
      f = a.f_qp[c0 + q];
    } else {
      double x[dim];
#pragma unroll
      for (int d = 0; d < dim; ++d) x[d] = a.qpts[(c0 + q) * dim + d];
      f = rhs_value<dim>(x);
    }
    F[q] = f * a.jxw[c0 + q];
    if (a.u_b) A[q] = a.u_b[a.loc2glob[c0 + q]];
  }
  const double *S = tab + TB::SE, *D = tab + TB::GE, *SI = tab + TB::SI, *GI = tab + TB::GI;
  tensor<dim, N, N>(F, LOC, SI, SI, SI, T1, T2);
  if (a.u_b) {
    if (mask) hn_resolve<dim, N, false>(A, mask, tab + TB::W);
    // reference gradients at the quadrature points
#pragma unroll
    for (int e = 0; e < dim; ++e) tensor<dim, N, N>(A, G + e * ND, e == 0 ? D : S, e == 1 ? D : S, e == 2 ? D : S, T1, T2);
    // flux in reference coordinates: a J0^2 JxW g, or (a JxW J^-1 J^-T) g
    for (int q = threadIdx.x; q < ND; q += 64) {
      if (!a.general) {
        const double m = a.metric[c0 + q];
#pragma unroll
        for (int e = 0; e < dim; ++e) G[e * ND + q] *= m;
      } else if (dim == 3) {
        const double *m = a.metric + c0 * 6 + q;
        const double g0 = G[q], g1 = G[ND + q], g2 = G[2 * ND + q];
        const double m00 = m[0], m01 = m[ND], m02 = m[2 * ND], m11 = m[3 * ND], m12 = m[4 * ND], m22 = m[5 * ND];
        G[q] = m00 * g0 + m01 * g1 + m02 * g2;
        G[ND + q] = m01 * g0 + m11 * g1 + m12 * g2;
        G[2 * ND + q] = m02 * g0 + m12 * g1 + m22 * g2;
      } else {
        const double *m = a.metric + c0 * 3 + q;
        const double g0 = G[q], g1 = G[ND + q];
        const double m00 = m[0], m01 = m[ND], m11 = m[2 * ND];
        G[q] = m00 * g0 + m01 * g1;
        G[ND + q] = m01 * g0 + m11 * g1;
      }
    }
#pragma unroll
    for (int e = 0; e < dim; ++e) {
      tensor<dim, N, N>(G + e * ND, TO, e == 0 ? GI : SI, e == 1 ? GI : SI, e == 2 ? GI : SI, T1, T2);
      for (int i = threadIdx.x; i < ND; i += 64) LOC[i] -= TO[i];
    }
    if (a.mass) {  // mass part of the lift: u_b at the quadrature points, times c JxW, integrated against phi_i
      tensor<dim, N, N>(A, G, S, S, S, T1, T2);
      for (int q = threadIdx.x; q < ND; q += 64) G[q] *= a.mass[c0 + q];
      tensor<dim, N, N>(G, TO, SI, SI, SI, T1, T2);
      for (int i = threadIdx.x; i < ND; i += 64) LOC[i] -= TO[i];
    }
  }
  if (mask) hn_resolve<dim, N, true>(LOC, mask, tab + TB::W);
  __syncthreads();
  for (int i = threadIdx.x; i < ND; i += 64) a.local[c0 + i] = LOC[i];
}

// rhs[dof] = sum of the dof's local entries in ascending (cell, local index) order; empty ranges (constrained or
// unreferenced dofs) give 0
__global__ void __launch_bounds__(256) rhs_gather_kernel(double *__restrict__ rhs, const double *__restrict__ local,
                                                         const uint32_t *__restrict__ off,
                                                         const uint32_t *__restrict__ idx, uint32_t n_dofs) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_dofs) return;
  double s = 0;
  for (uint32_t j = off[i]; j < off[i + 1]; ++j) s += local[idx[j]];
  rhs[i] = s;
}

// x (into X, dim x M^dim) and |det J| (into DET) at the error points of the cell whose QGauss(N) points are in Q
template <int dim, int N>
__device__ __forceinline__ void geometry(const double *tab, const double *Q, double *X, double *C1, double *DET,
                                         double *TO, double *T1, double *T2) {
  constexpr int ND = cpow(N, dim), M = N + 1, MD = cpow(M, dim);
  using TB = Tab<N>;
  const double *V = tab + TB::LV, *D = tab + TB::LD;
  // columns 0 and 1 of J = dx / dxi
#pragma unroll
  for (int d = 0; d < dim; ++d) {
    tensor<dim, N, M>(Q + d * ND, X + d * MD, D, V, V, T1, T2);
    tensor<dim, N, M>(Q + d * ND, C1 + d * MD, V, D, V, T1, T2);
  }
  if constexpr (dim == 2) {
    for (int k = threadIdx.x; k < MD; k += 64) DET[k] = fabs(X[k] * C1[MD + k] - X[MD + k] * C1[k]);
  } else {
    // det J = col2 . (col0 x col1); the cross product replaces col0 (the thread owns point k throughout)
    for (int k = threadIdx.x; k < MD; k += 64) {
      const double a0 = X[k], a1 = X[MD + k], a2 = X[2 * MD + k];
      const double b0 = C1[k], b1 = C1[MD + k], b2 = C1[2 * MD + k];
      X[k] = a1 * b2 - a2 * b1;
      X[MD + k] = a2 * b0 - a0 * b2;
      X[2 * MD + k] = a0 * b1 - a1 * b0;
      DET[k] = 0;
    }
#pragma unroll
    for (int d = 0; d < dim; ++d) {
      tensor<dim, N, M>(Q + d * ND, TO, V, V, D, T1, T2);
      for (int k = threadIdx.x; k < MD; k += 64) DET[k] += X[d * MD + k] * TO[k];
    }
    for (int k = threadIdx.x; k < MD; k += 64) DET[k] = fabs(DET[k]);
  }
#pragma unroll
  for (int d = 0; d < dim; ++d) tensor<dim, N, M>(Q + d * ND, X + d * MD, V, V, V, T1, T2);
  __syncthreads();
}


// squared L2 error of the cell on QGauss(N + 1) (VectorTools::integrate_difference, L2_norm)
template <int dim, int N>
__global__ void __launch_bounds__(64) l2_error_kernel(IntArgs a) {
  constexpr int ND = cpow(N, dim), M = N + 1, MD = cpow(M, dim);
  using TB = Tab<N>;
  __shared__ double tab[TB::size], A[ND], U[MD], Q[dim * ND], X[dim * MD], C1[dim * MD], DET[MD], TO[MD], T1[MD],
      T2[MD];
  const uint32_t c = blockIdx.x;
  const size_t c0 = (size_t)c * ND;
  load_tab<N>(tab, a.tab);
  for (int i = threadIdx.x; i < ND; i += 64) A[i] = a.u[a.loc2glob[c0 + i]];
  load_qpts<dim, N>(Q, a.qpts, c);
  const unsigned mask = a.cmask ? a.cmask[c] : 0u;
  if (mask) hn_resolve<dim, N, false>(A, mask, tab + TB::W);
  const double *E = tab + TB::E;
  tensor<dim, N, M>(A, U, E, E, E, T1, T2);
  geometry<dim, N>(tab, Q, X, C1, DET, TO, T1, T2);
  double acc = 0;
  for (int k = threadIdx.x; k < MD; k += 64) {
    double ex;
    if (a.exact) {
      ex = a.exact[(size_t)c * MD + k];
    } else {
      double x[dim];
#pragma unroll
      for (int d = 0; d < dim; ++d) x[d] = X[d * MD + k];
      ex = solution_value<dim>(x);
    }
    const int kx = k % M, ky = (k / M) % M, kz = k / (M * M);
    double w = tab[TB::WM + kx] * tab[TB::WM + ky];
    if (dim == 3) w *= tab[TB::WM + kz];
    const double diff = U[k] - ex;
    acc += diff * diff * (w * DET[k]);
  }
  acc = wave_sum(acc);
  if (threadIdx.x == 0) a.per_cell[c] = acc;
}

template <int dim, int N>
__global__ void __launch_bounds__(64) error_points_kernel(IntArgs a) {
  constexpr int ND = cpow(N, dim), M = N + 1, MD = cpow(M, dim);
  using TB = Tab<N>;
  __shared__ double tab[TB::size], Q[dim * ND], X[dim * MD], C1[dim * MD], DET[MD], TO[MD], T1[MD], T2[MD];
  const uint32_t c = blockIdx.x;
  load_tab<N>(tab, a.tab);
  load_qpts<dim, N>(Q, a.qpts, c);
  geometry<dim, N>(tab, Q, X, C1, DET, TO, T1, T2);
  for (int t = threadIdx.x; t < MD * dim; t += 64) {
    const int k = t / dim, d = t - k * dim;
    a.points[(size_t)c * MD * dim + t] = X[d * MD + k];
  }
}

// u and grad u at the quadrature points (the read_dof_values + evaluate + get_value / get_gradient half of
// FEEvaluationGpu, fee_gpu.cuh:155-281): nodal values through loc2glob, hanging-node interpolation, sum-factorised
// values and reference gradients, then grad_x = J^-T grad_xi per point (uniform: J0^-1 grad_xi).  Every output entry
// is written by exactly one thread.
template <int dim, int N>
__global__ void __launch_bounds__(64) evaluate_cell_kernel(IntArgs a) {
  constexpr int ND = cpow(N, dim);
  using TB = Tab<N>;
  __shared__ double tab[TB::size], A[ND], G[dim * ND], T1[ND], T2[ND];
  const uint32_t c = blockIdx.x;
  const size_t c0 = (size_t)c * ND;
  load_tab<N>(tab, a.tab);
  for (int i = threadIdx.x; i < ND; i += 64) A[i] = a.u[a.loc2glob[c0 + i]];
  const unsigned mask = a.cmask ? a.cmask[c] : 0u;
  if (mask) hn_resolve<dim, N, false>(A, mask, tab + TB::W);
  const double *S = tab + TB::SE, *D = tab + TB::GE;
  if (a.values) {
    tensor<dim, N, N>(A, G, S, S, S, T1, T2);
    for (int q = threadIdx.x; q < ND; q += 64) a.values[c0 + q] = G[q];
  }
  if (!a.grads) return;
#pragma unroll
  for (int e = 0; e < dim; ++e) tensor<dim, N, N>(A, G + e * ND, e == 0 ? D : S, e == 1 ? D : S, e == 2 ? D : S, T1, T2);
  const double j0 = a.general ? 0.0 : a.jinv[c];
  for (int q = threadIdx.x; q < ND; q += 64) {
    double g[dim], r[dim];
#pragma unroll
    for (int e = 0; e < dim; ++e) g[e] = G[e * ND + q];
    if (!a.general) {
#pragma unroll
      for (int k = 0; k < dim; ++k) r[k] = j0 * g[k];
    } else {
      const double *J = a.jinv + (c0 + q) * (dim * dim);  // J^-1[e][k] = d xi_e / d x_k
#pragma unroll
      for (int k = 0; k < dim; ++k) {
        double s = 0;
#pragma unroll
        for (int e = 0; e < dim; ++e) s = fma(J[e * dim + k], g[e], s);
        r[k] = s;
      }
    }
#pragma unroll
    for (int k = 0; k < dim; ++k) a.grads[(c0 + q) * dim + k] = r[k];
  }
}

// ---- gradient-recovery indicator (include/mfgpu.h, mfgpu_integrator_recovery_indicator)
struct IndArgs {
  const uint32_t *loc2glob, *cmask;
  const double *tab;     // Tab<N>
  const double *sinv;    // [i][q] inverse of Tab<N>::SE
  const double *jxw;     // [n_cells * N^dim]
  const double *jinv;    // as IntArgs::jinv
  const double *vol;     // [n_cells] |K|
  const double *u;       // [n_dofs]
  const double *weight;  // [n_cells * N^dim] or nullptr
  double *local;         // dim buffers [n_cells * N^dim], component k at k * local_stride
  double *nodal;         // dim vectors [n_dofs], component k at k * n_dofs
  double *per_cell;      // [n_cells]
  size_t local_stride;
  uint32_t n_dofs;
  int general;
};

// A = u at the cell's nodes (gathered, hanging-node interpolated); G[e * ND + q] = component e of the real-space
// gradient at quadrature point q, by the steps of evaluate_cell_kernel
template <int dim, int N>
__device__ __forceinline__ void cell_gradient(const IndArgs &a, uint32_t c, unsigned mask, const double *tab, double *A,
                                              double *G, double *T1, double *T2) {
  constexpr int ND = cpow(N, dim);
  using TB = Tab<N>;
  const size_t c0 = (size_t)c * ND;
  for (int i = threadIdx.x; i < ND; i += 64) A[i] = a.u[a.loc2glob[c0 + i]];
  if (mask) hn_resolve<dim, N, false>(A, mask, tab + TB::W);
  const double *S = tab + TB::SE, *D = tab + TB::GE;
#pragma unroll
  for (int e = 0; e < dim; ++e) tensor<dim, N, N>(A, G + e * ND, e == 0 ? D : S, e == 1 ? D : S, e == 2 ? D : S, T1, T2);
  const double j0 = a.general ? 0.0 : a.jinv[c];
  for (int q = threadIdx.x; q < ND; q += 64) {  // the thread owns point q: in place
    double g[dim], r[dim];
#pragma unroll
    for (int e = 0; e < dim; ++e) g[e] = G[e * ND + q];
    if (!a.general) {
#pragma unroll
      for (int k = 0; k < dim; ++k) r[k] = j0 * g[k];
    } else {
      const double *J = a.jinv + (c0 + q) * (dim * dim);  // J^-1[e][k] = d xi_e / d x_k
#pragma unroll
      for (int k = 0; k < dim; ++k) {
        double s = 0;
#pragma unroll
        for (int e = 0; e < dim; ++e) s = fma(J[e * dim + k], g[e], s);
        r[k] = s;
      }
    }
#pragma unroll
    for (int k = 0; k < dim; ++k) G[k * ND + q] = r[k];
  }
  __syncthreads();
}

// step a and the products of step b: local[k][cell][i] = |K| g_K,i of component k.  Entries at constrained positions
// are written like the others; the gather's index list leaves them out.
template <int dim, int N>
__global__ void __launch_bounds__(64) indicator_nodal_kernel(IndArgs a) {
  constexpr int ND = cpow(N, dim);
  using TB = Tab<N>;
  __shared__ double tab[TB::size], SINV[N * N], A[ND], G[dim * ND], TO[ND], T1[ND], T2[ND];
  const uint32_t c = blockIdx.x;
  const size_t c0 = (size_t)c * ND;
  load_tab<N>(tab, a.tab);
  for (int i = threadIdx.x; i < N * N; i += 64) SINV[i] = a.sinv[i];
  const unsigned mask = a.cmask ? a.cmask[c] : 0u;
  cell_gradient<dim, N>(a, c, mask, tab, A, G, T1, T2);
  const double vol = a.vol[c];
#pragma unroll
  for (int k = 0; k < dim; ++k) {
    tensor<dim, N, N>(G + k * ND, TO, SINV, SINV, SINV, T1, T2);
    for (int i = threadIdx.x; i < ND; i += 64) a.local[k * a.local_stride + c0 + i] = vol * TO[i];
  }
}

// step b: nodal[k][dof] = (sum of the dof's local entries of component k, ascending (cell, local index)) / den[dof];
// 0 for a dof without entries
__global__ void __launch_bounds__(256) indicator_gather_kernel(double *__restrict__ nodal, const double *__restrict__ local,
                                                               const double *__restrict__ den,
                                                               const uint32_t *__restrict__ off,
                                                               const uint32_t *__restrict__ idx, uint32_t n_dofs,
                                                               size_t local_stride) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_dofs) return;
  const uint32_t b = off[i], e = off[i + 1];
  const double *l = local + blockIdx.y * local_stride;
  double s = 0;
  for (uint32_t j = b; j < e; ++j) s += l[idx[j]];
  nodal[(size_t)blockIdx.y * n_dofs + i] = e > b ? s / den[i] : 0.0;
}

// step c: per_cell[cell] = sum_q weight_q |G(x_q) - grad u_h(x_q)|^2 JxW_q
template <int dim, int N>
__global__ void __launch_bounds__(64) indicator_cell_kernel(IndArgs a) {
  constexpr int ND = cpow(N, dim);
  using TB = Tab<N>;
  __shared__ double tab[TB::size], A[ND], G[dim * ND], B[ND], V[ND], T1[ND], T2[ND];
  const uint32_t c = blockIdx.x;
  const size_t c0 = (size_t)c * ND;
  load_tab<N>(tab, a.tab);
  const unsigned mask = a.cmask ? a.cmask[c] : 0u;
  cell_gradient<dim, N>(a, c, mask, tab, A, G, T1, T2);
  const double *S = tab + TB::SE;
#pragma unroll
  for (int k = 0; k < dim; ++k) {
    for (int i = threadIdx.x; i < ND; i += 64) B[i] = a.nodal[(size_t)k * a.n_dofs + a.loc2glob[c0 + i]];
    if (mask) hn_resolve<dim, N, false>(B, mask, tab + TB::W);
    tensor<dim, N, N>(B, V, S, S, S, T1, T2);
    for (int q = threadIdx.x; q < ND; q += 64) {  // the thread owns point q
      const double diff = V[q] - G[k * ND + q];
      G[k * ND + q] = diff * diff;
    }
  }
  double acc = 0;
  for (int q = threadIdx.x; q < ND; q += 64) {
    double s = G[q];
#pragma unroll
    for (int k = 1; k < dim; ++k) s += G[k * ND + q];
    const double w = a.weight ? a.weight[c0 + q] * a.jxw[c0 + q] : a.jxw[c0 + q];
    acc += s * w;
  }
  acc = wave_sum(acc);
  if (threadIdx.x == 0) a.per_cell[c] = acc;
}

template <int dim, int N>
hipError_t launch_indicator_dn(bool nodal, const IndArgs &a, uint32_t n_cells, hipStream_t st) {
  if (nodal) hipLaunchKernelGGL((indicator_nodal_kernel<dim, N>), dim3(n_cells), dim3(64), 0, st, a);
  else hipLaunchKernelGGL((indicator_cell_kernel<dim, N>), dim3(n_cells), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_indicator(int dim, int n, bool nodal, const IndArgs &a, uint32_t n_cells, hipStream_t st) {
#define CASE(N)                                                                                                      \
  case N:                                                                                                            \
    return dim == 2 ? launch_indicator_dn<2, N>(nodal, a, n_cells, st) : launch_indicator_dn<3, N>(nodal, a, n_cells, st);
  switch (n) {
    CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7)
    default: return hipErrorInvalidValue;
  }
#undef CASE
}

// inverse of the n x n row-major matrix m, Gauss-Jordan with partial pivoting in long double; false if singular
bool invert_table(int n, const double *m, std::vector<double> &inv) {
  std::vector<long double> a((size_t)n * 2 * n, 0.0L);
  for (int r = 0; r < n; ++r) {
    for (int c = 0; c < n; ++c) a[r * 2 * n + c] = m[r * n + c];
    a[r * 2 * n + n + r] = 1.0L;
  }
  for (int k = 0; k < n; ++k) {
    int piv = k;
    for (int r = k + 1; r < n; ++r)
      if (fabsl(a[r * 2 * n + k]) > fabsl(a[piv * 2 * n + k])) piv = r;
    if (a[piv * 2 * n + k] == 0.0L) return false;
    if (piv != k)
      for (int c = 0; c < 2 * n; ++c) std::swap(a[k * 2 * n + c], a[piv * 2 * n + c]);
    const long double d = a[k * 2 * n + k];
    for (int c = 0; c < 2 * n; ++c) a[k * 2 * n + c] /= d;
    for (int r = 0; r < n; ++r) {
      if (r == k) continue;
      const long double f = a[r * 2 * n + k];
      if (f == 0.0L) continue;
      for (int c = 0; c < 2 * n; ++c) a[r * 2 * n + c] -= f * a[k * 2 * n + c];
    }
  }
  inv.assign((size_t)n * n, 0.0);
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) inv[r * n + c] = (double)a[r * 2 * n + n + c];
  return true;
}

enum Which { RHS, L2, POINTS, EVAL };

template <int dim, int N>
hipError_t launch_dn(Which w, const IntArgs &a, hipStream_t st) {
  const dim3 grid(a.n_cells), block(64);
  if (w == RHS) hipLaunchKernelGGL((rhs_cell_kernel<dim, N>), grid, block, 0, st, a);
  if (w == L2) hipLaunchKernelGGL((l2_error_kernel<dim, N>), grid, block, 0, st, a);
  if (w == POINTS) hipLaunchKernelGGL((error_points_kernel<dim, N>), grid, block, 0, st, a);
  if (w == EVAL) hipLaunchKernelGGL((evaluate_cell_kernel<dim, N>), grid, block, 0, st, a);
  return hipGetLastError();
}

hipError_t launch(int dim, int n, Which w, const IntArgs &a, hipStream_t st) {
#define CASE(N)                                                                      \
  case N:                                                                            \
    return dim == 2 ? launch_dn<2, N>(w, a, st) : launch_dn<3, N>(w, a, st);
  switch (n) {
    CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7)
    default: return hipErrorInvalidValue;
  }
#undef CASE
}

// Gauss-Legendre points and weights on [0,1], ascending
void gauss_01(int m, std::vector<double> &x, std::vector<double> &w) {
  x.assign(m, 0.0);
  w.assign(m, 0.0);
  for (int i = 0; i < m; ++i) {
    double z = std::cos(M_PI * (i + 0.75) / (m + 0.5)), dp = 1;
    for (int it = 0; it < 100; ++it) {
      double p0 = 1, p1 = z;
      for (int k = 2; k <= m; ++k) {
        const double p2 = ((2 * k - 1) * z * p1 - (k - 1) * p0) / k;
        p0 = p1;
        p1 = p2;
      }
      dp = m * (z * p1 - p0) / (z * z - 1);
      const double dz = p1 / dp;
      z -= dz;
      if (std::fabs(dz) < 1e-16) break;
    }
    x[m - 1 - i] = 0.5 * (z + 1);
    w[m - 1 - i] = 1.0 / ((1 - z * z) * dp * dp);  // 2 / ((1 - z^2) P'^2) on [-1,1], halved
  }
}

// l[j] = L_j(y), dl[j] = L_j'(y) for the Lagrange basis on `nodes`
void lagrange(const std::vector<double> &nodes, double y, std::vector<double> &l, std::vector<double> &dl) {
  const int n = (int)nodes.size();
  l.assign(n, 0.0);
  dl.assign(n, 0.0);
  for (int j = 0; j < n; ++j) {
    double den = 1, v = 1, d = 0;
    for (int k = 0; k < n; ++k) {
      if (k == j) continue;
      den *= nodes[j] - nodes[k];
      v *= y - nodes[k];
      double t = 1;
      for (int m = 0; m < n; ++m)
        if (m != j && m != k) t *= y - nodes[m];
      d += t;
    }
    l[j] = v / den;
    dl[j] = d / den;
  }
}

}  // namespace

struct mfgpu_integrator {
  int dim = 0, n = 0;
  bool general = false;
  uint32_t n_cells = 0, n_dofs = 0;
  DeviceArray<uint32_t> d_l2g, d_cmask, d_off, d_idx;
  DeviceArray<uint8_t> d_con;  // [n_dofs] 1 on a constrained dof (mfgpu_qop.hip: src mask and identity rows)
  DeviceArray<double> d_tab, d_qpts, d_jxw, d_metric, d_mass;
  DeviceArray<double> d_local, d_err, d_ones;
  // MFGPU_UPDATABLE_COEFFICIENTS: inv_jac and the (identity) cell order of the folds stay on the device -- what
  // mfgpu_integrator_update_coefficients and the gradients of mfgpu_integrator_evaluate read (JxW: d_jxw)
  bool updatable = false;
  FoldGeometry geo;
  // mfgpu_integrator_recovery_indicator (updatable integrators): the inverse 1D table, |K|, the CSR over unconstrained
  // positions and the denominator from creation; the local buffers and nodal vectors from the first call
  DeviceArray<uint32_t> d_ind_off, d_ind_idx;
  DeviceArray<double> d_sinv, d_vol, d_den, d_ind_local, d_ind_nodal;
};

void mfgpu_integrator_destroy(mfgpu_integrator *it) { delete it; }

// what a points object (mfgpu_points.hip) borrows: pointers into this integrator's device arrays
IntegratorView mfgpu::integrator_view(const mfgpu_integrator *it) {
  IntegratorView v{};
  v.dim = it->dim;
  v.n = it->n;
  v.general = it->general;
  v.n_cells = it->n_cells;
  v.n_dofs = it->n_dofs;
  v.loc2glob = it->d_l2g.get();
  v.cmask = it->d_cmask.get();
  v.rhs_off = it->d_off.get();
  v.tab = it->d_tab.get();
  v.qpts = it->d_qpts.get();
  v.updatable = it->updatable;
  v.rhs_idx = it->d_idx.get();
  v.con = it->d_con.get();
  v.jxw = it->d_jxw.get();
  v.jinv = it->updatable ? it->geo.jinv.as<const double>() : nullptr;
  v.local = it->d_local.get();
  return v;
}

static int integrator_setup(mfgpu_integrator *it, const mfgpu_desc &d) {
  const int dim = d.dim, n = d.degree + 1, m = n + 1;
  const size_t nc = d.n_cells, nd = (size_t)ipow(n, dim);
  it->dim = dim;
  it->n = n;
  it->n_cells = d.n_cells;
  it->n_dofs = d.n_dofs;
  it->general = !(d.flags & MFGPU_UNIFORM_J0);
  const bool hn = (d.flags & MFGPU_HANGING_NODES) && d.constraint_mask;
  // tables (layout Tab<N>)
  const double *sv = (const double *)d.shape_values, *sg = (const double *)d.shape_gradients;
  std::vector<double> xq, wq, ym, wm;
  gauss_01(n, xq, wq);
  gauss_01(m, ym, wm);
  std::vector<double> tab;
  for (int q = 0; q < n; ++q)
    for (int i = 0; i < n; ++i) tab.push_back(sv[i * n + q]);
  for (int q = 0; q < n; ++q)
    for (int i = 0; i < n; ++i) tab.push_back(sg[i * n + q]);
  tab.insert(tab.end(), sv, sv + n * n);
  tab.insert(tab.end(), sg, sg + n * n);
  std::vector<std::vector<double>> L(m), DL(m);
  for (int k = 0; k < m; ++k) lagrange(xq, ym[k], L[k], DL[k]);
  for (int k = 0; k < m; ++k)  // phi_i(y_k) = sum_q L_q(y_k) phi_i(x_q): the degree-p shape function through its values
    for (int i = 0; i < n; ++i) {
      double s = 0;
      for (int q = 0; q < n; ++q) s += L[k][q] * sv[i * n + q];
      tab.push_back(s);
    }
  for (int k = 0; k < m; ++k) tab.insert(tab.end(), L[k].begin(), L[k].end());
  for (int k = 0; k < m; ++k) tab.insert(tab.end(), DL[k].begin(), DL[k].end());
  tab.insert(tab.end(), wm.begin(), wm.end());
  for (int i = 0; i < n * n; ++i) tab.push_back(hn ? d.constraint_weights[i] : 0.0);
  int rc;
  if ((rc = it->d_tab.upload(tab.data(), tab.size()))) return rc;
  if ((rc = it->d_l2g.upload(d.loc2glob, nc * nd))) return rc;
  if (hn && (rc = it->d_cmask.upload(d.constraint_mask, nc))) return rc;
  if ((rc = it->d_qpts.upload(d.quadrature_points, nc * nd * dim))) return rc;
  if ((rc = it->d_jxw.upload(d.JxW, nc * nd))) return rc;
  // dof -> (cell, local index) CSR, constrained dofs left empty
  std::vector<uint8_t> con(d.n_dofs, 0);
  for (uint32_t i = 0; i < d.n_constrained; ++i) con[d.constrained_dofs[i]] = 1;
  std::vector<uint32_t> off(d.n_dofs + 1, 0);
  for (size_t j = 0; j < nc * nd; ++j)
    if (!con[d.loc2glob[j]]) ++off[d.loc2glob[j] + 1];
  for (uint32_t i = 0; i < d.n_dofs; ++i) off[i + 1] += off[i];
  std::vector<uint32_t> idx(off[d.n_dofs]), pos(off.begin(), off.end() - 1);
  for (size_t j = 0; j < nc * nd; ++j)
    if (!con[d.loc2glob[j]]) idx[pos[d.loc2glob[j]]++] = (uint32_t)j;
  if ((rc = it->d_off.upload(off.data(), off.size()))) return rc;
  if ((rc = it->d_idx.upload(idx.data(), idx.size()))) return rc;
  if ((rc = it->d_con.upload(con.data(), con.size()))) return rc;
  if ((rc = it->d_local.alloc(nc * nd))) return rc;
  if ((rc = it->d_err.alloc(nc))) return rc;
  std::vector<double> ones(nc, 1.0);
  if ((rc = it->d_ones.upload(ones.data(), nc))) return rc;
  // coefficient (given, or evaluated from the quadrature points) folded with JxW and the inverse Jacobian by the
  // operator's own set-up (cell order = identity, JxW = the resident d_jxw); it uploads the quadrature points again as
  // its temporary rather than take the resident d_qpts
  std::vector<uint32_t> order(nc);
  for (size_t c = 0; c < nc; ++c) order[c] = (uint32_t)c;
  it->updatable = (d.flags & MFGPU_UPDATABLE_COEFFICIENTS) != 0;
  FoldGeometry geo;
  if ((rc = geo.upload(nullptr, d.inv_jac, order.data(), dim, (uint32_t)nc, (uint32_t)nd, it->general, MFGPU_F64)))
    return rc;
  const FoldInputs<double> in = geo.inputs<double>(it->d_jxw.get());
  if ((rc = fold_coefficient<double>(it->d_metric, d.coefficient, d.quadrature_points, in))) return rc;
  if (d.mass_coefficient && (rc = fold_mass<double>(it->d_mass, d.mass_coefficient, in))) return rc;
  if (it->updatable) it->geo = std::move(geo);
  if (it->updatable) {
    std::vector<double> se, sinv;  // [q][i] = phi_i(x_q) and its inverse
    for (int q = 0; q < n; ++q)
      for (int i = 0; i < n; ++i) se.push_back(sv[i * n + q]);
    if (!invert_table(n, se.data(), sinv)) {
      set_error("mfgpu_integrator: shape_values is singular");
      return MFGPU_EINVAL;
    }
    std::vector<double> vol(nc, 0.0), den(d.n_dofs, 0.0);
    for (size_t c = 0; c < nc; ++c)
      for (size_t q = 0; q < nd; ++q) vol[c] += ((const double *)d.JxW)[c * nd + q];
    std::vector<uint32_t> ioff(d.n_dofs + 1, 0);
    auto listed = [&](size_t j) { return !hn || !constrained_position(dim, n, d.constraint_mask[j / nd], (int)(j % nd)); };
    for (size_t j = 0; j < nc * nd; ++j)
      if (listed(j)) ++ioff[d.loc2glob[j] + 1];
    for (uint32_t i = 0; i < d.n_dofs; ++i) ioff[i + 1] += ioff[i];
    std::vector<uint32_t> iidx(ioff[d.n_dofs]), ipos(ioff.begin(), ioff.end() - 1);
    for (size_t j = 0; j < nc * nd; ++j)
      if (listed(j)) {
        iidx[ipos[d.loc2glob[j]]++] = (uint32_t)j;
        den[d.loc2glob[j]] += vol[j / nd];
      }
    if ((rc = it->d_sinv.upload(sinv.data(), sinv.size()))) return rc;
    if ((rc = it->d_vol.upload(vol.data(), vol.size()))) return rc;
    if ((rc = it->d_den.upload(den.data(), den.size()))) return rc;
    if ((rc = it->d_ind_off.upload(ioff.data(), ioff.size()))) return rc;
    if ((rc = it->d_ind_idx.upload(iidx.data(), iidx.size()))) return rc;
  }
  return 0;
}

int mfgpu_integrator_create(const mfgpu_desc *desc, mfgpu_integrator **out) {
  if (!desc || !out) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  *out = nullptr;
  const mfgpu_desc &d = *desc;
  if (d.number_type == MFGPU_F32) {
    set_error("mfgpu_integrator: MFGPU_F64 only (the reference's poisson uses double)");
    return MFGPU_EUNSUPPORTED;
  }
  if (d.number_type != MFGPU_F64) {
    set_error("number_type must be MFGPU_F64");
    return MFGPU_EINVAL;
  }
  if ((d.dim != 2 && d.dim != 3) || d.degree < 1 || d.degree > 6) {
    set_error("mfgpu_integrator: dim 2 or 3, degree 1..6");
    return MFGPU_EUNSUPPORTED;
  }
  if (!d.quadrature_points) {
    set_error("mfgpu_integrator: quadrature_points are required (right-hand side, error-point geometry)");
    return MFGPU_EINVAL;
  }
  if (!d.loc2glob || !d.JxW || !d.inv_jac || !d.shape_values || !d.shape_gradients || d.n_cells == 0 ||
      (d.n_constrained && !d.constrained_dofs)) {
    set_error("mfgpu_integrator: loc2glob, JxW, inv_jac, shape tables and cells are required");
    return MFGPU_EINVAL;
  }
  if ((d.flags & MFGPU_HANGING_NODES) && (!d.constraint_mask || !d.constraint_weights)) {
    set_error("MFGPU_HANGING_NODES needs constraint_mask and constraint_weights");
    return MFGPU_EINVAL;
  }
  const size_t nd = (size_t)ipow(d.degree + 1, d.dim);
  for (size_t j = 0; j < (size_t)d.n_cells * nd; ++j)
    if (d.loc2glob[j] >= d.n_dofs) {
      set_error("loc2glob entry out of range");
      return MFGPU_EINVAL;
    }
  for (uint32_t i = 0; i < d.n_constrained; ++i)
    if (d.constrained_dofs[i] >= d.n_dofs) {
      set_error("constrained dof out of range");
      return MFGPU_EINVAL;
    }
  std::unique_ptr<mfgpu_integrator> it(new mfgpu_integrator());
  if (const int rc = integrator_setup(it.get(), d)) return rc;
  *out = it.release();
  return 0;
}

static IntArgs base_args(const mfgpu_integrator *it) {
  IntArgs a{};
  a.loc2glob = it->d_l2g.get();
  a.cmask = it->d_cmask.get();
  a.tab = it->d_tab.get();
  a.qpts = it->d_qpts.get();
  a.jxw = it->d_jxw.get();
  a.metric = it->d_metric.get();
  a.mass = it->d_mass.get();
  a.general = it->general ? 1 : 0;
  a.n_cells = it->n_cells;
  return a;
}

int mfgpu_integrator_rhs(mfgpu_integrator *it, void *rhs, const void *f_qp, const void *u_b, void *stream) {
  if (!it || !rhs) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  IntArgs a = base_args(it);
  a.f_qp = (const double *)f_qp;
  a.u_b = (const double *)u_b;
  a.local = it->d_local.get();
  HIP_TRY(launch(it->dim, it->n, RHS, a, st));
  hipLaunchKernelGGL(rhs_gather_kernel, dim3((it->n_dofs + 255) / 256), dim3(256), 0, st, (double *)rhs,
                     (const double *)it->d_local.get(), it->d_off.get(), it->d_idx.get(), it->n_dofs);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mfgpu_integrator_l2_error(mfgpu_integrator *it, const void *u, const void *exact, void *per_cell, void *stream,
                              double *l2) {
  if (!it || !u || !l2) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  IntArgs a = base_args(it);
  a.u = (const double *)u;
  a.exact = (const double *)exact;
  a.per_cell = per_cell ? (double *)per_cell : it->d_err.get();
  HIP_TRY(launch(it->dim, it->n, L2, a, st));
  double sum = 0;
  HIP_TRY(vec_reduce_launch<double>(0, a.per_cell, nullptr, it->d_ones.get(), 0.0, it->n_cells, st, &sum));
  *l2 = std::sqrt(sum);
  return 0;
}

int mfgpu_integrator_error_points(mfgpu_integrator *it, void *points, void *stream) {
  if (!it || !points) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  IntArgs a = base_args(it);
  a.points = (double *)points;
  HIP_TRY(launch(it->dim, it->n, POINTS, a, (hipStream_t)stream));
  return 0;
}

int mfgpu_integrator_update_coefficients(mfgpu_integrator *it, const void *coefficient_dev,
                                         const void *mass_coefficient_dev, void *stream) {
  if (!it) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  if (!it->updatable) {
    set_error("mfgpu_integrator_update_coefficients: the integrator was created without MFGPU_UPDATABLE_COEFFICIENTS");
    return MFGPU_EINVAL;
  }
  if (!coefficient_dev && !mass_coefficient_dev) {
    set_error("mfgpu_integrator_update_coefficients: coefficient_dev and mass_coefficient_dev are both NULL");
    return MFGPU_EINVAL;
  }
  if (mass_coefficient_dev && !it->d_mass.get()) {
    set_error("mfgpu_integrator_update_coefficients: the integrator was created without a mass term");
    return MFGPU_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const FoldInputs<double> in = it->geo.inputs<double>(it->d_jxw.get());
  if (coefficient_dev) HIP_TRY(fold_coefficient_launch<double>(it->d_metric.get(), (const double *)coefficient_dev, in, st));
  if (mass_coefficient_dev) HIP_TRY(fold_mass_launch<double>(it->d_mass.get(), (const double *)mass_coefficient_dev, in, st));
  return 0;
}

int mfgpu_integrator_evaluate(mfgpu_integrator *it, const void *u, void *values_qp, void *gradients_qp, void *stream) {
  if (!it || !u) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  if (!values_qp && !gradients_qp) {
    set_error("mfgpu_integrator_evaluate: values_qp and gradients_qp are both NULL");
    return MFGPU_EINVAL;
  }
  if (gradients_qp && !it->updatable) {
    set_error("mfgpu_integrator_evaluate: gradients need inv_jac on the device; create the integrator with "
              "MFGPU_UPDATABLE_COEFFICIENTS");
    return MFGPU_EINVAL;
  }
  IntArgs a = base_args(it);
  a.u = (const double *)u;
  a.jinv = it->geo.jinv.as<const double>();
  a.values = (double *)values_qp;
  a.grads = (double *)gradients_qp;
  HIP_TRY(launch(it->dim, it->n, EVAL, a, (hipStream_t)stream));
  return 0;
}

int mfgpu_integrator_recovery_indicator(mfgpu_integrator *it, const void *u, const void *weight_qp, void *per_cell,
                                        void *stream) {
  if (!it || !u || !per_cell) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  if (!it->updatable) {
    set_error("mfgpu_integrator_recovery_indicator: gradients need inv_jac on the device; create the integrator with "
              "MFGPU_UPDATABLE_COEFFICIENTS");
    return MFGPU_EINVAL;
  }
  const size_t local_stride = (size_t)it->n_cells * (size_t)ipow(it->n, it->dim);
  int rc;
  if (!it->d_ind_local.get() && (rc = it->d_ind_local.alloc(local_stride * it->dim))) return rc;
  if (!it->d_ind_nodal.get() && (rc = it->d_ind_nodal.alloc((size_t)it->n_dofs * it->dim))) return rc;
  hipStream_t st = (hipStream_t)stream;
  IndArgs a{};
  a.loc2glob = it->d_l2g.get();
  a.cmask = it->d_cmask.get();
  a.tab = it->d_tab.get();
  a.sinv = it->d_sinv.get();
  a.jxw = it->d_jxw.get();
  a.jinv = it->geo.jinv.as<const double>();
  a.vol = it->d_vol.get();
  a.u = (const double *)u;
  a.weight = (const double *)weight_qp;
  a.local = it->d_ind_local.get();
  a.nodal = it->d_ind_nodal.get();
  a.per_cell = (double *)per_cell;
  a.local_stride = local_stride;
  a.n_dofs = it->n_dofs;
  a.general = it->general ? 1 : 0;
  HIP_TRY(launch_indicator(it->dim, it->n, true, a, it->n_cells, st));
  hipLaunchKernelGGL(indicator_gather_kernel, dim3((it->n_dofs + 255) / 256, it->dim), dim3(256), 0, st, a.nodal,
                     (const double *)a.local, (const double *)it->d_den.get(), it->d_ind_off.get(), it->d_ind_idx.get(),
                     it->n_dofs, local_stride);
  HIP_TRY(hipGetLastError());
  HIP_TRY(launch_indicator(it->dim, it->n, false, a, it->n_cells, st));
  return 0;
}
