// The vector-valued quadrature-point operator (include/mfgpu.h, "mfgpu_vqop"): linear elasticity.
// Double only, as the integrator.  A field has dim components in blocks, u[a * n_dofs + i].
//
//   (A u)_(a,i) = sum_cells sum_q JxW_q [sum_k d_k phi_i sigma_ak + phi_i rho u_a],
//   sigma = lambda (div u) I + mu (grad u + grad u^T)   or   sigma_ak = sum_bl C[a][k][b][l] d_l u_b
//
// Structure, as mfgpu_qop.hip: one wave64 workgroup per cell, sum factorisation in LDS (tensor<>), hn_resolve on LDS
// pencils per component, dim per-cell local vectors (component 0 in the integrator's scratch, the others in the
// operator's), then one per-entry gather over the integrator's CSR for all components.  No atomics: bitwise repeatable.
// Everything only enqueues.  Folded arrays are component-major inside a cell ([cell][component][q]).
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "mfgpu_device.h"
#include "mfgpu_integrate_cell.h"
#include "mfgpu_points.h"

using namespace mfgpu;

namespace {

enum Law { LAW_NONE, LAW_ISO_UNIFORM, LAW_ISO_GENERAL, LAW_TENSOR4 };

struct VqopArgs {
  const uint32_t *loc2glob;  // [n_cells * N^dim]
  const uint32_t *cmask;     // [n_cells] or nullptr
  const uint8_t *con;        // [dim * n_dofs] the operator's own flags
  const double *tab;         // Tab<N>
  double *local0, *localx;   // [n_cells * N^dim] component 0; [(dim - 1) * n_cells * N^dim] the others
  const double *src;         // [dim * n_dofs]
  const double *lam, *mu;    // [cell][q] folded
  const double *c4;          // [cell][((a * dim + e) * dim + b) * dim + f][q] folded
  const double *mass;        // [cell][q] folded; nullptr without the term
  const double *jinv;        // LAW_ISO_GENERAL: the integrator's J^-1 per point, row-major
  uint32_t n_dofs, n_cells;
  int law;
};

__device__ __forceinline__ double *local_of(const VqopArgs &a, int comp, size_t cell_stride) {
  return comp == 0 ? a.local0 : a.localx + (size_t)(comp - 1) * cell_stride;
}

// LOC = integral of V (if has_v) against phi_i plus the reference fluxes G[e] (if has_g) against d phi_i / d xi_e: the
// integrate_local of mfgpu_qop.hip.  Thread t owns LOC[t], LOC[t + 64], ...; tensor<> begins and ends with a barrier.
template <int dim, int N>
__device__ __forceinline__ void integrate_component(const double *tab, bool has_v, bool has_g, const double *V,
                                                    const double *G, double *LOC, double *TO, double *T1, double *T2) {
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

// The cell operator on the nodal values A[dim][ND] (hanging-node resolved); the result overwrites A.  only >= 0: the
// input is nonzero in component `only` alone and only that component of the result is formed (the diagonal).
// G[(b * dim + f) * ND + q] = d u_b / d xi_f on entry to the law, the reference flux of component b, direction f after.
template <int dim, int N, bool MASS>
__device__ __forceinline__ void vqop_cell_apply(const VqopArgs &a, size_t c0, const double *tab, int only, double *A,
                                                double *U, double *G, double *TO, double *T1, double *T2) {
  constexpr int ND = cpow(N, dim);
  using TB = Tab<N>;
  const double *S = tab + TB::SE, *D = tab + TB::GE;
  const bool stress = a.law != LAW_NONE;
#pragma unroll
  for (int b = 0; b < dim; ++b) {
    if (only >= 0 && b != only) continue;
    if constexpr (MASS) tensor<dim, N, N>(A + b * ND, U + b * ND, S, S, S, T1, T2);
    if (stress) {
#pragma unroll
      for (int f = 0; f < dim; ++f)
        tensor<dim, N, N>(A + b * ND, G + (b * dim + f) * ND, f == 0 ? D : S, f == 1 ? D : S, f == 2 ? D : S, T1, T2);
    }
  }
  for (int q = threadIdx.x; q < ND; q += 64) {  // the thread owns point q in every array: in place
    if constexpr (MASS) {
      const double m = a.mass[c0 + q];
#pragma unroll
      for (int b = 0; b < dim; ++b)
        if (only < 0 || b == only) U[b * ND + q] *= m;
    }
    if (!stress) continue;
    double h[dim][dim], fl[dim][dim];
#pragma unroll
    for (int b = 0; b < dim; ++b)
#pragma unroll
      for (int f = 0; f < dim; ++f) h[b][f] = (only < 0 || b == only) ? G[(b * dim + f) * ND + q] : 0.0;
    if (a.law == LAW_TENSOR4) {
      const double *T = a.c4 + c0 * (dim * dim * dim * dim) + q;
#pragma unroll
      for (int c = 0; c < dim; ++c)
#pragma unroll
        for (int e = 0; e < dim; ++e) {
          double s = 0;
          if (only < 0 || c == only) {
#pragma unroll
            for (int b = 0; b < dim; ++b)
#pragma unroll
              for (int f = 0; f < dim; ++f) s = fma(T[(size_t)(((c * dim + e) * dim + b) * dim + f) * ND], h[b][f], s);
          }
          fl[c][e] = s;
        }
    } else if (a.law == LAW_ISO_UNIFORM) {  // lam, mu carry J0^2 JxW: the law in reference gradients
      const double l = a.lam[c0 + q], m = a.mu[c0 + q];
      double tr = 0;
#pragma unroll
      for (int b = 0; b < dim; ++b) tr += h[b][b];
#pragma unroll
      for (int c = 0; c < dim; ++c)
#pragma unroll
        for (int e = 0; e < dim; ++e) fl[c][e] = fma(m, h[c][e] + h[e][c], c == e ? l * tr : 0.0);
    } else {  // LAW_ISO_GENERAL: grad_x u_b = J^-T grad_xi u_b, sigma, reference flux J^-1 sigma_c
      const double l = a.lam[c0 + q], m = a.mu[c0 + q];
      const double *Jp = a.jinv + (c0 + q) * (dim * dim);  // J^-1[e][k] = d xi_e / d x_k
      double J[dim][dim], g[dim][dim];
#pragma unroll
      for (int e = 0; e < dim; ++e)
#pragma unroll
        for (int k = 0; k < dim; ++k) J[e][k] = Jp[e * dim + k];
      double tr = 0;
#pragma unroll
      for (int b = 0; b < dim; ++b) {
#pragma unroll
        for (int k = 0; k < dim; ++k) {
          double s = 0;
#pragma unroll
          for (int f = 0; f < dim; ++f) s = fma(J[f][k], h[b][f], s);
          g[b][k] = s;
        }
        tr += g[b][b];
      }
#pragma unroll
      for (int c = 0; c < dim; ++c) {
        double sg[dim];
#pragma unroll
        for (int k = 0; k < dim; ++k) sg[k] = fma(m, g[c][k] + g[k][c], c == k ? l * tr : 0.0);
#pragma unroll
        for (int e = 0; e < dim; ++e) {
          double s = 0;
#pragma unroll
          for (int k = 0; k < dim; ++k) s = fma(J[e][k], sg[k], s);
          fl[c][e] = s;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < dim; ++c)
#pragma unroll
      for (int e = 0; e < dim; ++e)
        if (only < 0 || c == only) G[(c * dim + e) * ND + q] = fl[c][e];
  }
#pragma unroll
  for (int c = 0; c < dim; ++c) {
    if (only >= 0 && c != only) continue;
    integrate_component<dim, N>(tab, MASS, stress, U + c * ND, G + c * dim * ND, A + c * ND, TO, T1, T2);
  }
}

template <int dim, int N, bool MASS>
__global__ void __launch_bounds__(64) vqop_cell_kernel(VqopArgs a) {
  constexpr int ND = cpow(N, dim);
  using TB = Tab<N>;
  __shared__ double tab[TB::size], A[dim * ND], U[MASS ? dim * ND : 1], G[dim * dim * ND], TO[ND], T1[ND], T2[ND];
  const uint32_t c = blockIdx.x;
  const size_t c0 = (size_t)c * ND, cell_stride = (size_t)a.n_cells * ND;
  load_tab<N>(tab, a.tab);
  const unsigned mask = a.cmask ? a.cmask[c] : 0u;
  for (int i = threadIdx.x; i < ND; i += 64) {  // constrained entries of src are read as 0
    const uint32_t gi = a.loc2glob[c0 + i];
#pragma unroll
    for (int b = 0; b < dim; ++b) {
      const size_t j = (size_t)b * a.n_dofs + gi;
      const double s = a.src[j];
      A[b * ND + i] = a.con[j] ? 0.0 : s;
    }
  }
  if (mask) {
#pragma unroll
    for (int b = 0; b < dim; ++b) hn_resolve<dim, N, false>(A + b * ND, mask, tab + TB::W);
  }
  vqop_cell_apply<dim, N, MASS>(a, c0, tab, -1, A, U, G, TO, T1, T2);
  if (mask) {
#pragma unroll
    for (int b = 0; b < dim; ++b) hn_resolve<dim, N, true>(A + b * ND, mask, tab + TB::W);
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < dim; ++b) {
    double *loc = local_of(a, b, cell_stride);
    for (int i = threadIdx.x; i < ND; i += 64) loc[c0 + i] = A[b * ND + i];
  }
}

// local_b[cell][i] = (C^T K C)_(b,i),(b,i) of the cell: the cell operator with both hanging-node resolutions on the
// local unit vector e_i of component b, entry i of component b.  Set-up work: dim N^dim (one-component) applies per cell.
template <int dim, int N, bool MASS>
__global__ void __launch_bounds__(64) vqop_diag_kernel(VqopArgs a) {
  constexpr int ND = cpow(N, dim);
  using TB = Tab<N>;
  __shared__ double tab[TB::size], A[dim * ND], U[MASS ? dim * ND : 1], G[dim * dim * ND], TO[ND], T1[ND], T2[ND];
  const uint32_t c = blockIdx.x;
  const size_t c0 = (size_t)c * ND, cell_stride = (size_t)a.n_cells * ND;
  load_tab<N>(tab, a.tab);
  const unsigned mask = a.cmask ? a.cmask[c] : 0u;
  for (int b = 0; b < dim; ++b) {
    double *Ab = A + b * ND, *loc = local_of(a, b, cell_stride);
    for (int i = 0; i < ND; ++i) {
      for (int j = threadIdx.x; j < ND; j += 64) Ab[j] = j == i ? 1.0 : 0.0;
      if (mask) hn_resolve<dim, N, false>(Ab, mask, tab + TB::W);
      vqop_cell_apply<dim, N, MASS>(a, c0, tab, b, A, U, G, TO, T1, T2);
      if (mask) hn_resolve<dim, N, true>(Ab, mask, tab + TB::W);
      __syncthreads();
      if ((int)threadIdx.x == (i & 63)) loc[c0 + i] = Ab[i];
      __syncthreads();
    }
  }
}

// dst[j], j = a * n_dofs + i: the sum of dof i's local entries of component a in ascending (cell, local index) order,
// as qop_gather_kernel; constrained rows are identity rows.  dst may be src: no __restrict__ on the two.
__global__ void __launch_bounds__(256) vqop_gather_kernel(double *dst, const double *src, const double *__restrict__ local0,
                                                          const double *__restrict__ localx, size_t cell_stride,
                                                          const uint32_t *__restrict__ off,
                                                          const uint32_t *__restrict__ idx,
                                                          const uint8_t *__restrict__ con, uint32_t n_dofs, size_t n) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint32_t a = (uint32_t)(j / n_dofs), i = (uint32_t)(j - (size_t)a * n_dofs);
  const double *local = a == 0 ? local0 : localx + (size_t)(a - 1) * cell_stride;
  double s = 0;
  for (uint32_t k = off[i]; k < off[i + 1]; ++k) s += local[idx[k]];
  dst[j] = con[j] ? src[j] : s;
}

// inv_diag[j] = 1 / (sum of the entry's local diagonals); 1 on constrained and unreferenced entries
__global__ void __launch_bounds__(256) vqop_inv_diag_kernel(double *__restrict__ inv_diag,
                                                            const double *__restrict__ local0,
                                                            const double *__restrict__ localx, size_t cell_stride,
                                                            const uint32_t *__restrict__ off,
                                                            const uint32_t *__restrict__ idx,
                                                            const uint8_t *__restrict__ con, uint32_t n_dofs, size_t n) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const uint32_t a = (uint32_t)(j / n_dofs), i = (uint32_t)(j - (size_t)a * n_dofs);
  const double *local = a == 0 ? local0 : localx + (size_t)(a - 1) * cell_stride;
  const uint32_t b = off[i], e = off[i + 1];
  double s = 0;
  for (uint32_t k = b; k < e; ++k) s += local[idx[k]];
  inv_diag[j] = (e > b && !con[j]) ? 1.0 / s : 1.0;
}

__global__ void __launch_bounds__(256) vqop_set_constrained_kernel(double *__restrict__ vec,
                                                                   const uint8_t *__restrict__ con, double value,
                                                                   size_t n) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n && con[j]) vec[j] = value;
}

// The folds of mfgpu_vqop_set_coefficients, one thread per point; nullptr = leave that term alone.
struct VFoldArgs {
  const double *jxw, *jinv;  // jinv nullptr: mass only
  const double *lam, *mu, *c4, *mass;  // the caller's real-space arrays
  double *o_lam, *o_mu, *o_c4, *o_mass;
  int general;
  uint32_t n_cells, nd;
};

template <int dim>
__global__ void __launch_bounds__(256) vqop_fold_kernel(VFoldArgs a) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)a.n_cells * a.nd) return;
  const uint32_t c = (uint32_t)(p / a.nd), q = (uint32_t)(p - (size_t)c * a.nd);
  const size_t c0 = (size_t)c * a.nd, nd = a.nd;
  const double w = a.jxw[p];
  if (a.mass) a.o_mass[p] = w * a.mass[p];
  if (a.lam) {  // with mu; uniform-J0: the law stays in reference gradients, so J0^2 goes into the coefficient
    const double s = a.general ? w : w * a.jinv[c] * a.jinv[c];
    a.o_lam[p] = s * a.lam[p];
    a.o_mu[p] = s * a.mu[p];
  }
  if (!a.c4) return;
  constexpr int d4 = dim * dim * dim * dim;
  double J[dim][dim];  // J^-1[e][k] = d xi_e / d x_k
#pragma unroll
  for (int e = 0; e < dim; ++e)
#pragma unroll
    for (int k = 0; k < dim; ++k)
      J[e][k] = a.general ? a.jinv[p * (dim * dim) + e * dim + k] : (e == k ? a.jinv[c] : 0.0);
  const double *C = a.c4 + p * d4;
  double *o = a.o_c4 + c0 * d4 + q;
#pragma unroll
  for (int ca = 0; ca < dim; ++ca)
#pragma unroll
    for (int cb = 0; cb < dim; ++cb) {
#pragma unroll
      for (int e = 0; e < dim; ++e) {
        double t[dim];  // (J^-1 C[ca][.][cb][.])[e][l]
#pragma unroll
        for (int l = 0; l < dim; ++l) {
          double s = 0;
#pragma unroll
          for (int k = 0; k < dim; ++k) s = fma(J[e][k], C[((ca * dim + k) * dim + cb) * dim + l], s);
          t[l] = s;
        }
#pragma unroll
        for (int f = 0; f < dim; ++f) {
          double s = 0;
#pragma unroll
          for (int l = 0; l < dim; ++l) s = fma(t[l], J[f][l], s);
          o[(size_t)(((ca * dim + e) * dim + cb) * dim + f) * nd] = w * s;
        }
      }
    }
}

enum Which { APPLY, DIAG };

template <int dim, int N>
hipError_t launch_dn(Which w, bool mass, const VqopArgs &a, hipStream_t st) {
  const dim3 grid(a.n_cells), block(64);
  if (w == APPLY) {
    if (mass) hipLaunchKernelGGL((vqop_cell_kernel<dim, N, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((vqop_cell_kernel<dim, N, false>), grid, block, 0, st, a);
  } else {
    if (mass) hipLaunchKernelGGL((vqop_diag_kernel<dim, N, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((vqop_diag_kernel<dim, N, false>), grid, block, 0, st, a);
  }
  return hipGetLastError();
}

hipError_t launch(int dim, int n, Which w, bool mass, const VqopArgs &a, hipStream_t st) {
#define CASE(N)                                                                      \
  case N:                                                                            \
    return dim == 2 ? launch_dn<2, N>(w, mass, a, st) : launch_dn<3, N>(w, mass, a, st);
  switch (n) {
    CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7)
    default: return hipErrorInvalidValue;
  }
#undef CASE
}

constexpr uint32_t kAllTerms = MFGPU_VQOP_ISOTROPIC | MFGPU_VQOP_TENSOR4 | MFGPU_VQOP_MASS;
constexpr uint32_t kStress = MFGPU_VQOP_ISOTROPIC | MFGPU_VQOP_TENSOR4;

}  // namespace

struct mfgpu_vqop {
  IntegratorView iv{};
  uint32_t terms = 0, set = 0;  // MFGPU_VQOP_* bits: requested, and given to set_coefficients at least once
  size_t n = 0;                 // dim * n_dofs
  DeviceArray<double> d_lam, d_mu, d_c4, d_mass;
  DeviceArray<uint8_t> d_con;   // [dim * n_dofs] 1 on a constrained entry
  DeviceArray<double> d_local;  // [(dim - 1) * n_cells * N^dim] local vectors of components 1..dim-1 (scratch)
};

int mfgpu_vqop_create(mfgpu_integrator *it, uint32_t terms, const uint32_t *constrained, size_t n_constrained,
                      mfgpu_vqop **out) {
  if (!it || !out) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  *out = nullptr;
  if (terms == 0 || (terms & ~kAllTerms)) return einval("mfgpu_vqop_create: terms must be a non-empty set of MFGPU_VQOP_* bits");
  if ((terms & kStress) == kStress)
    return einval("mfgpu_vqop_create: MFGPU_VQOP_ISOTROPIC and MFGPU_VQOP_TENSOR4 exclude each other");
  const IntegratorView iv = integrator_view(it);
  if ((terms & kStress) && !iv.updatable)
    return einval("mfgpu_vqop_create: the stress terms need inv_jac on the device; create the integrator with "
                  "MFGPU_UPDATABLE_COEFFICIENTS");
  if (!constrained && n_constrained) return einval("mfgpu_vqop_create: constrained is NULL but n_constrained is not 0");
  const size_t dim = (size_t)iv.dim, n = dim * iv.n_dofs;
  if (n > 0xffffffffull) return einval("mfgpu_vqop_create: dim * n_dofs does not fit the 32-bit block numbering");
  // the operator's own flags: the description's list in every component, or the caller's, which must cover it
  std::vector<uint8_t> base(iv.n_dofs), con(n, 0);
  if (iv.n_dofs) HIP_TRY(hipMemcpy(base.data(), iv.con, iv.n_dofs, hipMemcpyDeviceToHost));
  if (!constrained) {
    for (size_t a = 0; a < dim; ++a) std::copy(base.begin(), base.end(), con.begin() + a * iv.n_dofs);
  } else {
    for (size_t k = 0; k < n_constrained; ++k) {
      if (constrained[k] >= n) return einval("mfgpu_vqop_create: constrained index out of range [0, dim * n_dofs)");
      if (k && constrained[k] <= constrained[k - 1]) return einval("mfgpu_vqop_create: constrained is not strictly ascending");
      con[constrained[k]] = 1;
    }
    for (size_t a = 0; a < dim; ++a)
      for (size_t i = 0; i < iv.n_dofs; ++i)
        if (base[i] && !con[a * iv.n_dofs + i])
          return einval("mfgpu_vqop_create: constrained must hold every dof of the description's constrained_dofs (the "
                        "hanging dofs among them) in every component");
  }
  std::unique_ptr<mfgpu_vqop> q(new mfgpu_vqop());
  q->iv = iv;
  q->terms = terms;
  q->n = n;
  const size_t np = (size_t)iv.n_cells * (size_t)ipow(iv.n, iv.dim);
  int rc;
  if ((terms & MFGPU_VQOP_ISOTROPIC) && ((rc = q->d_lam.alloc(np)) || (rc = q->d_mu.alloc(np)))) return rc;
  if ((terms & MFGPU_VQOP_TENSOR4) && (rc = q->d_c4.alloc(np * dim * dim * dim * dim))) return rc;
  if ((terms & MFGPU_VQOP_MASS) && (rc = q->d_mass.alloc(np))) return rc;
  if ((rc = q->d_con.upload(con.data(), n))) return rc;
  if ((rc = q->d_local.alloc((dim - 1) * np))) return rc;
  *out = q.release();
  return 0;
}

int mfgpu_vqop_set_coefficients(mfgpu_vqop *q, const mfgpu_vqop_coefficients *c, void *stream) {
  if (!q || !c) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  if (!c->lambda != !c->mu) return einval("mfgpu_vqop_set_coefficients: lambda and mu are set together");
  uint32_t given = 0;
  if (c->lambda) given |= MFGPU_VQOP_ISOTROPIC;
  if (c->tensor) given |= MFGPU_VQOP_TENSOR4;
  if (c->mass) given |= MFGPU_VQOP_MASS;
  if (given & ~q->terms) return einval("mfgpu_vqop_set_coefficients: a coefficient was given for a term the operator was created without");
  if (!given) return einval("mfgpu_vqop_set_coefficients: every coefficient is NULL");
  const IntegratorView &iv = q->iv;
  VFoldArgs a{};
  a.jxw = iv.jxw;
  a.jinv = iv.jinv;
  a.lam = (const double *)c->lambda;
  a.mu = (const double *)c->mu;
  a.c4 = (const double *)c->tensor;
  a.mass = (const double *)c->mass;
  a.o_lam = q->d_lam.get();
  a.o_mu = q->d_mu.get();
  a.o_c4 = q->d_c4.get();
  a.o_mass = q->d_mass.get();
  a.general = iv.general ? 1 : 0;
  a.n_cells = iv.n_cells;
  a.nd = (uint32_t)ipow(iv.n, iv.dim);
  const size_t np = (size_t)a.n_cells * a.nd;
  const dim3 grid((unsigned)((np + 255) / 256)), block(256);
  if (iv.dim == 2) hipLaunchKernelGGL(vqop_fold_kernel<2>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(vqop_fold_kernel<3>, grid, block, 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  q->set |= given;
  return 0;
}

static int vqop_args(const mfgpu_vqop *q, const char *who, VqopArgs &a) {
  if (q->set != q->terms) {
    set_error(std::string(who) + ": mfgpu_vqop_set_coefficients has not set every term yet");
    return MFGPU_EINVAL;
  }
  const IntegratorView &iv = q->iv;
  a = VqopArgs{};
  a.loc2glob = iv.loc2glob;
  a.cmask = iv.cmask;
  a.con = q->d_con.get();
  a.tab = iv.tab;
  a.local0 = iv.local;
  a.localx = q->d_local.get();
  a.lam = q->d_lam.get();
  a.mu = q->d_mu.get();
  a.c4 = q->d_c4.get();
  a.mass = q->d_mass.get();
  a.jinv = iv.jinv;
  a.n_dofs = iv.n_dofs;
  a.n_cells = iv.n_cells;
  a.law = (q->terms & MFGPU_VQOP_TENSOR4)      ? LAW_TENSOR4
          : !(q->terms & MFGPU_VQOP_ISOTROPIC) ? LAW_NONE
          : iv.general                         ? LAW_ISO_GENERAL
                                               : LAW_ISO_UNIFORM;
  return 0;
}

int mfgpu_vqop_vmult(mfgpu_vqop *q, void *dst, const void *src, void *stream) {
  if (!q || !dst || !src) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  VqopArgs a;
  if (const int rc = vqop_args(q, "mfgpu_vqop_vmult", a)) return rc;
  a.src = (const double *)src;
  const IntegratorView &iv = q->iv;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(launch(iv.dim, iv.n, APPLY, (q->terms & MFGPU_VQOP_MASS) != 0, a, st));
  const size_t cell_stride = (size_t)iv.n_cells * (size_t)ipow(iv.n, iv.dim);
  hipLaunchKernelGGL(vqop_gather_kernel, dim3((unsigned)((q->n + 255) / 256)), dim3(256), 0, st, (double *)dst,
                     (const double *)src, (const double *)iv.local, (const double *)q->d_local.get(), cell_stride,
                     iv.rhs_off, iv.rhs_idx, (const uint8_t *)q->d_con.get(), iv.n_dofs, q->n);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mfgpu_vqop_compute_inverse_diagonal(mfgpu_vqop *q, void *inv_diag, void *stream) {
  if (!q || !inv_diag) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  VqopArgs a;
  if (const int rc = vqop_args(q, "mfgpu_vqop_compute_inverse_diagonal", a)) return rc;
  const IntegratorView &iv = q->iv;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(launch(iv.dim, iv.n, DIAG, (q->terms & MFGPU_VQOP_MASS) != 0, a, st));
  const size_t cell_stride = (size_t)iv.n_cells * (size_t)ipow(iv.n, iv.dim);
  hipLaunchKernelGGL(vqop_inv_diag_kernel, dim3((unsigned)((q->n + 255) / 256)), dim3(256), 0, st, (double *)inv_diag,
                     (const double *)iv.local, (const double *)q->d_local.get(), cell_stride, iv.rhs_off, iv.rhs_idx,
                     (const uint8_t *)q->d_con.get(), iv.n_dofs, q->n);
  HIP_TRY(hipGetLastError());
  return 0;
}

int mfgpu_vqop_set_constrained_values(mfgpu_vqop *q, void *vec, double value, void *stream) {
  if (!q || !vec) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  hipLaunchKernelGGL(vqop_set_constrained_kernel, dim3((unsigned)((q->n + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, (double *)vec, (const uint8_t *)q->d_con.get(), value, q->n);
  HIP_TRY(hipGetLastError());
  return 0;
}

size_t mfgpu_vqop_memory_consumption(const mfgpu_vqop *q) {
  return q ? q->d_lam.bytes() + q->d_mu.bytes() + q->d_c4.bytes() + q->d_mass.bytes() + q->d_con.bytes() : 0;
}

void mfgpu_vqop_destroy(mfgpu_vqop *q) { delete q; }

namespace mfgpu {
size_t vqop_length(const mfgpu_vqop *q) { return q->n; }
}  // namespace mfgpu
