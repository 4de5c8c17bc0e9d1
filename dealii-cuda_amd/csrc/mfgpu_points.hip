// The points object (include/mfgpu.h, "points"): a finite element field and its gradient at
// arbitrary points of the mesh, and the transpose of the value part (point sources).  Double only.
//
// Structure: the points are sorted by cell on the host (mfgpu_points_locate.cpp) and cut into work items of at most
// kPointsPerItem points of one cell; one wave64 workgroup per work item.
//   evaluate:  the wave stages its cell in LDS exactly as evaluate_cell_kernel does (gather through loc2glob,
//              hanging-node resolution, S x S (x S): U at the Gauss points; on general geometry the cell's Gauss points
//              X next to it).  Then lane = point, 64 at a time: the lane forms L and L' of its xi (x direction in
//              registers, y and z in its own LDS column) and contracts U (and X) direction by direction -- all lanes
//              read the same LDS address at every step, a broadcast -- forms J, inverts it and stores through the
//              permutation.  The workgroups behind the last
//              work item write the zeros of the points without a cell.
//   integrate: the roles turn round.  64 points at a time put w L(xi) into LDS, [point][direction][index]; lane = Gauss
//              point q sums its products over the chunk's points in index order; then S^T per direction, transposed
//              hanging-node resolution, the work item's local vector; a gather kernel sums per dof over the CSR built
//              at creation, in ascending (work item, local index) order.  No atomics.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "mfgpu_device.h"
#include "mfgpu_integrate_cell.h"
#include "mfgpu_points.h"

using namespace mfgpu;

namespace {

struct PtArgs {
  const uint32_t *loc2glob, *cmask;
  const double *tab;      // Tab<N>
  const double *ptab;     // point_table(N)
  const double *qpts;     // [n_cells * N^dim * dim]
  const uint32_t *items;  // [n_items * kItemWords]
  const double *xi;       // [n_found * dim], sorted order
  const uint32_t *perm;   // [n] sorted position -> caller's index
  uint32_t n_items, n_found, n;
  int general;
  // evaluate
  const double *u;
  double *values, *grads;
  // integrate
  const double *weights;
  double *local;  // [n_items * N^dim]
};

// l[j] = L_j(t) (and dl[j] = L_j'(t)) in the product form of point_basis, from the table in LDS
template <int N, bool DERIV>
__device__ __forceinline__ void lane_basis(const double *__restrict__ pt, double t, double (&l)[N], double (&dl)[N]) {
  double f[N];
#pragma unroll
  for (int k = 0; k < N; ++k) f[k] = t - pt[k];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double v = 1, d = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (k == j) continue;
      const double r = pt[N + j * N + k], fk = f[k] * r;
      if (DERIV) d = fma(d, fk, v * r);
      v *= fk;
    }
    l[j] = v;
    dl[j] = d;
    __builtin_amdgcn_sched_barrier(0);  // row by row: the N * N table entries are not all fetched up front
  }
}

// v = sum_q L_q F_q and g[e] = sum_q dL_q / dxi_e F_q of the LDS array F [N^dim] (x fastest).  The lane keeps L and L' of
// the x direction in registers; those of y (and z) sit in its column of LL, row (2 (e - 1) + derivative) N + index,
// 64 lanes per row, so the loops over y and z stay loops: N^dim values of a field are never live at once (fully
// unrolled, the scheduler fetched whole cells up front: scratch from p = 3 on in 3D).  Every lane reads the same
// address of F at every step (a broadcast), and its own bank of LL.
template <int dim, int N, bool GRAD>
__device__ __forceinline__ void contract(const double *__restrict__ F, const double (&lx)[N], const double (&dlx)[N],
                                         const double *__restrict__ LL, double &v, double (&g)[dim]) {
  v = 0;
#pragma unroll
  for (int e = 0; e < dim; ++e) g[e] = 0;
  constexpr int NZ = dim == 3 ? N : 1;
#pragma unroll 1
  for (int k = 0; k < NZ; ++k) {
    double t0 = 0, tx = 0, ty = 0;
#pragma unroll 1
    for (int j = 0; j < N; ++j) {
      const double *row = F + (k * N + j) * N;
      double s0 = 0, s1 = 0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const double f = row[i];
        s0 = fma(lx[i], f, s0);
        if (GRAD) s1 = fma(dlx[i], f, s1);
      }
      const double ly = LL[j * 64];
      t0 = fma(ly, s0, t0);
      if (GRAD) {
        tx = fma(ly, s1, tx);
        ty = fma(LL[(N + j) * 64], s0, ty);
      }
    }
    if constexpr (dim == 3) {
      const double lz = LL[(2 * N + k) * 64];
      v = fma(lz, t0, v);
      if (GRAD) {
        g[0] = fma(lz, tx, g[0]);
        g[1] = fma(lz, ty, g[1]);
        g[2] = fma(LL[(3 * N + k) * 64], t0, g[2]);
      }
    } else {
      v = t0;
      g[0] = tx;
      g[1] = ty;
    }
  }
}

// r = J^-T g for J[d][e] = d x_d / d xi_e: the solution of sum_d J[d][e] r_d = g_e
template <int dim>
__device__ __forceinline__ void apply_inverse_transpose(const double (&J)[dim][dim], const double (&g)[dim],
                                                        double (&r)[dim]) {
  if constexpr (dim == 2) {
    const double inv = 1.0 / (J[0][0] * J[1][1] - J[0][1] * J[1][0]);
    r[0] = (J[1][1] * g[0] - J[1][0] * g[1]) * inv;
    r[1] = (J[0][0] * g[1] - J[0][1] * g[0]) * inv;
  } else {
    // cofactors C[d][e] of J: J^-1 = C^T / det, J^-T = C / det
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2],
                 c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double c10 = J[0][2] * J[2][1] - J[0][1] * J[2][2], c11 = J[0][0] * J[2][2] - J[0][2] * J[2][0],
                 c12 = J[0][1] * J[2][0] - J[0][0] * J[2][1];
    const double c20 = J[0][1] * J[1][2] - J[0][2] * J[1][1], c21 = J[0][2] * J[1][0] - J[0][0] * J[1][2],
                 c22 = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    const double inv = 1.0 / (J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02);
    r[0] = (c00 * g[0] + c01 * g[1] + c02 * g[2]) * inv;
    r[1] = (c10 * g[0] + c11 * g[1] + c12 * g[2]) * inv;
    r[2] = (c20 * g[0] + c21 * g[1] + c22 * g[2]) * inv;
  }
}

// GEN: general geometry (the cell's Gauss points staged for J); uniform-J0 instantiations leave X out of LDS
template <int dim, int N, bool GEN>
__global__ void __launch_bounds__(64) points_evaluate_kernel(PtArgs a) {
  constexpr int ND = cpow(N, dim), NLL = (dim - 1) * 2 * N * 64;
  using TB = Tab<N>;
  // the staging arrays A, T1, T2 are dead once U is there: the lanes' columns LLS lie over them
  __shared__ double tab[TB::size], PT[N + N * N], U[ND], X[GEN ? dim * ND : 1], WORK[NLL > 3 * ND ? NLL : 3 * ND];
  double *A = WORK, *T1 = WORK + ND, *T2 = WORK + 2 * ND, *LLS = WORK;
  if (blockIdx.x >= a.n_items) {  // the points without a cell: zeros, one lane per point
    const size_t s = (size_t)a.n_found + (size_t)(blockIdx.x - a.n_items) * 64 + threadIdx.x;
    if (s < a.n) {
      const size_t k = a.perm[s];
      if (a.values) a.values[k] = 0.0;
      if (a.grads) {
#pragma unroll
        for (int e = 0; e < dim; ++e) a.grads[k * dim + e] = 0.0;
      }
    }
    return;
  }
  const uint32_t *item = a.items + (size_t)blockIdx.x * kItemWords;
  const uint32_t c = item[0], begin = item[1], count = item[2];
  const size_t c0 = (size_t)c * ND;
  load_tab<N>(tab, a.tab);
  for (int i = threadIdx.x; i < N + N * N; i += 64) PT[i] = a.ptab[i];
  for (int i = threadIdx.x; i < ND; i += 64) A[i] = a.u[a.loc2glob[c0 + i]];
  const bool grad = a.grads != nullptr;
  if (GEN && grad) load_qpts<dim, N>(X, a.qpts, c);
  const unsigned mask = a.cmask ? a.cmask[c] : 0u;
  if (mask) hn_resolve<dim, N, false>(A, mask, tab + TB::W);
  tensor<dim, N, N>(A, U, tab + TB::SE, tab + TB::SE, tab + TB::SE, T1, T2);
  // MFGPU_UNIFORM_J0: J = h I, h from the first and the last Gauss point of the cell's first x-line
  double hinv = 0.0;
  if (!GEN && grad) hinv = (PT[N - 1] - PT[0]) / (a.qpts[(c0 + N - 1) * dim] - a.qpts[c0 * dim]);
  for (uint32_t j = threadIdx.x; j < count; j += 64) {
    const size_t s = (size_t)begin + j, k = a.perm[s];
    double lx[N], dlx[N], v, g[dim];
    double *LL = LLS + threadIdx.x;  // the lane's column
#pragma unroll
    for (int e = dim - 1; e >= 0; --e) {  // x last: it stays in registers
      if (grad) lane_basis<N, true>(PT, a.xi[s * dim + e], lx, dlx);
      else lane_basis<N, false>(PT, a.xi[s * dim + e], lx, dlx);
      if (e > 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
          LL[((2 * (e - 1)) * N + i) * 64] = lx[i];
          LL[((2 * (e - 1) + 1) * N + i) * 64] = dlx[i];
        }
      }
    }
    if (!grad) {
      contract<dim, N, false>(U, lx, dlx, LL, v, g);
      a.values[k] = v;
      continue;
    }
    contract<dim, N, true>(U, lx, dlx, LL, v, g);
    if (a.values) a.values[k] = v;
    double r[dim];
    if constexpr (!GEN) {
#pragma unroll
      for (int e = 0; e < dim; ++e) r[e] = g[e] * hinv;
    } else {
      double J[dim][dim], x;
#pragma unroll
      for (int d = 0; d < dim; ++d) contract<dim, N, true>(X + d * ND, lx, dlx, LL, x, J[d]);
      apply_inverse_transpose<dim>(J, g, r);
    }
#pragma unroll
    for (int e = 0; e < dim; ++e) a.grads[k * dim + e] = r[e];
  }
}

template <int dim, int N>
__global__ void __launch_bounds__(64) points_integrate_kernel(PtArgs a) {
  constexpr int ND = cpow(N, dim), LN = dim * N;
  using TB = Tab<N>;
  __shared__ double tab[TB::size], PT[N + N * N], LT[64 * LN], F[ND], LOC[ND], T1[ND], T2[ND];
  const uint32_t *item = a.items + (size_t)blockIdx.x * kItemWords;
  const uint32_t c = item[0], begin = item[1], count = item[2];
  load_tab<N>(tab, a.tab);
  for (int i = threadIdx.x; i < N + N * N; i += 64) PT[i] = a.ptab[i];
  for (int q = threadIdx.x; q < ND; q += 64) F[q] = 0.0;  // lane-owned throughout the chunks
  for (uint32_t j0 = 0; j0 < count; j0 += 64) {
    __syncthreads();  // PT is there; the previous chunk's LT has been read
    if (j0 + threadIdx.x < count) {
      const size_t s = (size_t)begin + j0 + threadIdx.x;
      const double w = a.weights ? a.weights[a.perm[s]] : 1.0;
#pragma unroll
      for (int e = 0; e < dim; ++e) {
        double l[N], dl[N];
        lane_basis<N, false>(PT, a.xi[s * dim + e], l, dl);
#pragma unroll
        for (int i = 0; i < N; ++i) LT[threadIdx.x * LN + e * N + i] = e == 0 ? w * l[i] : l[i];
      }
    }
    __syncthreads();
    const int m = (int)(count - j0 < 64u ? count - j0 : 64u);
    for (int q = threadIdx.x; q < ND; q += 64) {
      const int qx = q % N, qy = (q / N) % N, qz = q / (N * N);
      double acc = F[q];
      for (int pt = 0; pt < m; ++pt) {  // index order: a fixed order
        const double *t = LT + pt * LN;
        double prod = t[qx] * t[N + qy];
        if constexpr (dim == 3) prod *= t[2 * N + qz];
        acc += prod;
      }
      F[q] = acc;
    }
  }
  const double *SI = tab + TB::SI;
  tensor<dim, N, N>(F, LOC, SI, SI, SI, T1, T2);
  const unsigned mask = a.cmask ? a.cmask[c] : 0u;
  if (mask) hn_resolve<dim, N, true>(LOC, mask, tab + TB::W);
  __syncthreads();
  for (int i = threadIdx.x; i < ND; i += 64) a.local[(size_t)blockIdx.x * ND + i] = LOC[i];
}

// rhs[dof] = sum of the dof's local entries in ascending (work item, local index) order; empty ranges give 0
__global__ void __launch_bounds__(256) points_gather_kernel(double *__restrict__ rhs, const double *__restrict__ local,
                                                            const uint32_t *__restrict__ off,
                                                            const uint32_t *__restrict__ idx, uint32_t n_dofs) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_dofs) return;
  double s = 0;
  for (uint32_t j = off[i]; j < off[i + 1]; ++j) s += local[idx[j]];
  rhs[i] = s;
}

template <int dim, int N>
hipError_t launch_dn(bool evaluate, const PtArgs &a, uint32_t grid, hipStream_t st) {
  if (evaluate && a.general) hipLaunchKernelGGL((points_evaluate_kernel<dim, N, true>), dim3(grid), dim3(64), 0, st, a);
  else if (evaluate) hipLaunchKernelGGL((points_evaluate_kernel<dim, N, false>), dim3(grid), dim3(64), 0, st, a);
  else hipLaunchKernelGGL((points_integrate_kernel<dim, N>), dim3(grid), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch(int dim, int n, bool evaluate, const PtArgs &a, uint32_t grid, hipStream_t st) {
#define CASE(N)                                                                      \
  case N:                                                                            \
    return dim == 2 ? launch_dn<2, N>(evaluate, a, grid, st) : launch_dn<3, N>(evaluate, a, grid, st);
  switch (n) {
    CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7)
    default: return hipErrorInvalidValue;
  }
#undef CASE
}

}  // namespace

struct mfgpu_points {
  IntegratorView iv{};
  uint32_t n = 0, n_found = 0, n_items = 0;
  std::vector<uint32_t> cells;  // caller's order
  DeviceArray<double> d_ptab, d_xi, d_local;
  DeviceArray<uint32_t> d_perm, d_items, d_off, d_idx;
};

void mfgpu_points_destroy(mfgpu_points *p) { delete p; }

int mfgpu_points_create_in_cells(mfgpu_integrator *it, const uint32_t *cell, const double *xi, uint32_t n,
                                 mfgpu_points **out) {
  if (!it || !out || (n && (!cell || !xi))) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  *out = nullptr;
  std::unique_ptr<mfgpu_points> p(new mfgpu_points());
  p->iv = integrator_view(it);
  const IntegratorView &iv = p->iv;
  const uint32_t nd = (uint32_t)ipow(iv.n, iv.dim);
  // the host half works on the integrator's own lists: loc2glob, and the rows mfgpu_integrator_rhs leaves empty
  std::vector<uint32_t> l2g((size_t)iv.n_cells * nd), roff((size_t)iv.n_dofs + 1);
  HIP_TRY(hipMemcpy(l2g.data(), iv.loc2glob, l2g.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(roff.data(), iv.rhs_off, roff.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  std::vector<uint8_t> constrained(iv.n_dofs);
  for (uint32_t i = 0; i < iv.n_dofs; ++i) constrained[i] = roff[i] == roff[i + 1];
  PointsPlan plan;
  int rc;
  if ((rc = build_points_plan(iv.dim, nd, iv.n_cells, iv.n_dofs, l2g.data(), constrained.data(), cell, xi, n, plan)))
    return rc;
  p->n = n;
  p->n_found = plan.n_found;
  p->n_items = plan.n_items();
  p->cells.assign(cell, cell + n);
  const std::vector<double> ptab = point_table(iv.n);
  if ((rc = p->d_ptab.upload(ptab.data(), ptab.size()))) return rc;
  if ((rc = p->d_xi.upload(plan.xi.data(), plan.xi.size()))) return rc;
  if ((rc = p->d_perm.upload(plan.perm.data(), plan.perm.size()))) return rc;
  if ((rc = p->d_items.upload(plan.items.data(), plan.items.size()))) return rc;
  if ((rc = p->d_off.upload(plan.off.data(), plan.off.size()))) return rc;
  if ((rc = p->d_idx.upload(plan.idx.data(), plan.idx.size()))) return rc;
  if ((rc = p->d_local.alloc((size_t)p->n_items * nd))) return rc;
  *out = p.release();
  return 0;
}

int mfgpu_points_create(mfgpu_integrator *it, const mfgpu_desc *desc, const double *x, uint32_t n, mfgpu_points **out) {
  if (!it || !desc || !out || (n && !x)) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  *out = nullptr;
  std::vector<uint32_t> cell(n);
  std::vector<double> xi((size_t)n * 3);
  if (const int rc = mfgpu_locate_points(desc, x, n, cell.data(), xi.data(), nullptr)) return rc;
  const IntegratorView iv = integrator_view(it);
  if (desc->dim != iv.dim || desc->degree + 1 != iv.n || desc->n_cells != iv.n_cells)
    return einval("mfgpu_points_create: the description is not the one the integrator was created from");
  return mfgpu_points_create_in_cells(it, cell.data(), xi.data(), n, out);
}

int64_t mfgpu_points_cells(const mfgpu_points *p, const uint32_t **cell) {
  if (!p || !cell) return MFGPU_EINVAL;
  *cell = p->cells.data();
  return (int64_t)p->n;
}

uint32_t mfgpu_points_n_not_found(const mfgpu_points *p) { return p ? p->n - p->n_found : 0; }

size_t mfgpu_points_memory_consumption(const mfgpu_points *p) {
  if (!p) return 0;
  return p->d_ptab.bytes() + p->d_xi.bytes() + p->d_local.bytes() + p->d_perm.bytes() + p->d_items.bytes() +
         p->d_off.bytes() + p->d_idx.bytes();
}

static PtArgs base_args(const mfgpu_points *p) {
  PtArgs a{};
  a.loc2glob = p->iv.loc2glob;
  a.cmask = p->iv.cmask;
  a.tab = p->iv.tab;
  a.ptab = p->d_ptab.get();
  a.qpts = p->iv.qpts;
  a.items = p->d_items.get();
  a.xi = p->d_xi.get();
  a.perm = p->d_perm.get();
  a.n_items = p->n_items;
  a.n_found = p->n_found;
  a.n = p->n;
  a.general = p->iv.general ? 1 : 0;
  return a;
}

int mfgpu_points_evaluate(mfgpu_points *p, const void *u, void *values, void *gradients, void *stream) {
  if (!p || !u) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  if (!values && !gradients) return einval("mfgpu_points_evaluate: values and gradients are both NULL");
  const uint32_t grid = p->n_items + (p->n - p->n_found + 63) / 64;
  if (grid == 0) return 0;
  PtArgs a = base_args(p);
  a.u = (const double *)u;
  a.values = (double *)values;
  a.grads = (double *)gradients;
  HIP_TRY(launch(p->iv.dim, p->iv.n, true, a, grid, (hipStream_t)stream));
  return 0;
}

int mfgpu_points_integrate(mfgpu_points *p, void *rhs, const void *weights, void *stream) {
  if (!p || !rhs) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  PtArgs a = base_args(p);
  a.weights = (const double *)weights;
  a.local = p->d_local.get();
  if (p->n_items) HIP_TRY(launch(p->iv.dim, p->iv.n, false, a, p->n_items, st));
  hipLaunchKernelGGL(points_gather_kernel, dim3((p->iv.n_dofs + 255) / 256), dim3(256), 0, st, (double *)rhs,
                     (const double *)p->d_local.get(), p->d_off.get(), p->d_idx.get(), p->iv.n_dofs);
  HIP_TRY(hipGetLastError());
  return 0;
}
