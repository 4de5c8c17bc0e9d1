// The locator (include/mfgpu.h, "mfgpu_locator"): mfgpu_locate_points on the device, for points
// that move.  Double only.  The definition is the host's word for word -- candidate boxes through the bin grid in
// ascending order, Newton on F(xi) = sum_q L_q(xi) (x_q - x) from the cell's centre, the tolerances of mfgpu_points.h,
// the lowest accepting cell -- and the grid is the host's own (build_locator_grid, mfgpu_points_locate.cpp).
//
// Structure: lane = point, one wave64 per workgroup.  A lane computes its bin and walks the bin's cells; the box test
// (2 dim loads) comes first, Newton runs only inside a box.  Every lane works on a cell of its own, so the operand rows
// of the contraction come from global memory, qpts[(c ND + q) dim + d] - x_d, N dim contiguous doubles per row; nothing
// of a cell is staged in LDS.  The contraction has the shape of `contract` in mfgpu_points.hip: the x direction
// unrolled with its L and L' in registers, y and z rolled loops whose L and L' sit in the lane's own column of an LDS
// array; all dim components of F and J are formed in one pass over the rows.  The basis is the product form of
// point_basis, not the kernels' lane_basis: that one uses fused multiply-adds, and this kernel keeps the host's
// arithmetic (see FP_CONTRACT below).  The candidate loop and the Newton loop are lane-dependent: a lane that has its
// cell, or whose iteration has converged, idles until the slowest lane of its wave is done.  That divergence is
// accepted; what it costs is what points sorted by cell and hints win back (tools/bench_locate.py).
// The integrator's Gauss points are borrowed, not copied (they are the largest array of the set-up).
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "mfgpu_device.h"
#include "mfgpu_integrate_cell.h"
#include "mfgpu_points.h"

using namespace mfgpu;

// no fused multiply-adds in this file: the kernel keeps the host's arithmetic (see lane_basis below)
#pragma STDC FP_CONTRACT OFF

namespace {

struct LocArgs {
  const double *qpts;  // [n_cells * N^dim * dim], the integrator's
  const double *ptab;  // point_table(N)
  const double *lo, *hi;        // [n_cells * dim] inflated corner boxes
  const uint32_t *boff, *bidx;  // bin -> cells CSR, cells ascending
  double glo[3], ghi[3], inv_w[3];
  uint32_t nb, n_cells;
  const double *x;       // [n * dim]
  const uint32_t *hint;  // [n] or nullptr; may be `cell`
  uint32_t n;
  uint32_t *cell;     // [n]
  double *xi;         // [n * dim]
  uint32_t *missing;  // one counter or nullptr, zeroed on the stream before the launch
};

// The device code below restates the host's point_basis, map_eval, newton_step and newton_in_cell
// (mfgpu_points_locate.cpp) operation by operation, in the host's order and without fused multiply-adds: every
// operation is a correctly rounded IEEE one on both sides, so a lane takes the host's decisions (which candidate
// converges, which is accepted) and not merely close ones.

// l[j] = L_j(t), dl[j] = L_j'(t): point_basis of the host, from the table in LDS
template <int N>
__device__ __forceinline__ void lane_basis(const double *__restrict__ pt, double t, double (&l)[N], double (&dl)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double v = 1, d = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      if (k == j) continue;
      const double r = pt[N + j * N + k], f = (t - pt[k]) * r;
      d = d * f + v * r;
      v *= f;
    }
    l[j] = v;
    dl[j] = d;
    __builtin_amdgcn_sched_barrier(0);  // row by row: the N * N table entries are not all fetched up front
  }
}

// F_d = sum_q L_q (x_q,d - x_d) and J[d][e] = sum_q dL_q / dxi_e (x_q,d - x_d) of one cell's Gauss points xq in global
// memory: map_eval of the host.  The differences are formed before the contraction (with
// x(xi) - x formed afterwards the step at the solution is eps |x| / h).  lx, dlx: L and L' of the x direction; LL: the
// lane's LDS column, row (2 (e - 1) + derivative) N + index for e = y, z, as in contract (mfgpu_points.hip).
template <int dim, int N>
__device__ __forceinline__ void contract_map(const double *__restrict__ xq, const double (&x)[dim],
                                             const double (&lx)[N], const double (&dlx)[N],
                                             const double *__restrict__ LL, double (&F)[dim], double (&J)[dim][dim]) {
#pragma unroll
  for (int d = 0; d < dim; ++d) {
    F[d] = 0;
#pragma unroll
    for (int e = 0; e < dim; ++e) J[d][e] = 0;
  }
  constexpr int NZ = dim == 3 ? N : 1;
#pragma unroll 1
  for (int k = 0; k < NZ; ++k) {
    double wk = 1.0, dwk = 0.0;
    if constexpr (dim == 3) wk = LL[(2 * N + k) * 64], dwk = LL[(3 * N + k) * 64];
#pragma unroll 1
    for (int j = 0; j < N; ++j) {
      const double *row = xq + (size_t)((k * N + j) * N) * dim;
      const double wj = LL[j * 64], dwj = LL[(N + j) * 64];
      const double w00 = wk * wj, w01 = wk * dwj, w10 = dwk * wj;
#pragma unroll
      for (int d = 0; d < dim; ++d) {
        double a0 = 0, a1 = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          const double y = row[i * dim + d] - x[d];
          a0 += lx[i] * y;
          a1 += dlx[i] * y;
        }
        F[d] += w00 * a0;
        J[d][0] += w00 * a1;
        J[d][1] += w01 * a0;
        if constexpr (dim == 3) J[d][2] += w10 * a0;
      }
    }
  }
}

// delta = -J^-1 F (the formulas of the host's newton_step); false when J is singular or anything is not finite
template <int dim>
__device__ __forceinline__ bool newton_step(const double (&J)[dim][dim], const double (&F)[dim], double (&delta)[dim]) {
  if constexpr (dim == 2) {
    const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    if (!(fabs(det) > 0) || !isfinite(det)) return false;
    delta[0] = -(J[1][1] * F[0] - J[0][1] * F[1]) / det;
    delta[1] = -(-J[1][0] * F[0] + J[0][0] * F[1]) / det;
  } else {
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2],
                 c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    if (!(fabs(det) > 0) || !isfinite(det)) return false;
    const double c10 = J[0][2] * J[2][1] - J[0][1] * J[2][2], c11 = J[0][0] * J[2][2] - J[0][2] * J[2][0],
                 c12 = J[0][1] * J[2][0] - J[0][0] * J[2][1];
    const double c20 = J[0][1] * J[1][2] - J[0][2] * J[1][1], c21 = J[0][2] * J[1][0] - J[0][0] * J[1][2],
                 c22 = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    delta[0] = -(c00 * F[0] + c10 * F[1] + c20 * F[2]) / det;
    delta[1] = -(c01 * F[0] + c11 * F[1] + c21 * F[2]) / det;
    delta[2] = -(c02 * F[0] + c12 * F[1] + c22 * F[2]) / det;
  }
  bool ok = true;
#pragma unroll
  for (int d = 0; d < dim; ++d) ok = ok && isfinite(delta[d]);
  return ok;
}

__global__ void __launch_bounds__(64) zero_counter_kernel(uint32_t *counter) {
  if (threadIdx.x == 0) *counter = 0;
}

template <int dim, int N>
__global__ void __launch_bounds__(64) locate_kernel(LocArgs a) {
  constexpr int ND = cpow(N, dim);
  __shared__ double PT[N + N * N], LLS[(dim - 1) * 2 * N * 64];
  for (int i = threadIdx.x; i < N + N * N; i += 64) PT[i] = a.ptab[i];
  __syncthreads();
  const size_t k = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool active = k < a.n;  // a tail lane holds a NaN point and no hint: it finds nothing and stores nothing
  double x[dim];
#pragma unroll
  for (int d = 0; d < dim; ++d) x[d] = active ? a.x[k * dim + d] : __builtin_nan("");
  const uint32_t hint = active && a.hint ? a.hint[k] : MFGPU_POINT_NOT_FOUND;  // read before cell[k] is written
  bool hinting = hint < a.n_cells;
  // the candidates of the ordinary search: the cells of the point's bin, none for a point outside the global box (NaN)
  uint32_t j = 0, jend = 0;
  bool inside = true;
#pragma unroll
  for (int d = 0; d < dim; ++d) inside = inside && x[d] >= a.glo[d] && x[d] <= a.ghi[d];
  if (inside) {
    size_t b = 0;
#pragma unroll
    for (int d = dim - 1; d >= 0; --d) {
      const double t = (x[d] - a.glo[d]) * a.inv_w[d];
      b = b * a.nb + (t <= 0 ? 0u : t >= a.nb ? a.nb - 1 : (uint32_t)t);
    }
    j = a.boff[b];
    jend = a.boff[b + 1];
  }
  uint32_t found = MFGPU_POINT_NOT_FOUND;
  double r[dim];
#pragma unroll
  for (int d = 0; d < dim; ++d) r[d] = 0.0;
  double *LL = LLS + threadIdx.x;  // the lane's column
#pragma unroll 1
  for (;;) {
    // the lane's next candidate: the hinted cell once, then the bin's cells whose box holds the point, ascending
    uint32_t c = MFGPU_POINT_NOT_FOUND;
    if (hinting) c = hint;
    else
      while (j < jend) {
        const uint32_t cc = a.bidx[j++];
        bool in_box = true;
#pragma unroll
        for (int d = 0; d < dim; ++d)
          in_box = in_box && x[d] >= a.lo[(size_t)cc * dim + d] && x[d] <= a.hi[(size_t)cc * dim + d];
        if (in_box) {
          c = cc;
          break;
        }
      }
    if (c == MFGPU_POINT_NOT_FOUND) break;
    // Newton from the cell's centre
    const double *xq = a.qpts + (size_t)c * ND * dim;
    double t[dim];
#pragma unroll
    for (int d = 0; d < dim; ++d) t[d] = 0.5;
    bool ok = true, converged = false;
#pragma unroll 1
    for (int it = 0; it < kNewtonSteps && ok && !converged; ++it) {
      double lx[N], dlx[N], F[dim], J[dim][dim], delta[dim];
#pragma unroll
      for (int e = dim - 1; e >= 0; --e) {  // x last: it stays in registers
        lane_basis<N>(PT, t[e], lx, dlx);
        if (e > 0) {
#pragma unroll
          for (int i = 0; i < N; ++i) {
            LL[((2 * (e - 1)) * N + i) * 64] = lx[i];
            LL[((2 * (e - 1) + 1) * N + i) * 64] = dlx[i];
          }
        }
      }
      contract_map<dim, N>(xq, x, lx, dlx, LL, F, J);
      ok = newton_step<dim>(J, F, delta);
      double step = 0;
      if (ok) {
#pragma unroll
        for (int d = 0; d < dim; ++d) {
          t[d] += delta[d];
          step = fmax(step, fabs(delta[d]));
          ok = ok && fabs(t[d] - 0.5) < 1e3;  // else diverging
        }
      }
      converged = ok && step <= kNewtonTol;
    }
    // a hinted cell is taken only well inside (then no other cell accepts the point: a condition of the interface);
    // a candidate of the search within the acceptance tolerance, clamped
    const double margin = hinting ? kHintMargin : -kAcceptTol;
    bool take = converged;
#pragma unroll
    for (int d = 0; d < dim; ++d) take = take && t[d] >= margin && t[d] <= 1 - margin;
    hinting = false;
    if (take) {
      found = c;
#pragma unroll
      for (int d = 0; d < dim; ++d) r[d] = fmin(1.0, fmax(0.0, t[d]));
      break;
    }
  }
  if (active) {
    a.cell[k] = found;
#pragma unroll
    for (int d = 0; d < dim; ++d) a.xi[k * dim + d] = r[d];
  }
  // the count: whole numbers, one ordinary atomic add per wave that has any, so the sum does not depend on the order
  const unsigned long long lost = __ballot(active && found == MFGPU_POINT_NOT_FOUND);
  if (a.missing && threadIdx.x == 0 && lost) atomicAdd(a.missing, (uint32_t)__popcll(lost));
}

template <int dim>
hipError_t launch_d(int n, const LocArgs &a, uint32_t grid, hipStream_t st) {
#define CASE(N)                                                                          \
  case N:                                                                                \
    hipLaunchKernelGGL((locate_kernel<dim, N>), dim3(grid), dim3(64), 0, st, a); \
    break;
  switch (n) {
    CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7)
    default: return hipErrorInvalidValue;
  }
#undef CASE
  return hipGetLastError();
}

}  // namespace

struct mfgpu_locator {
  IntegratorView iv{};  // qpts is read; the integrator must outlive the locator
  double glo[3] = {0, 0, 0}, ghi[3] = {0, 0, 0}, inv_w[3] = {0, 0, 0};
  uint32_t nb = 1;
  DeviceArray<double> d_ptab, d_lo, d_hi;
  DeviceArray<uint32_t> d_boff, d_bidx;
};

void mfgpu_locator_destroy(mfgpu_locator *l) { delete l; }

int mfgpu_locator_create(mfgpu_integrator *it, const mfgpu_desc *desc, mfgpu_locator **out) {
  if (!it || !desc || !out) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  *out = nullptr;
  const mfgpu_desc &d = *desc;
  if (d.number_type == MFGPU_F32) {
    set_error("mfgpu_locator_create: MFGPU_F64 only");
    return MFGPU_EUNSUPPORTED;
  }
  if (d.number_type != MFGPU_F64) return einval("number_type must be MFGPU_F64");
  std::unique_ptr<mfgpu_locator> l(new mfgpu_locator());
  l->iv = integrator_view(it);
  const IntegratorView &iv = l->iv;
  if (d.dim != iv.dim || d.degree + 1 != iv.n || d.n_cells != iv.n_cells)
    return einval("mfgpu_locator_create: the description is not the one the integrator was created from");
  if (!d.quadrature_points || d.n_cells == 0)
    return einval("mfgpu_locator_create: quadrature_points and cells are required");
  LocatorGrid g;
  build_locator_grid(iv.dim, iv.n, d.n_cells, (const double *)d.quadrature_points, g);
  for (int e = 0; e < 3; ++e) l->glo[e] = g.glo[e], l->ghi[e] = g.ghi[e], l->inv_w[e] = g.inv_w[e];
  l->nb = g.nb;
  const std::vector<double> ptab = point_table(iv.n);
  int rc;
  if ((rc = l->d_ptab.upload(ptab.data(), ptab.size()))) return rc;
  if ((rc = l->d_lo.upload(g.lo.data(), g.lo.size()))) return rc;
  if ((rc = l->d_hi.upload(g.hi.data(), g.hi.size()))) return rc;
  if ((rc = l->d_boff.upload(g.boff.data(), g.boff.size()))) return rc;
  if ((rc = l->d_bidx.upload(g.bidx.data(), g.bidx.size()))) return rc;
  *out = l.release();
  return 0;
}

size_t mfgpu_locator_memory_consumption(const mfgpu_locator *l) {
  if (!l) return 0;
  return l->d_ptab.bytes() + l->d_lo.bytes() + l->d_hi.bytes() + l->d_boff.bytes() + l->d_bidx.bytes();
}

int mfgpu_locator_locate(mfgpu_locator *l, const double *x, uint32_t n, const uint32_t *hint, uint32_t *cell, double *xi,
                         uint32_t *n_not_found, void *stream) {
  if (!l || (n && (!x || !cell || !xi))) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  if (n_not_found) {  // a kernel, not hipMemsetAsync: a captured memset node does not replay reliably (mfgpu_level.hip)
    hipLaunchKernelGGL(zero_counter_kernel, dim3(1), dim3(64), 0, st, n_not_found);
    HIP_TRY(hipGetLastError());
  }
  if (n == 0) return 0;
  LocArgs a{};
  a.qpts = l->iv.qpts;
  a.ptab = l->d_ptab.get();
  a.lo = l->d_lo.get();
  a.hi = l->d_hi.get();
  a.boff = l->d_boff.get();
  a.bidx = l->d_bidx.get();
  for (int e = 0; e < 3; ++e) a.glo[e] = l->glo[e], a.ghi[e] = l->ghi[e], a.inv_w[e] = l->inv_w[e];
  a.nb = l->nb;
  a.n_cells = l->iv.n_cells;
  a.x = x;
  a.hint = hint;
  a.n = n;
  a.cell = cell;
  a.xi = xi;
  a.missing = n_not_found;
  const uint32_t grid = (uint32_t)(((uint64_t)n + 63) / 64);
  HIP_TRY(l->iv.dim == 2 ? launch_d<2>(l->iv.n, a, grid, st) : launch_d<3>(l->iv.n, a, grid, st));
  return 0;
}

int mfgpu_points_create_located(mfgpu_integrator *it, const uint32_t *cell_dev, const double *xi_dev, uint32_t n,
                                void *stream, mfgpu_points **out) {
  if (!it || !out || (n && (!cell_dev || !xi_dev))) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  *out = nullptr;
  const int dim = integrator_view(it).dim;
  std::vector<uint32_t> cell(n);
  std::vector<double> xi((size_t)n * dim);
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // the one synchronising step between locating and evaluating
  if (n) {
    HIP_TRY(hipMemcpy(cell.data(), cell_dev, cell.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(xi.data(), xi_dev, xi.size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  return mfgpu_points_create_in_cells(it, cell.data(), xi.data(), n, out);
}
