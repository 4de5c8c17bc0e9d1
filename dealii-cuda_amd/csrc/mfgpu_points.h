// Evaluation and point sources at arbitrary points (include/mfgpu.h, "points"): what the host
// half (mfgpu_points_locate.cpp, plain C++) and the device half (mfgpu_points.hip) share.
#ifndef MFGPU_POINTS_H
#define MFGPU_POINTS_H

#include <cstdint>
#include <vector>

#include "mfgpu_internal.h"

namespace mfgpu {

// A work item is one wave's share of one cell's points: at most kPointsPerItem of them, walked in chunks of 64.
constexpr uint32_t kPointsPerItem = 512;
constexpr int kItemWords = 4;  // {cell, first sorted position, number of points, 0}

// The 1D table of the point kernels for N = degree + 1 Gauss abscissae on [0, 1]: the abscissae g_j, then
// r[j][k] = 1 / (g_j - g_k) (0 on the diagonal).  L_j(t) = prod_{k != j} (t - g_k) r[j][k] and
// L_j'(t) = sum_{m != j} r[j][m] prod_{k != j, m} (t - g_k) r[j][k]: products only, so well defined at the abscissae.
std::vector<double> point_table(int n);
// l[j] = L_j(t), dl[j] = L_j'(t) from a point_table (the formula of the kernels)
void point_basis(int n, const double *table, double t, double *l, double *dl);

// The constants of point location (include/mfgpu.h, "mfgpu_locate_points"), read by the host search and by
// locate_kernel (mfgpu_locate.hip) alike.
constexpr int kNewtonSteps = 30;
constexpr double kNewtonTol = 1e-14, kAcceptTol = 1e-10, kBoxInflation = 1e-10;
constexpr double kHintMargin = 1e-8;  // a hinted cell is taken only when every xi_d lies in [kHintMargin, 1 - kHintMargin]

// The candidate grid of point location, one for host and device: the boxes of the cells' 2^dim corners inflated by
// kBoxInflation of their diagonal, the box of all of them, and a uniform grid of nb bins per direction over it with the
// cells whose box meets a bin, in ascending order (CSR).
struct LocatorGrid {
  std::vector<double> lo, hi;  // [n_cells * dim]
  double glo[3] = {0, 0, 0}, ghi[3] = {0, 0, 0};
  uint32_t nb = 1;
  double inv_w[3] = {0, 0, 0};  // bins per unit length; 0 in a direction without extent
  std::vector<uint32_t> boff, bidx;  // [nb^dim + 1]; [boff.back()]
  // the bin of coordinate v in direction e, clamped to the grid (the formula of the kernel)
  uint32_t bin_of(double v, int e) const {
    const double t = (v - glo[e]) * inv_w[e];
    return t <= 0 ? 0u : t >= nb ? nb - 1 : (uint32_t)t;
  }
};
// xq: the description's quadrature_points [n_cells * n^dim * dim], n = degree + 1
void build_locator_grid(int dim, int n, size_t n_cells, const double *xq, LocatorGrid &grid);
// Newton on x(xi) = x in one cell (xq: its n^dim Gauss points) from the cell's centre; true when it converged to an
// accepted xi (then clamped to [0, 1]).  y: [n^dim * dim] scratch.
bool newton_in_cell(int dim, int n, const double *table, const double *xq, size_t nd, const double *x, double *y,
                    double *xi);

// Host half of mfgpu_points_create_in_cells: the points sorted by cell (stable, the points without a cell last), cut
// into work items, and the dof -> slot CSR of integrate (slot = item * N^dim + local index, ascending; constrained dofs
// and dofs no item touches stay empty).
struct PointsPlan {
  uint32_t n = 0, n_found = 0;
  std::vector<uint32_t> perm;   // [n] sorted position -> caller's index
  std::vector<double> xi;       // [n_found * dim] in sorted order
  std::vector<uint32_t> items;  // [n_items * kItemWords]
  std::vector<uint32_t> off, idx;
  uint32_t n_items() const { return (uint32_t)(items.size() / kItemWords); }
};
// loc2glob: [n_cells * nd]; constrained[dof] != 0: the dof's row stays 0.  MFGPU_EINVAL for a cell >= n_cells other
// than MFGPU_POINT_NOT_FOUND and for a xi outside [0, 1] (NaN included).
int build_points_plan(int dim, uint32_t nd, uint32_t n_cells, uint32_t n_dofs, const uint32_t *loc2glob,
                      const uint8_t *constrained, const uint32_t *cell, const double *xi, uint32_t n, PointsPlan &plan);

// What a points object or a quadrature-point operator (mfgpu_qop.hip) borrows from its integrator
// (mfgpu_integrate.hip): device pointers, valid while it lives.
struct IntegratorView {
  int dim, n;
  bool general, updatable;
  uint32_t n_cells, n_dofs;
  const uint32_t *loc2glob, *cmask;  // [n_cells * n^dim]; [n_cells] or nullptr
  const uint32_t *rhs_off;           // [n_dofs + 1] CSR offsets of mfgpu_integrator_rhs: an empty range marks a
                                     // constrained (or unreferenced) dof
  const uint32_t *rhs_idx;           // its index list: cell-major local indices, ascending per dof
  const uint8_t *con;                // [n_dofs] 1 on a constrained dof
  const double *tab, *qpts;          // Tab<n>; [n_cells * n^dim * dim]
  const double *jxw;                 // [n_cells * n^dim]
  const double *jinv;                // updatable only: [n_cells] J0^-1, or with `general` J^-1 per point, row-major
  double *local;                     // [n_cells * n^dim] the per-cell local vectors of mfgpu_integrator_rhs (scratch)
};
IntegratorView integrator_view(const mfgpu_integrator *it);

}  // namespace mfgpu
#endif
