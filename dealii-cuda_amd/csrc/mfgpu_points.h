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

// What a points object borrows from its integrator (mfgpu_integrate.hip): device pointers, valid while it lives.
struct IntegratorView {
  int dim, n;
  bool general;
  uint32_t n_cells, n_dofs;
  const uint32_t *loc2glob, *cmask;  // [n_cells * n^dim]; [n_cells] or nullptr
  const uint32_t *rhs_off;           // [n_dofs + 1] CSR offsets of mfgpu_integrator_rhs: an empty range marks a
                                     // constrained (or unreferenced) dof
  const double *tab, *qpts;          // Tab<n>; [n_cells * n^dim * dim]
};
IntegratorView integrator_view(const mfgpu_integrator *it);

}  // namespace mfgpu
#endif
