// Host half of the points object (include/mfgpu.h, "points"), plain C++ without HIP:
// mfgpu_locate_points (which cell holds a point, and where in it) and what mfgpu_points_create_in_cells derives on the
// host (the points sorted by cell, the work items, the dof -> slot CSR of integrate).
//
// The mapping of a cell is x(xi) = sum_q L_q(xi) x_q over its QGauss(N) points x_q (N = degree + 1, x fastest) with the
// tensor Lagrange basis L_q on the 1D Gauss abscissae: exact for affine cells and MappingQ1.  Newton works on
// F(xi) = sum_q L_q(xi) (x_q - x): the differences are of the size of the cell, so the residual's rounding error is
// relative to the cell and not to the distance from the origin, and F = x(xi) - x because the L_q sum to 1.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "mfgpu_points.h"

namespace mfgpu {

namespace {

// Gauss-Legendre abscissae on [0, 1], ascending
void gauss_abscissae_01(int n, double *x) {
  for (int i = 0; i < n; ++i) {
    double z = std::cos(M_PI * (i + 0.75) / (n + 0.5));
    for (int it = 0; it < 100; ++it) {
      double p0 = 1, p1 = z;
      for (int k = 2; k <= n; ++k) {
        const double p2 = ((2 * k - 1) * z * p1 - (k - 1) * p0) / k;
        p0 = p1;
        p1 = p2;
      }
      const double dp = n * (z * p1 - p0) / (z * z - 1);
      const double dz = p1 / dp;
      z -= dz;
      if (std::fabs(dz) < 1e-16) break;
    }
    x[n - 1 - i] = 0.5 * (z + 1);
  }
}

constexpr int kMaxN = 7;

// F(xi) = sum_q L_q(xi) y_q and its Jacobian dF_d / dxi_e (row-major), y = [nd][dim], sum-factorised
void map_eval(int dim, int n, const double *table, const double *y, const double *xi, double *F, double *J) {
  double l[3][kMaxN], dl[3][kMaxN];
  for (int d = 0; d < dim; ++d) point_basis(n, table, xi[d], l[d], dl[d]);
  for (int d = 0; d < dim; ++d) F[d] = 0;
  for (int i = 0; i < dim * dim; ++i) J[i] = 0;
  const int nz = dim == 3 ? n : 1;
  for (int k = 0; k < nz; ++k) {
    const double wk = dim == 3 ? l[2][k] : 1.0, dwk = dim == 3 ? dl[2][k] : 0.0;
    for (int j = 0; j < n; ++j) {
      const double *row = y + (size_t)(k * n + j) * n * dim;
      const double wj = l[1][j], dwj = dl[1][j];
      for (int d = 0; d < dim; ++d) {
        double a0 = 0, a1 = 0;
        for (int i = 0; i < n; ++i) {
          a0 += l[0][i] * row[i * dim + d];
          a1 += dl[0][i] * row[i * dim + d];
        }
        F[d] += wk * wj * a0;
        J[d * dim + 0] += wk * wj * a1;
        J[d * dim + 1] += wk * dwj * a0;
        if (dim == 3) J[d * dim + 2] += dwk * wj * a0;
      }
    }
  }
}

// delta = -J^-1 F; false when J is singular or anything is not finite
bool newton_step(int dim, const double *J, const double *F, double *delta) {
  if (dim == 2) {
    const double det = J[0] * J[3] - J[1] * J[2];
    if (!(std::fabs(det) > 0) || !std::isfinite(det)) return false;
    delta[0] = -(J[3] * F[0] - J[1] * F[1]) / det;
    delta[1] = -(-J[2] * F[0] + J[0] * F[1]) / det;
  } else {
    const double c00 = J[4] * J[8] - J[5] * J[7], c01 = J[5] * J[6] - J[3] * J[8], c02 = J[3] * J[7] - J[4] * J[6];
    const double det = J[0] * c00 + J[1] * c01 + J[2] * c02;
    if (!(std::fabs(det) > 0) || !std::isfinite(det)) return false;
    const double c10 = J[2] * J[7] - J[1] * J[8], c11 = J[0] * J[8] - J[2] * J[6], c12 = J[1] * J[6] - J[0] * J[7];
    const double c20 = J[1] * J[5] - J[2] * J[4], c21 = J[2] * J[3] - J[0] * J[5], c22 = J[0] * J[4] - J[1] * J[3];
    delta[0] = -(c00 * F[0] + c10 * F[1] + c20 * F[2]) / det;
    delta[1] = -(c01 * F[0] + c11 * F[1] + c21 * F[2]) / det;
    delta[2] = -(c02 * F[0] + c12 * F[1] + c22 * F[2]) / det;
  }
  for (int d = 0; d < dim; ++d)
    if (!std::isfinite(delta[d])) return false;
  return true;
}

}  // namespace

// Newton on x(xi) = x in one cell from its centre; true when it converged to an accepted xi (then clamped to [0, 1])
bool newton_in_cell(int dim, int n, const double *table, const double *xq, size_t nd, const double *x, double *y,
                    double *xi) {
  for (size_t q = 0; q < nd; ++q)
    for (int d = 0; d < dim; ++d) y[q * dim + d] = xq[q * dim + d] - x[d];
  for (int d = 0; d < dim; ++d) xi[d] = 0.5;
  bool converged = false;
  for (int it = 0; it < kNewtonSteps && !converged; ++it) {
    double F[3], J[9], delta[3], step = 0;
    map_eval(dim, n, table, y, xi, F, J);
    if (!newton_step(dim, J, F, delta)) return false;
    for (int d = 0; d < dim; ++d) {
      xi[d] += delta[d];
      step = std::max(step, std::fabs(delta[d]));
      if (!(std::fabs(xi[d] - 0.5) < 1e3)) return false;  // diverging
    }
    converged = step <= kNewtonTol;
  }
  if (!converged) return false;
  for (int d = 0; d < dim; ++d)
    if (!(xi[d] >= -kAcceptTol && xi[d] <= 1 + kAcceptTol)) return false;
  for (int d = 0; d < dim; ++d) xi[d] = std::min(1.0, std::max(0.0, xi[d]));
  return true;
}

void build_locator_grid(int dim, int N, size_t nc, const double *xq, LocatorGrid &g) {
  g = LocatorGrid();
  const size_t nd = (size_t)ipow(N, dim);
  const std::vector<double> table = point_table(N);
  // boxes of the cells' corners (the mapping at xi in {0, 1}^dim), inflated
  std::vector<double> &lo = g.lo, &hi = g.hi;
  lo.resize(nc * dim);
  hi.resize(nc * dim);
  double *glo = g.glo, *ghi = g.ghi;
  for (size_t c = 0; c < nc; ++c) {
    double *l = &lo[c * dim], *h = &hi[c * dim];
    for (int v = 0; v < (1 << dim); ++v) {
      double corner[3], F[3], J[9];
      for (int e = 0; e < dim; ++e) corner[e] = (v >> e) & 1;
      map_eval(dim, N, table.data(), xq + c * nd * dim, corner, F, J);
      for (int e = 0; e < dim; ++e) {
        l[e] = v == 0 ? F[e] : std::min(l[e], F[e]);
        h[e] = v == 0 ? F[e] : std::max(h[e], F[e]);
      }
    }
    double diag = 0;
    for (int e = 0; e < dim; ++e) diag += (h[e] - l[e]) * (h[e] - l[e]);
    diag = std::sqrt(diag);
    for (int e = 0; e < dim; ++e) {
      l[e] -= kBoxInflation * diag;
      h[e] += kBoxInflation * diag;
      glo[e] = c == 0 ? l[e] : std::min(glo[e], l[e]);
      ghi[e] = c == 0 ? h[e] : std::max(ghi[e], h[e]);
    }
  }
  // uniform bin grid over the boxes: bin -> cells whose box meets it, ascending
  uint32_t nb = (uint32_t)std::floor(std::pow((double)nc, 1.0 / dim) + 1e-9);
  nb = std::max(1u, std::min(nb, 256u));
  g.nb = nb;
  for (int e = 0; e < dim; ++e) g.inv_w[e] = ghi[e] > glo[e] ? nb / (ghi[e] - glo[e]) : 0.0;
  const size_t n_bins = (size_t)ipow((int)nb, dim);
  std::vector<uint32_t> &boff = g.boff, &bidx = g.bidx;
  boff.assign(n_bins + 1, 0);
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<uint32_t> pos(boff.begin(), boff.end() - 1);
    for (size_t c = 0; c < nc; ++c) {
      uint32_t b0[3] = {0, 0, 0}, b1[3] = {0, 0, 0};
      for (int e = 0; e < dim; ++e) {
        b0[e] = g.bin_of(lo[c * dim + e], e);
        b1[e] = g.bin_of(hi[c * dim + e], e);
      }
      for (uint32_t bz = b0[2]; bz <= b1[2]; ++bz)
        for (uint32_t by = b0[1]; by <= b1[1]; ++by)
          for (uint32_t bx = b0[0]; bx <= b1[0]; ++bx) {
            const size_t b = bx + (size_t)nb * (by + (size_t)nb * bz);
            if (pass == 0) ++boff[b + 1];
            else bidx[pos[b]++] = (uint32_t)c;
          }
    }
    if (pass == 0) {
      for (size_t b = 0; b < n_bins; ++b) boff[b + 1] += boff[b];
      bidx.resize(boff[n_bins]);
    }
  }
}

std::vector<double> point_table(int n) {
  std::vector<double> t((size_t)n + (size_t)n * n, 0.0);
  gauss_abscissae_01(n, t.data());
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < n; ++k)
      if (k != j) t[n + j * n + k] = 1.0 / (t[j] - t[k]);
  return t;
}

void point_basis(int n, const double *table, double t, double *l, double *dl) {
  const double *g = table, *r = table + n;
  for (int j = 0; j < n; ++j) {
    double v = 1, d = 0;  // the product over k != j, and its derivative, built factor by factor
    for (int k = 0; k < n; ++k) {
      if (k == j) continue;
      const double f = (t - g[k]) * r[j * n + k];
      d = d * f + v * r[j * n + k];
      v *= f;
    }
    l[j] = v;
    dl[j] = d;
  }
}

int build_points_plan(int dim, uint32_t nd, uint32_t n_cells, uint32_t n_dofs, const uint32_t *loc2glob,
                      const uint8_t *constrained, const uint32_t *cell, const double *xi, uint32_t n, PointsPlan &plan) {
  plan = PointsPlan();
  plan.n = n;
  // counting sort by cell, stable; the points without a cell go last
  std::vector<uint32_t> first((size_t)n_cells + 2, 0);
  for (uint32_t k = 0; k < n; ++k) {
    if (cell[k] != MFGPU_POINT_NOT_FOUND) {
      if (cell[k] >= n_cells) {
        set_error("mfgpu_points_create_in_cells: cell index out of range");
        return MFGPU_EINVAL;
      }
      for (int d = 0; d < dim; ++d)
        if (!(xi[(size_t)k * dim + d] >= 0.0 && xi[(size_t)k * dim + d] <= 1.0)) {
          set_error("mfgpu_points_create_in_cells: xi outside [0, 1]");
          return MFGPU_EINVAL;
        }
    }
    ++first[(cell[k] == MFGPU_POINT_NOT_FOUND ? n_cells : cell[k]) + 1];
  }
  for (size_t c = 0; c <= n_cells; ++c) first[c + 1] += first[c];
  plan.n_found = first[n_cells];
  plan.perm.resize(n);
  plan.xi.resize((size_t)plan.n_found * dim);
  {
    std::vector<uint32_t> pos(first.begin(), first.end() - 1);
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t s = pos[cell[k] == MFGPU_POINT_NOT_FOUND ? n_cells : cell[k]]++;
      plan.perm[s] = k;
      if (s < plan.n_found)
        for (int d = 0; d < dim; ++d) plan.xi[(size_t)s * dim + d] = xi[(size_t)k * dim + d];
    }
  }
  for (uint32_t c = 0; c < n_cells; ++c)
    for (uint32_t b = first[c]; b < first[c + 1]; b += kPointsPerItem) {
      const uint32_t item[kItemWords] = {c, b, std::min(kPointsPerItem, first[c + 1] - b), 0u};
      plan.items.insert(plan.items.end(), item, item + kItemWords);
    }
  // dof -> slot CSR, slots ascending
  const uint32_t ni = plan.n_items();
  if ((uint64_t)ni * nd > 0xffffffffull) {
    set_error("mfgpu_points_create_in_cells: more than 2^32 local entries");
    return MFGPU_EUNSUPPORTED;
  }
  plan.off.assign((size_t)n_dofs + 1, 0);
  auto listed = [&](uint32_t w, uint32_t i) { return loc2glob[(size_t)plan.items[(size_t)w * kItemWords] * nd + i]; };
  for (uint32_t w = 0; w < ni; ++w)
    for (uint32_t i = 0; i < nd; ++i)
      if (!constrained[listed(w, i)]) ++plan.off[listed(w, i) + 1];
  for (uint32_t i = 0; i < n_dofs; ++i) plan.off[i + 1] += plan.off[i];
  plan.idx.resize(plan.off[n_dofs]);
  std::vector<uint32_t> pos(plan.off.begin(), plan.off.end() - 1);
  for (uint32_t w = 0; w < ni; ++w)
    for (uint32_t i = 0; i < nd; ++i)
      if (!constrained[listed(w, i)]) plan.idx[pos[listed(w, i)]++] = w * nd + i;
  return 0;
}

}  // namespace mfgpu

using namespace mfgpu;

int mfgpu_locate_points(const mfgpu_desc *desc, const double *x, uint32_t n, uint32_t *cell, double *xi,
                        uint32_t *n_not_found) {
  if (n_not_found) *n_not_found = 0;
  if (!desc || (n && (!x || !cell || !xi))) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  const mfgpu_desc &d = *desc;
  if (d.number_type == MFGPU_F32) {
    set_error("mfgpu_locate_points: MFGPU_F64 only");
    return MFGPU_EUNSUPPORTED;
  }
  if (d.number_type != MFGPU_F64) {
    set_error("number_type must be MFGPU_F64");
    return MFGPU_EINVAL;
  }
  if ((d.dim != 2 && d.dim != 3) || d.degree < 1 || d.degree > 6) {
    set_error("mfgpu_locate_points: dim 2 or 3, degree 1..6");
    return MFGPU_EUNSUPPORTED;
  }
  if (!d.quadrature_points || d.n_cells == 0) {
    set_error("mfgpu_locate_points: quadrature_points and cells are required");
    return MFGPU_EINVAL;
  }
  const int dim = d.dim, N = d.degree + 1;
  const size_t nd = (size_t)ipow(N, dim), nc = d.n_cells;
  const double *xq = (const double *)d.quadrature_points;
  const std::vector<double> table = point_table(N);
  LocatorGrid g;
  build_locator_grid(dim, N, nc, xq, g);
  const std::vector<double> &lo = g.lo, &hi = g.hi;
  const std::vector<uint32_t> &boff = g.boff, &bidx = g.bidx;
  std::vector<double> y(nd * dim);
  uint32_t missing = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const double *xk = x + (size_t)k * dim;
    cell[k] = MFGPU_POINT_NOT_FOUND;
    for (int e = 0; e < dim; ++e) xi[(size_t)k * dim + e] = 0.0;
    bool inside = true;
    for (int e = 0; e < dim; ++e) inside = inside && xk[e] >= g.glo[e] && xk[e] <= g.ghi[e];  // false for NaN
    if (inside) {
      size_t b = 0;
      for (int e = dim - 1; e >= 0; --e) b = b * g.nb + g.bin_of(xk[e], e);
      for (uint32_t j = boff[b]; j < boff[b + 1]; ++j) {  // ascending: the lowest accepting cell wins
        const size_t c = bidx[j];
        bool in_box = true;
        for (int e = 0; e < dim; ++e) in_box = in_box && xk[e] >= lo[c * dim + e] && xk[e] <= hi[c * dim + e];
        double t[3];
        if (in_box && newton_in_cell(dim, N, table.data(), xq + c * nd * dim, nd, xk, y.data(), t)) {
          cell[k] = (uint32_t)c;
          for (int e = 0; e < dim; ++e) xi[(size_t)k * dim + e] = t[e];
          break;
        }
      }
    }
    if (cell[k] == MFGPU_POINT_NOT_FOUND) ++missing;
  }
  if (n_not_found) *n_not_found = missing;
  return 0;
}
