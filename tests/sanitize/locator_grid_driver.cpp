// The candidate grid of point location (build_locator_grid, csrc/mfgpu_points_locate.cpp: the one grid the host search
// and the device locator share) under AddressSanitizer + UBSan (CPU build only), on the meshes of
// tests/test_points_host.py (uniform, one refined cell, adaptive, ball; 2D and 3D; p = 1, 2, 4):
//   - every cell is listed, in ascending order, in every bin its box meets (the bins' extents restated here, a cell
//     whose box only touches a bin's boundary to rounding may or may not be listed), and in the bin of every point its
//     box holds;
//   - every bin list is sorted and free of duplicates, the CSR is consistent;
//   - mfgpu_locate_points, which searches through the grid, equals a search over ALL cells without boxes and bins
//     (newton_in_cell per cell, the lowest accepting cell wins): cells and xi bit for bit.
// Built and run by tests/test_locator_sanitizers.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mfgpu.h"
#include "mfgpu_points.h"

using mfgpu::LocatorGrid;

static int bad = 0;
static void expect(bool ok, const std::string &what) {
  if (!ok) {
    std::printf("FAILED: %s (%s)\n", what.c_str(), mfgpu_last_error());
    ++bad;
  }
}

static uint32_t rng_state = 2463534242u;
static double rnd() {  // xorshift32 -> [0, 1)
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state / 4294967296.0;
}

static size_t ipow(size_t a, int e) { return e == 0 ? 1 : a * ipow(a, e - 1); }

static bool listed(const LocatorGrid &g, size_t b, uint32_t c) {
  for (uint32_t j = g.boff[b]; j < g.boff[b + 1]; ++j)
    if (g.bidx[j] == c) return true;
  return false;
}

static void run_mesh(mfgpu_mesh *m, const std::string &tag) {
  mfgpu_desc d;
  std::memset(&d, 0, sizeof d);
  expect(m && mfgpu_mesh_desc(m, &d) == 0, tag + ": mesh");
  if (!m) return;
  const int dim = d.dim, N = d.degree + 1;
  const size_t nc = d.n_cells, nd = ipow(N, dim);
  const double *xq = (const double *)d.quadrature_points;
  LocatorGrid g;
  mfgpu::build_locator_grid(dim, N, nc, xq, g);
  const size_t n_bins = ipow(g.nb, dim);
  // the CSR; sorted lists without duplicates
  bool ok = g.nb >= 1 && g.lo.size() == nc * dim && g.hi.size() == nc * dim && g.boff.size() == n_bins + 1 &&
            g.boff[0] == 0 && g.boff[n_bins] == g.bidx.size();
  expect(ok, tag + ": sizes");
  if (!ok) return;
  for (size_t b = 0; ok && b < n_bins; ++b) {
    ok = g.boff[b] <= g.boff[b + 1];
    for (uint32_t j = g.boff[b]; ok && j < g.boff[b + 1]; ++j)
      ok = g.bidx[j] < nc && (j == g.boff[b] || g.bidx[j - 1] < g.bidx[j]);
  }
  expect(ok, tag + ": bin lists ascending, no duplicates");
  // boxes inside the global box; every cell in every bin its box meets
  ok = true;
  for (size_t c = 0; ok && c < nc; ++c)
    for (int e = 0; e < dim; ++e)
      ok = ok && g.lo[c * dim + e] <= g.hi[c * dim + e] && g.lo[c * dim + e] >= g.glo[e] && g.hi[c * dim + e] <= g.ghi[e];
  expect(ok, tag + ": boxes");
  size_t unlisted = 0, entries = 0;
  for (size_t b = 0; b < n_bins; ++b) {
    size_t rest = b;
    double blo[3], bhi[3];
    for (int e = 0; e < dim; ++e) {
      const size_t be = rest % g.nb;
      rest /= g.nb;
      const double w = (g.ghi[e] - g.glo[e]) / g.nb;
      blo[e] = g.glo[e] + be * w + 1e-9 * w;  // the bin's interior: what touches only its boundary is free
      bhi[e] = g.glo[e] + (be + 1) * w - 1e-9 * w;
    }
    for (size_t c = 0; c < nc; ++c) {
      bool meets = true;
      for (int e = 0; e < dim; ++e) meets = meets && g.lo[c * dim + e] <= bhi[e] && g.hi[c * dim + e] >= blo[e];
      if (meets) {
        ++entries;
        unlisted += !listed(g, b, (uint32_t)c);
      }
    }
  }
  expect(unlisted == 0 && entries <= g.bidx.size() && entries >= nc, tag + ": every cell in every bin its box meets");
  // the points: all dofs, pseudo-random points in and around the domain, far outside, NaN
  const double *coords = nullptr;
  const int64_t ncoord = mfgpu_mesh_dof_coords(m, &coords);
  std::vector<double> x(coords, coords + ncoord);
  for (int k = 0; k < 300; ++k)
    for (int e = 0; e < dim; ++e) x.push_back(-1.2 + 2.4 * rnd());
  for (int k = 0; k < 4; ++k)
    for (int e = 0; e < dim; ++e) x.push_back(e == k % dim ? (k < 2 ? 2.0 : -2.0) : 0.1);
  x.push_back(std::nan(""));
  for (int e = 1; e < dim; ++e) x.push_back(0.0);
  const uint32_t n = (uint32_t)(x.size() / dim);
  // the bin of a point lists every cell whose box holds the point
  ok = true;
  for (uint32_t k = 0; ok && k < n; ++k) {
    const double *xk = &x[(size_t)k * dim];
    bool inside = true;
    for (int e = 0; e < dim; ++e) inside = inside && xk[e] >= g.glo[e] && xk[e] <= g.ghi[e];
    if (!inside) continue;
    size_t b = 0;
    for (int e = dim - 1; e >= 0; --e) b = b * g.nb + g.bin_of(xk[e], e);
    ok = b < n_bins;
    for (size_t c = 0; ok && c < nc; ++c) {
      bool in_box = true;
      for (int e = 0; e < dim; ++e) in_box = in_box && xk[e] >= g.lo[c * dim + e] && xk[e] <= g.hi[c * dim + e];
      ok = !in_box || listed(g, b, (uint32_t)c);
    }
  }
  expect(ok, tag + ": a point's bin lists every cell whose box holds it");
  // through the grid == over all cells
  std::vector<uint32_t> cell(n);
  std::vector<double> xi((size_t)n * dim), y(nd * dim);
  uint32_t missing = 0, count = 0;
  expect(mfgpu_locate_points(&d, x.data(), n, cell.data(), xi.data(), &missing) == 0, tag + ": locate");
  const std::vector<double> table = mfgpu::point_table(N);
  ok = true;
  for (uint32_t k = 0; ok && k < n; ++k) {
    uint32_t want = MFGPU_POINT_NOT_FOUND;
    double t[3] = {0, 0, 0}, got[3];
    for (size_t c = 0; c < nc; ++c)
      if (mfgpu::newton_in_cell(dim, N, table.data(), xq + c * nd * dim, nd, &x[(size_t)k * dim], y.data(), got)) {
        want = (uint32_t)c;
        for (int e = 0; e < dim; ++e) t[e] = got[e];
        break;
      }
    count += want == MFGPU_POINT_NOT_FOUND;
    ok = cell[k] == want;
    for (int e = 0; ok && e < dim; ++e) ok = xi[(size_t)k * dim + e] == t[e];
    if (!ok) std::printf("point %u: cell %u, over all cells %u\n", k, cell[k], want);
  }
  expect(ok && count == missing && missing >= 5, tag + ": the search through the grid equals the search over all cells");
  mfgpu_mesh_destroy(m);
}

int main() {
  for (int dim = 2; dim <= 3; ++dim)
    for (int p : {1, 2, 4}) {
      const std::string tag = std::to_string(dim) + "D p=" + std::to_string(p);
      mfgpu_mesh *m = nullptr;
      const uint32_t npd[3] = {3, 2, 2};
      mfgpu_mesh_create_uniform(dim, p, npd, -1.0, 1.0, 0, 0, MFGPU_F64, &m);
      run_mesh(m, "uniform " + tag);
      std::vector<uint32_t> leaves;  // 2^dim cells of level 1, the first one refined
      for (int lv = 2; lv >= 1; --lv)
        for (uint32_t z = 0; z < (dim == 3 ? 2u : 1u); ++z)
          for (uint32_t y = 0; y < 2; ++y)
            for (uint32_t x = 0; x < 2; ++x)
              if (lv == 2 || x + y + z > 0) leaves.insert(leaves.end(), {(uint32_t)lv, x, y, z});
      m = nullptr;
      mfgpu_mesh_create_from_leaves(dim, p, leaves.data(), (uint32_t)(leaves.size() / 4), MFGPU_F64, &m);
      run_mesh(m, "one refined " + tag);
      m = nullptr;
      mfgpu_mesh_create_adaptive(dim, p, 2, MFGPU_F64, &m);
      run_mesh(m, "adaptive " + tag);
      for (int n_ref = 0; n_ref <= 1; ++n_ref) {
        m = nullptr;
        mfgpu_mesh_create_ball(dim, p, n_ref, MFGPU_F64, &m);
        run_mesh(m, "ball " + std::to_string(n_ref) + " " + tag);
      }
    }
  std::printf("done bad=%d\n", bad);
  return bad ? 1 : 0;
}
