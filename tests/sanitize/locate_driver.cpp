// Point location and the host half of mfgpu_points_create_in_cells under AddressSanitizer + UBSan (CPU build only):
// mfgpu_locate_points over the meshes of tests/test_points_host.py (uniform, one refined cell, adaptive, ball; 2D and 3D;
// p = 1, 2, 4) on the coordinates of all dofs, pseudo-random points in and around the domain and points far outside;
// build_points_plan (sorting, work items, the dof -> slot CSR) on what it returns and on one cell holding more points than
// a work item; every output checked in plain loops; the inputs both refuse.
// Built and run by tests/test_points_sanitizers.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mfgpu.h"
#include "mfgpu_points.h"

using mfgpu::kItemWords;
using mfgpu::kPointsPerItem;
using mfgpu::PointsPlan;

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

static int ipow(int a, int e) { return e == 0 ? 1 : a * ipow(a, e - 1); }

static void check_plan(const mfgpu_desc &d, const std::vector<uint32_t> &cell, const std::vector<double> &xi,
                       const std::string &tag) {
  const int dim = d.dim;
  const uint32_t nd = (uint32_t)ipow(d.degree + 1, dim), n = (uint32_t)cell.size();
  std::vector<uint8_t> con(d.n_dofs, 0);
  for (uint32_t i = 0; i < d.n_constrained; ++i) con[d.constrained_dofs[i]] = 1;
  PointsPlan plan;
  const int rc = mfgpu::build_points_plan(dim, nd, d.n_cells, d.n_dofs, d.loc2glob, con.data(), cell.data(), xi.data(), n, plan);
  expect(rc == 0, tag + ": build_points_plan");
  if (rc) return;
  // perm: a permutation, found points first, sorted by cell, stable
  std::vector<uint8_t> seen(n, 0);
  bool ok = plan.perm.size() == n && plan.xi.size() == (size_t)plan.n_found * dim;
  for (uint32_t s = 0; ok && s < n; ++s) {
    const uint32_t k = plan.perm[s];
    ok = k < n && !seen[k];
    if (!ok) break;
    seen[k] = 1;
    ok = (cell[k] != MFGPU_POINT_NOT_FOUND) == (s < plan.n_found);
    if (ok && s > 0 && s < plan.n_found) {
      const uint32_t kp = plan.perm[s - 1];
      ok = cell[kp] < cell[k] || (cell[kp] == cell[k] && kp < k);
    }
    for (int e = 0; ok && s < plan.n_found && e < dim; ++e) ok = plan.xi[(size_t)s * dim + e] == xi[(size_t)k * dim + e];
  }
  expect(ok, tag + ": permutation");
  // items: consecutive, one cell each, bounded, covering the found points
  uint32_t next = 0;
  ok = plan.items.size() % kItemWords == 0;
  for (uint32_t w = 0; ok && w < plan.n_items(); ++w) {
    const uint32_t *it = &plan.items[(size_t)w * kItemWords];
    ok = it[0] < d.n_cells && it[1] == next && it[2] >= 1 && it[2] <= kPointsPerItem && it[1] + it[2] <= plan.n_found;
    for (uint32_t j = 0; ok && j < it[2]; ++j) ok = cell[plan.perm[it[1] + j]] == it[0];
    next += it[2];
  }
  expect(ok && next == plan.n_found, tag + ": work items");
  // CSR: ascending slots, every unconstrained listed position exactly once
  ok = plan.off.size() == (size_t)d.n_dofs + 1 && plan.off[0] == 0 && plan.off[d.n_dofs] == plan.idx.size();
  size_t want = 0;
  for (uint32_t w = 0; ok && w < plan.n_items(); ++w)
    for (uint32_t i = 0; i < nd; ++i) want += !con[d.loc2glob[(size_t)plan.items[(size_t)w * kItemWords] * nd + i]];
  ok = ok && want == plan.idx.size();
  for (uint32_t i = 0; ok && i < d.n_dofs; ++i) {
    ok = plan.off[i] <= plan.off[i + 1] && (!con[i] || plan.off[i] == plan.off[i + 1]);
    for (uint32_t j = plan.off[i]; ok && j < plan.off[i + 1]; ++j) {
      const uint32_t slot = plan.idx[j], w = slot / nd, li = slot % nd;
      ok = w < plan.n_items() && d.loc2glob[(size_t)plan.items[(size_t)w * kItemWords] * nd + li] == i &&
           (j == plan.off[i] || plan.idx[j - 1] < slot);
    }
  }
  expect(ok, tag + ": CSR");
}

static void run_mesh(mfgpu_mesh *m, const std::string &tag) {
  mfgpu_desc d;
  std::memset(&d, 0, sizeof d);
  expect(m && mfgpu_mesh_desc(m, &d) == 0, tag + ": mesh");
  if (!m) return;
  const int dim = d.dim;
  const double *coords = nullptr;
  const int64_t nc = mfgpu_mesh_dof_coords(m, &coords);
  std::vector<double> x(coords, coords + nc);
  const size_t n_dof_points = x.size() / dim;
  for (int k = 0; k < 200; ++k)
    for (int e = 0; e < dim; ++e) x.push_back(-1.2 + 2.4 * rnd());
  for (int k = 0; k < 4; ++k)
    for (int e = 0; e < dim; ++e) x.push_back(e == k % dim ? (k < 2 ? 2.0 : -2.0) : 0.1);
  x.push_back(std::nan(""));
  for (int e = 1; e < dim; ++e) x.push_back(0.0);
  const uint32_t n = (uint32_t)(x.size() / dim);
  std::vector<uint32_t> cell(n);
  std::vector<double> xi((size_t)n * dim);
  uint32_t missing = 0;
  expect(mfgpu_locate_points(&d, x.data(), n, cell.data(), xi.data(), &missing) == 0, tag + ": locate");
  uint32_t count = 0;
  bool ok = true;
  for (uint32_t k = 0; k < n; ++k) {
    if (cell[k] == MFGPU_POINT_NOT_FOUND) {
      ++count;
      ok = ok && k >= n_dof_points;  // every dof lies in the mesh
      for (int e = 0; e < dim; ++e) ok = ok && xi[(size_t)k * dim + e] == 0.0;
    } else {
      ok = ok && cell[k] < d.n_cells;
      for (int e = 0; e < dim; ++e) ok = ok && xi[(size_t)k * dim + e] >= 0.0 && xi[(size_t)k * dim + e] <= 1.0;
    }
  }
  expect(ok && count == missing && missing >= 5, tag + ": located cells and xi");
  check_plan(d, cell, xi, tag);
  // one cell with more points than two work items hold, the others empty; then no point at all, then none found
  const uint32_t many = 2 * kPointsPerItem + 7;
  std::vector<uint32_t> c1(many, d.n_cells - 1);
  std::vector<double> x1((size_t)many * dim);
  for (double &v : x1) v = rnd();
  check_plan(d, c1, x1, tag + " one cell");
  check_plan(d, {}, {}, tag + " empty");
  check_plan(d, std::vector<uint32_t>(3, MFGPU_POINT_NOT_FOUND), std::vector<double>(3 * dim, 0.0), tag + " none found");
  // refused inputs
  PointsPlan plan;
  std::vector<uint8_t> con(d.n_dofs, 0);
  const uint32_t nd = (uint32_t)ipow(d.degree + 1, dim);
  const uint32_t cbad = d.n_cells;
  const std::vector<double> half(dim, 0.5);
  expect(mfgpu::build_points_plan(dim, nd, d.n_cells, d.n_dofs, d.loc2glob, con.data(), &cbad, half.data(), 1, plan) ==
             MFGPU_EINVAL, tag + ": cell out of range refused");
  const uint32_t c0 = 0;
  std::vector<double> out(dim, 0.5);
  out[dim - 1] = 1.0 + 1e-12;
  expect(mfgpu::build_points_plan(dim, nd, d.n_cells, d.n_dofs, d.loc2glob, con.data(), &c0, out.data(), 1, plan) ==
             MFGPU_EINVAL, tag + ": xi outside refused");
  out[dim - 1] = std::nan("");
  expect(mfgpu::build_points_plan(dim, nd, d.n_cells, d.n_dofs, d.loc2glob, con.data(), &c0, out.data(), 1, plan) ==
             MFGPU_EINVAL, tag + ": xi NaN refused");
  mfgpu_desc f32 = d;
  f32.number_type = MFGPU_F32;
  expect(mfgpu_locate_points(&f32, x.data(), 1, cell.data(), xi.data(), nullptr) == MFGPU_EUNSUPPORTED, tag + ": F32 refused");
  expect(mfgpu_locate_points(&d, x.data(), 0, nullptr, nullptr, &missing) == 0 && missing == 0, tag + ": n = 0");
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
