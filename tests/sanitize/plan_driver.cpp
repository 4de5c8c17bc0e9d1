// Host-side planner and mesh stand-ins under AddressSanitizer + UBSan (CPU build only: the GPU pool has no sanitizer runs):
// every mesh kind x degree -> description -> plan (batching, plane records, hanging-node records), then teardown; and
// the descriptions no stand-in produces -- periodic rings and tori, shuffled numberings and cell orders, a pinched
// vertex -- made here from a uniform mesh's arrays, with the plan's permutation and lmap checked in place.
// Built and run by tests/test_host_sanitizers.py.
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <map>
#include <numeric>
#include <random>
#include <vector>
#include "mfgpu.h"
static int plan_of(mfgpu_mesh *m, int kernel) {
  mfgpu_desc d;
  if (mfgpu_mesh_desc(m, &d)) return 1;
  d.kernel = kernel;
  mfgpu_plan *p = nullptr;
  int rc = mfgpu_plan_create(&d, &p);
  if (rc) { std::printf("plan rc=%d %s\n", rc, mfgpu_last_error()); return rc; }
  const uint32_t *ptr;
  long n16 = mfgpu_plan_array_u32(p, 16, &ptr), n15 = mfgpu_plan_array_u32(p, 15, &ptr), n0 = mfgpu_plan_array_u32(p, 0, &ptr);
  std::printf("  batches %ld hn_slot %ld hn words %ld\n", n0 - 1, n16, n15);
  mfgpu_plan_destroy(p);
  return 0;
}

// ---- a description with its own cell-to-dof map and constrained list (everything else is the mesh's)
struct Topo {
  mfgpu_mesh *mesh = nullptr;
  mfgpu_desc d;
  std::vector<uint32_t> l2g, con;
  std::vector<double> x;  // dof coordinates [n_dofs * dim]
  uint32_t nd = 0;
  ~Topo() { mfgpu_mesh_destroy(mesh); }
  void sync() {
    std::sort(con.begin(), con.end());
    con.erase(std::unique(con.begin(), con.end()), con.end());
    d.loc2glob = l2g.data();
    d.constrained_dofs = con.data();
    d.n_constrained = (uint32_t)con.size();
  }
};
static bool make_box(Topo &t, int dim, int p, uint32_t nx, uint32_t ny, uint32_t nz) {
  uint32_t n[3] = {nx, ny, nz};
  if (mfgpu_mesh_create_uniform(dim, p, n, -1, 1, 0, 0, 0, &t.mesh) || mfgpu_mesh_desc(t.mesh, &t.d)) return false;
  t.nd = 1;
  for (int k = 0; k < dim; ++k) t.nd *= (uint32_t)(p + 1);
  t.l2g.assign(t.d.loc2glob, t.d.loc2glob + (size_t)t.d.n_cells * t.nd);
  t.con.assign(t.d.constrained_dofs, t.d.constrained_dofs + t.d.n_constrained);
  const double *xc = nullptr;
  const int64_t cnt = mfgpu_mesh_dof_coords(t.mesh, &xc);
  if (cnt != (int64_t)t.d.n_dofs * dim) return false;
  t.x.assign(xc, xc + cnt);
  t.sync();
  return true;
}
// rename dof g to m[g] (not necessarily injective), then number the image densely
static void rename_dofs(Topo &t, std::vector<uint32_t> m, const std::vector<uint8_t> *constrained_old = nullptr) {
  const uint32_t N = t.d.n_dofs, dim = (uint32_t)t.d.dim;
  std::vector<uint32_t> rank(N, 0xffffffffu);
  for (uint32_t g = 0; g < N; ++g) rank[m[g]] = 0;
  uint32_t n_new = 0;
  for (uint32_t g = 0; g < N; ++g)
    if (rank[g] == 0) rank[g] = n_new++;
  for (uint32_t g = 0; g < N; ++g) m[g] = rank[m[g]];
  for (uint32_t &g : t.l2g) g = m[g];
  std::vector<uint32_t> con;
  if (constrained_old) {
    for (uint32_t g = 0; g < N; ++g)
      if ((*constrained_old)[g]) con.push_back(m[g]);
  } else {
    for (uint32_t g : t.con) con.push_back(m[g]);
  }
  t.con = con;
  std::vector<double> x((size_t)n_new * dim);
  for (uint32_t g = N; g-- > 0;)
    for (uint32_t k = 0; k < dim; ++k) x[(size_t)m[g] * dim + k] = t.x[(size_t)g * dim + k];
  t.x = x;
  t.d.n_dofs = n_new;
  t.sync();
}
// identify the hi face of every axis in `axes` (bits) with the lo face; constrained = the faces that remain boundary
static void make_periodic(Topo &t, unsigned axes) {
  const uint32_t N = t.d.n_dofs;
  const int dim = t.d.dim;
  auto key = [&](uint32_t g, int k) { return (int64_t)std::llround((t.x[(size_t)g * dim + k] + 1.0) * (1 << 28)); };
  int64_t lo[3], hi[3];
  for (int k = 0; k < dim; ++k) {
    lo[k] = hi[k] = key(0, k);
    for (uint32_t g = 1; g < N; ++g) lo[k] = std::min(lo[k], key(g, k)), hi[k] = std::max(hi[k], key(g, k));
  }
  std::vector<uint32_t> m(N);
  std::iota(m.begin(), m.end(), 0u);
  for (int a = 0; a < dim; ++a) {
    if (!((axes >> a) & 1)) continue;
    std::map<std::vector<int64_t>, uint32_t> on_lo;
    auto others = [&](uint32_t g) {
      std::vector<int64_t> v;
      for (int k = 0; k < dim; ++k)
        if (k != a) v.push_back(key(g, k));
      return v;
    };
    for (uint32_t g = 0; g < N; ++g)
      if (key(g, a) == lo[a]) on_lo[others(g)] = g;
    std::vector<uint32_t> r(N);
    std::iota(r.begin(), r.end(), 0u);
    for (uint32_t g = 0; g < N; ++g)
      if (key(g, a) == hi[a]) r[g] = on_lo.at(others(g));
    for (uint32_t g = 0; g < N; ++g) m[g] = r[m[g]];
  }
  std::vector<uint8_t> boundary(N, 0);
  for (int k = 0; k < dim; ++k)
    if (!((axes >> k) & 1))
      for (uint32_t g = 0; g < N; ++g) boundary[g] |= key(g, k) == lo[k] || key(g, k) == hi[k];
  rename_dofs(t, m, &boundary);
}
static void shuffle_dofs(Topo &t, unsigned seed) {
  std::vector<uint32_t> m(t.d.n_dofs);
  std::iota(m.begin(), m.end(), 0u);
  std::mt19937 rng(seed);
  std::shuffle(m.begin(), m.end(), rng);
  for (uint32_t &g : t.l2g) g = m[g];
  for (uint32_t &g : t.con) g = m[g];
  t.sync();
}
// (the planner reads loc2glob and the constrained list only: the quadrature arrays need not move with the cells here)
static void shuffle_cells(Topo &t, unsigned seed) {
  std::vector<uint32_t> order(t.d.n_cells), l2g(t.l2g.size());
  std::iota(order.begin(), order.end(), 0u);
  std::mt19937 rng(seed);
  std::shuffle(order.begin(), order.end(), rng);
  for (uint32_t c = 0; c < t.d.n_cells; ++c)
    std::copy_n(t.l2g.begin() + (size_t)order[c] * t.nd, t.nd, l2g.begin() + (size_t)c * t.nd);
  t.l2g = l2g;
  t.sync();
}
// identify the free dofs at cell corners into one
static void pinch_interior_vertices(Topo &t) {
  const uint32_t N = t.d.n_dofs, n = (uint32_t)t.d.degree + 1;
  std::vector<uint8_t> con(N, 0), vertex(N, 0);
  for (uint32_t g : t.con) con[g] = 1;
  for (uint32_t c = 0; c < t.d.n_cells; ++c)
    for (uint32_t k = 0; k < (1u << t.d.dim); ++k) {
      uint32_t li = 0, s = 1;
      for (int a = 0; a < t.d.dim; ++a, s *= n) li += ((k >> a) & 1) * (n - 1) * s;
      vertex[t.l2g[(size_t)c * t.nd + li]] = 1;
    }
  std::vector<uint32_t> m(N);
  std::iota(m.begin(), m.end(), 0u);
  uint32_t first = 0xffffffffu;
  for (uint32_t g = 0; g < N; ++g)
    if (vertex[g] && !con[g]) m[g] = first == 0xffffffffu ? (first = g) : first;
  rename_dofs(t, m);
}
// plan it; cell_order must be a permutation and bdofs[batch_dof_off[b] + lmap[pos][i]] the description's loc2glob
static int plan_checked(Topo &t, const char *what, int kernel, bool colored = false, int expect_rc = 0) {
  mfgpu_desc d = t.d;
  d.kernel = (uint32_t)kernel;
  if (colored) d.flags |= MFGPU_COLORED_SCATTER;
  mfgpu_plan *p = nullptr;
  const int rc = mfgpu_plan_create(&d, &p);
  if (rc != expect_rc) {
    std::printf("%s kernel %d: rc=%d (expected %d) %s\n", what, kernel, rc, expect_rc, mfgpu_last_error());
    if (!rc) mfgpu_plan_destroy(p);
    return 1;
  }
  if (rc) {
    std::printf("%s kernel %d: refused as expected: %s\n", what, kernel, mfgpu_last_error());
    return 0;
  }
  const uint32_t *bco, *bdo, *order, *bdofs;
  const uint16_t *lmap;
  const int64_t nb = mfgpu_plan_array_u32(p, 0, &bco) - 1, nb1 = mfgpu_plan_array_u32(p, 1, &bdo) - 1;
  const int64_t nc = mfgpu_plan_array_u32(p, 3, &order), nbd = mfgpu_plan_array_u32(p, 4, &bdofs);
  const int64_t nl = mfgpu_plan_lmap(p, &lmap);
  int bad = 0;
  if (nb < 1 || nb1 != nb || nc != (int64_t)d.n_cells || nl != nc * (int64_t)t.nd || bco[nb] != d.n_cells || bdo[nb] != nbd) bad = 1;
  std::vector<uint8_t> seen(d.n_cells, 0);
  for (int64_t c = 0; c < nc && !bad; ++c) {
    if (order[c] >= d.n_cells || seen[order[c]]) bad = 2;
    else seen[order[c]] = 1;
  }
  for (int64_t b = 0; b < nb && !bad; ++b)
    for (uint32_t pos = bco[b]; pos < bco[b + 1] && !bad; ++pos)
      for (uint32_t i = 0; i < t.nd && !bad; ++i) {
        const uint32_t l = lmap[(size_t)pos * t.nd + i];
        if (l >= bdo[b + 1] - bdo[b]) bad = 3;
        else if ((bdofs[bdo[b] + l] & 0x7fffffffu) != t.l2g[(size_t)order[pos] * t.nd + i]) bad = 4;
      }
  const uint32_t *pr;
  std::printf("%s kernel %d%s: batches %ld plane-record words %ld%s\n", what, kernel, colored ? " coloured" : "", (long)nb,
              (long)mfgpu_plan_array_u32(p, 13, &pr), bad ? "  INCONSISTENT" : "");
  if (bad) std::printf("  check %d failed\n", bad);
  mfgpu_plan_destroy(p);
  return bad;
}
static int topologies() {
  int bad = 0;
  char what[96];
  const int kernels[3] = {0, 3, 4};
  // x-periodic rings of 2, 3 and 4 cells (the +x walk of a box comes back to its seed), and of 1 (x-face dofs twice)
  for (int p = 3; p <= 6; ++p)
    for (uint32_t nx = 1; nx <= 4; ++nx)
      for (int kernel : kernels) {
        Topo t;
        if (!make_box(t, 3, p, nx, 4, 4)) return 1;
        make_periodic(t, 1);
        std::snprintf(what, sizeof what, "ring%u p=%d", nx, p);
        bad |= plan_checked(t, what, kernel);
      }
  for (int variant = 0; variant < 3; ++variant)
    for (int kernel : kernels) {
      Topo t;
      if (!make_box(t, 3, 4, 3, 3, 3)) return 1;
      make_periodic(t, 7);
      if (variant >= 1) shuffle_dofs(t, 5);
      if (variant >= 2) shuffle_cells(t, 6);
      std::snprintf(what, sizeof what, "torus 3x3x3 p=4 variant %d", variant);
      bad |= plan_checked(t, what, kernel);
      if (kernel == 0) bad |= plan_checked(t, what, kernel, true);
    }
  for (int p = 1; p <= 2; ++p) {
    Topo t;
    if (!make_box(t, 3, p, 2, 2, 2)) return 1;
    make_periodic(t, 7);
    std::snprintf(what, sizeof what, "torus 2x2x2 p=%d", p);
    bad |= plan_checked(t, what, 0) | plan_checked(t, what, 0, true);
  }
  for (int variant = 1; variant < 4; ++variant)
    for (int kernel : kernels) {
      Topo t;
      if (!make_box(t, 3, 4, 3, 4, 4)) return 1;
      if (variant & 1) shuffle_dofs(t, 7);
      if (variant & 2) shuffle_cells(t, 8);
      std::snprintf(what, sizeof what, "shuffled box 3x4x4 p=4 variant %d", variant);
      bad |= plan_checked(t, what, kernel);
    }
  for (int p = 2; p <= 4; p += 2)
    for (uint32_t one_cell = 0; one_cell < 2; ++one_cell) {
      Topo t;
      if (!make_box(t, 3, p, 3, 3, 3)) return 1;
      pinch_interior_vertices(t);
      t.d.max_cells_per_batch = one_cell;
      std::snprintf(what, sizeof what, "pinch27 p=%d max_cells %u", p, one_cell);
      bad |= plan_checked(t, what, 0) | plan_checked(t, what, 0, true);
      if (p == 4) bad |= plan_checked(t, what, 3) | plan_checked(t, what, 4);
    }
  {  // 2D: ring, torus, 1-ring, pinch
    Topo a, b, c, e;
    if (!make_box(a, 2, 2, 2, 5, 1) || !make_box(b, 2, 4, 3, 3, 1) || !make_box(c, 2, 3, 1, 4, 1) || !make_box(e, 2, 3, 6, 6, 1)) return 1;
    make_periodic(a, 1);
    make_periodic(b, 3);
    make_periodic(c, 1);
    pinch_interior_vertices(e);
    bad |= plan_checked(a, "2D ring2 p=2", 0) | plan_checked(b, "2D torus p=4", 0) | plan_checked(c, "2D ring1 p=3", 0) |
           plan_checked(e, "2D pinch p=3", 0) | plan_checked(b, "2D torus p=4", 0, true);
  }
  {  // the loud limit: a vertex 125 one-cell batches touch needs 125 batch colours
    Topo t;
    if (!make_box(t, 3, 2, 5, 5, 5)) return 1;
    pinch_interior_vertices(t);
    t.d.max_cells_per_batch = 1;
    bad |= plan_checked(t, "pinch125 p=2", 0, false, MFGPU_EUNSUPPORTED);
  }
  return bad;
}
int main() {
  int bad = 0;
  for (int p = 2; p <= 6; ++p)
    for (int nref = 3; nref <= 4; ++nref) {
      mfgpu_mesh *m = nullptr;
      if (mfgpu_mesh_create_adaptive(3, p, nref, 0, &m)) { std::printf("mesh fail\n"); return 1; }
      std::printf("adaptive p=%d nref=%d\n", p, nref);
      bad |= plan_of(m, 0);
      mfgpu_mesh_destroy(m);
    }
  for (int p = 3; p <= 6; ++p) {
    uint32_t n[3] = {7, 8, 10};
    mfgpu_mesh *m = nullptr;
    if (mfgpu_mesh_create_uniform(3, p, n, -1, 1, 2, 7, 0, &m)) { std::printf("mesh fail\n"); return 1; }
    std::printf("uniform slab p=%d\n", p);
    bad |= plan_of(m, 0);
    mfgpu_mesh_destroy(m);
  }
  { mfgpu_mesh *m = nullptr; mfgpu_mesh_create_ball(3, 4, 2, 0, &m); std::printf("ball\n"); bad |= plan_of(m, 0); mfgpu_mesh_destroy(m); }
  bad |= topologies();
  std::printf("done bad=%d\n", bad);
  return bad;
}
