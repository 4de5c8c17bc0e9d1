// Adaptive mesh stand-in (host only): single-root octree/quadtree on hyper_cube(-1,1) with the
// refinement recipe of bmop's ADAPTIVE_GRID (reference bmop_common.h:49-105), one-irregular
// (2:1 over faces and, in 3D, edges, as deal.II's execute_coarsening_and_refinement enforces),
// FE_Q(p) dofs with separate hanging-node dofs, and the per-cell hanging-node data the GPU path
// needs: constraint mask (hanging_nodes.cuh:23-53) and loc2glob with constrained face / edge entries
// replaced by the coarse neighbour's dofs (HangingNodes::setup_constraints, :209-454).
//
// On a single-root octree every face orientation is standard, so the rotation / flip branches of the
// reference (:285-302, :457-578) never trigger; the mask and substitution logic is the same.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <unordered_set>

#include "mfgpu_mesh.h"

namespace mfgpu {
namespace {

struct Cell {
  int level;
  uint32_t c[3];
};

inline uint64_t ckey(int level, const uint32_t *c) {
  return ((uint64_t)level << 57) | ((uint64_t)c[2] << 38) | ((uint64_t)c[1] << 19) | (uint64_t)c[0];
}

struct Tree {
  int dim;
  std::unordered_set<uint64_t> active;  // leaves
  int max_level = 0;
  bool balance_vertices = false;  // Triangulation::limit_level_difference_at_vertices (poisson_mg.cu:131)

  bool is_active(int l, const uint32_t *c) const { return active.count(ckey(l, c)) != 0; }

  // level of the leaf covering cell (l, c) or any ancestor of it; -1 if (l,c) is refined further
  // (i.e. the covering leaves are finer) or outside the domain.
  int covering_level(int l, const int64_t *ci) const {
    uint32_t c[3] = {0, 0, 0};
    for (int d = 0; d < dim; ++d) {
      if (ci[d] < 0 || ci[d] >= ((int64_t)1 << l)) return -2;  // outside
      c[d] = (uint32_t)ci[d];
    }
    for (int ll = l; ll >= 0; --ll) {
      if (is_active(ll, c)) return ll;
      for (int d = 0; d < dim; ++d) c[d] >>= 1;
    }
    return -1;  // finer leaves
  }

  void refine(const Cell &cell) {
    active.erase(ckey(cell.level, cell.c));
    for (int k = 0; k < (1 << dim); ++k) {
      uint32_t c[3] = {0, 0, 0};
      for (int d = 0; d < dim; ++d) c[d] = 2 * cell.c[d] + ((k >> d) & 1);
      active.insert(ckey(cell.level + 1, c));
    }
    max_level = std::max(max_level, cell.level + 1);
  }

  std::vector<Cell> leaves() const {
    std::vector<Cell> v;
    v.reserve(active.size());
    for (uint64_t k : active) {
      Cell c;
      c.level = (int)(k >> 57);
      c.c[0] = (uint32_t)(k & 0x7ffff);
      c.c[1] = (uint32_t)((k >> 19) & 0x7ffff);
      c.c[2] = (uint32_t)((k >> 38) & 0x7ffff);
      v.push_back(c);
    }
    return v;
  }

  // refine the flagged leaves and whatever else is needed to stay one-irregular over faces and
  // (3D) edges: a leaf next to a flagged leaf of HIGHER level is flagged too, until stable.
  void refine_flagged(std::vector<Cell> flagged) {
    std::unordered_set<uint64_t> flag;
    for (const Cell &c : flagged) flag.insert(ckey(c.level, c.c));
    std::vector<Cell> work = flagged;
    while (!work.empty()) {
      std::vector<Cell> next;
      for (const Cell &c : work) {
        // neighbours over faces and edges at the cell's own level
        for (int ox = -1; ox <= 1; ++ox)
          for (int oy = -1; oy <= 1; ++oy)
            for (int oz = (dim == 3 ? -1 : 0); oz <= (dim == 3 ? 1 : 0); ++oz) {
              const int nz = (ox != 0) + (oy != 0) + (oz != 0);
              if (nz == 0) continue;
              if (!balance_vertices) {
                if (nz > 2) continue;               // faces (1) and edges (2); not vertices
                if (dim == 2 && nz == 2) continue;  // 2D: faces only
              }
              int64_t ci[3] = {(int64_t)c.c[0] + ox, (int64_t)c.c[1] + oy, (int64_t)c.c[2] + oz};
              const int lv = covering_level(c.level, ci);
              if (lv >= 0 && lv < c.level) {
                // the covering leaf is coarser: it must be refined as well
                Cell nb;
                nb.level = lv;
                for (int d = 0; d < 3; ++d) nb.c[d] = d < dim ? (uint32_t)(ci[d] >> (c.level - lv)) : 0u;
                if (flag.insert(ckey(nb.level, nb.c)).second) next.push_back(nb);
              }
            }
      }
      work.swap(next);
    }
    // refine coarse-to-fine so that parents exist as leaves when their turn comes
    std::vector<Cell> all;
    for (uint64_t k : flag) {
      Cell c;
      c.level = (int)(k >> 57);
      c.c[0] = (uint32_t)(k & 0x7ffff);
      c.c[1] = (uint32_t)((k >> 19) & 0x7ffff);
      c.c[2] = (uint32_t)((k >> 38) & 0x7ffff);
      all.push_back(c);
    }
    std::sort(all.begin(), all.end(), [](const Cell &a, const Cell &b) { return a.level < b.level; });
    for (const Cell &c : all)
      if (is_active(c.level, c.c)) refine(c);
  }
};

struct DofKey {
  int level;
  uint32_t k[3];
  uint8_t i[3];
  bool operator==(const DofKey &o) const {
    return level == o.level && k[0] == o.k[0] && k[1] == o.k[1] && k[2] == o.k[2] && i[0] == o.i[0] &&
           i[1] == o.i[1] && i[2] == o.i[2];
  }
};
struct DofKeyHash {
  size_t operator()(const DofKey &a) const {
    uint64_t h = (uint64_t)a.level * 0x9E3779B97F4A7C15ull;
    for (int d = 0; d < 3; ++d) {
      h ^= ((uint64_t)a.k[d] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2));
      h ^= ((uint64_t)a.i[d] + 0x517cc1b727220a95ull + (h << 6) + (h >> 2));
    }
    return (size_t)h;
  }
};

// Structural identity of the node (i0,i1,i2) of a cell: per direction the lattice coordinate of the
// entity at the cell's level (high boundary -> next cell's low boundary); pure vertices are moved to
// the coarsest level on which they are lattice points.  Nodes of a fine edge / face lying on a coarse
// edge / face keep the fine level: they are the separate hanging-node dofs deal.II creates.
DofKey dof_key(int dim, int p, const Cell &c, const int *idx) {
  DofKey key;
  key.level = c.level;
  bool vertex = true;
  for (int d = 0; d < 3; ++d) {
    if (d >= dim) {
      key.k[d] = 0;
      key.i[d] = 0;
      continue;
    }
    if (idx[d] == p) {
      key.k[d] = c.c[d] + 1;
      key.i[d] = 0;
    } else {
      key.k[d] = c.c[d];
      key.i[d] = (uint8_t)idx[d];
      if (idx[d] != 0) vertex = false;
    }
  }
  if (vertex) {
    while (key.level > 0) {
      bool even = true;
      for (int d = 0; d < dim; ++d) even = even && (key.k[d] % 2 == 0);
      if (!even) break;
      for (int d = 0; d < dim; ++d) key.k[d] >>= 1;
      key.level--;
    }
  }
  return key;
}

}  // namespace

int build_adaptive(Mesh &M, int n_ref, bool balance_vertices) {
  const int dim = M.dim, p = M.degree, n = p + 1, nd = ipow(n, dim);
  if (n_ref < 0 || n_ref > 12) {
    set_error("mfgpu_mesh_create_adaptive: n_ref out of range");
    return MFGPU_EINVAL;
  }
  M.init_tables();
  Tree T;
  T.dim = dim;
  T.balance_vertices = balance_vertices;
  {
    uint32_t c0[3] = {0, 0, 0};
    T.active.insert(ckey(0, c0));
  }
  // pseudo_adaptive_refinement (bmop_common.h:49-105), CUBE domain
  const int nglob = std::max(n_ref - 2, 0);
  for (int r = 0; r < nglob; ++r) T.refine_flagged(T.leaves());
  const double reduction = dim == 2 ? 0.005 : 0.015;
  auto center = [&](const Cell &c, double *x) {
    const double h = 2.0 / (double)(1u << c.level);
    for (int d = 0; d < dim; ++d) x[d] = -1.0 + h * (c.c[d] + 0.5);
  };
  auto annulus = [&](double R, double r, const double *ctr) {
    std::vector<Cell> fl;
    for (const Cell &c : T.leaves()) {
      double x[3], s = 0;
      center(c, x);
      for (int d = 0; d < dim; ++d) s += (x[d] - ctr[d]) * (x[d] - ctr[d]);
      const double dist = std::sqrt(s);
      if (dist > r && dist < R) fl.push_back(c);
    }
    T.refine_flagged(fl);
  };
  const double origin[3] = {0, 0, 0};
  double offset[3] = {0, 0, 0};
  for (int d = 0; d < dim; ++d) offset[d] = -0.1 * (d + 1);
  annulus(0.55 - reduction, 0.0, origin);
  annulus(0.42 - reduction, 0.3 + reduction, origin);
  annulus(0.41 - reduction, 0.32 + reduction, origin);
  annulus(0.33 - reduction, 0.17 + reduction, offset);
  annulus(0.31 - reduction, 0.21 + reduction, offset);
  if (dim == 2) {
    for (int s = 0; s < 4; ++s) {  // mark_cells_on_shell (bmop_common.h:27-47,98-104)
      std::vector<Cell> fl;
      for (const Cell &c : T.leaves()) {
        const double h = 2.0 / (double)(1u << c.level);
        int inside = 0;
        for (int v = 0; v < 4; ++v) {
          double s2 = 0;
          for (int d = 0; d < 2; ++d) {
            const double x = -1.0 + h * (c.c[d] + ((v >> d) & 1)) - offset[d];
            s2 += x * x;
          }
          inside += std::sqrt(s2) < 0.25;
        }
        if (inside != 0 && inside != 4) fl.push_back(c);
      }
      T.refine_flagged(fl);
    }
  }
  std::vector<std::array<uint32_t, 4>> v;
  for (const Cell &c : T.leaves()) v.push_back({(uint32_t)c.level, c.c[0], c.c[1], c.c[2]});
  (void)n;
  (void)nd;
  return build_from_tree_leaves(M, dim, v);
}

// Builds every array of the mesh from a one-irregular set of leaves (level, cx, cy, cz).
int build_from_tree_leaves(Mesh &M, int dim, std::vector<std::array<uint32_t, 4>> leaves_in) {
  const int p = M.degree, n = p + 1, nd = ipow(n, dim);
  if (M.nodes.empty()) M.init_tables();
  Tree T;
  T.dim = dim;
  for (auto &l : leaves_in) {
    uint32_t c[3] = {l[1], l[2], l[3]};
    T.active.insert(ckey((int)l[0], c));
    T.max_level = std::max(T.max_level, (int)l[0]);
  }
  // Morton (depth-first) order: consecutive cells are close in space, which is what the batch
  // planner's locality relies on (deal.II orders children of a cell consecutively as well)
  std::vector<Cell> cells = T.leaves();
  const int L = T.max_level;
  auto morton = [&](const Cell &c) {
    uint64_t m = 0;
    for (int b = L - 1; b >= 0; --b)
      for (int d = dim - 1; d >= 0; --d) {
        const uint32_t cc = c.c[d] << (L - c.level);
        m = (m << 1) | ((cc >> b) & 1);
      }
    return m;
  };
  std::sort(cells.begin(), cells.end(), [&](const Cell &a, const Cell &b) {
    const uint64_t ma = morton(a), mb = morton(b);
    return ma != mb ? ma < mb : a.level < b.level;
  });
  const uint32_t nc = (uint32_t)cells.size();
  std::unordered_map<uint64_t, uint32_t> cell_id;
  for (uint32_t i = 0; i < nc; ++i) cell_id[ckey(cells[i].level, cells[i].c)] = i;

  // ---- dofs (structural keys) and unsubstituted loc2glob
  std::unordered_map<DofKey, uint32_t, DofKeyHash> dof_id;
  std::vector<uint32_t> l2g((size_t)nc * nd);
  std::vector<double> coords;
  std::vector<uint8_t> on_boundary;
  for (uint32_t ci = 0; ci < nc; ++ci) {
    const Cell &c = cells[ci];
    const double h = 2.0 / (double)(1u << c.level);
    for (int i = 0; i < nd; ++i) {
      int idx[3] = {i % n, (i / n) % n, dim == 3 ? i / (n * n) : 0};
      DofKey key = dof_key(dim, p, c, idx);
      auto it = dof_id.find(key);
      uint32_t g;
      if (it == dof_id.end()) {
        g = (uint32_t)dof_id.size();
        dof_id.emplace(key, g);
        bool onb = false;
        for (int d = 0; d < dim; ++d) {
          const double x = -1.0 + h * (c.c[d] + M.nodes[idx[d]]);
          coords.push_back(x);
          const uint32_t last = (1u << c.level) - 1;
          if ((idx[d] == 0 && c.c[d] == 0) || (idx[d] == p && c.c[d] == last)) onb = true;
        }
        on_boundary.push_back(onb);
      } else {
        g = it->second;
      }
      l2g[(size_t)ci * nd + i] = g;
    }
  }
  const uint32_t N = (uint32_t)dof_id.size();

  // ---- hanging-node constraints per cell (HangingNodes::setup_constraints)
  const uint32_t TYPE[3] = {1u << 0, 1u << 1, 1u << 2};
  const uint32_t FACE[3] = {1u << 3, 1u << 4, 1u << 5};
  // edge along direction e: perpendicular directions (e+1)%3, (e+2)%3; mask bit as the kernel's
  // interpolate_boundary_3d expects it for interpolation direction e (hanging_nodes.cuh:636-637)
  const uint32_t EDGE_DIR[3] = {1u << 7 /*YZ: along x*/, 1u << 8 /*ZX: along y*/, 1u << 6 /*XY: along z*/};
  std::vector<uint32_t> sub(l2g);  // substituted loc2glob
  std::vector<uint32_t> mask(nc, 0);
  std::vector<uint8_t> hanging(N, 0);
  bool any_mask = false;
  auto find_cell = [&](int level, const int64_t *ci, const Cell *&out) -> bool {
    uint32_t c[3] = {0, 0, 0};
    for (int d = 0; d < dim; ++d) c[d] = (uint32_t)ci[d];
    auto it = cell_id.find(ckey(level, c));
    if (it == cell_id.end()) return false;
    out = &cells[it->second];
    return true;
  };
  for (uint32_t ci = 0; ci < nc; ++ci) {
    const Cell &c = cells[ci];
    if (c.level == 0) continue;
    uint32_t m = 0;
    bool face_con[3] = {false, false, false};
    // faces
    for (int d = 0; d < dim; ++d)
      for (int side = 0; side < 2; ++side) {
        int64_t nbc[3] = {c.c[0], c.c[1], c.c[2]};
        nbc[d] += side ? 1 : -1;
        const int lv = T.covering_level(c.level, nbc);
        if (lv < 0 || lv >= c.level) continue;  // boundary, same level or finer
        // coarse neighbour (exactly one level coarser in a one-irregular mesh)
        int64_t pc[3] = {nbc[0] >> 1, nbc[1] >> 1, nbc[2] >> 1};
        const Cell *nb = nullptr;
        if (lv != c.level - 1 || !find_cell(lv, pc, nb)) {
          set_error("internal: mesh is not one-irregular over faces");
          return MFGPU_EINVAL;
        }
        const uint32_t nbi = cell_id[ckey(nb->level, nb->c)];
        face_con[d] = true;
        m |= FACE[d];
        if (side == 0) m |= TYPE[d];  // constrained face is the low one (hanging_nodes.cuh:307-308)
        // tangential type bits: set when this cell is the first child along that direction
        // (subface index parity, :309-312,319-322,329-332)
        for (int t = 0; t < dim; ++t)
          if (t != d && (c.c[t] % 2 == 0)) m |= TYPE[t];
        // copy the coarse neighbour's dofs of the opposite face onto this face's entries (:336-353)
        const int fi = side ? p : 0;      // this cell's face index along d
        const int nfi = side ? 0 : p;     // neighbour's opposite face
        for (int a = 0; a < n; ++a)
          for (int b2 = 0; b2 < (dim == 3 ? n : 1); ++b2) {
            int idx[3], nidx[3];
            int t1 = (d + 1) % dim, t2 = dim == 3 ? (d + 2) % 3 : -1;
            if (dim == 2) t1 = 1 - d;
            idx[d] = fi;
            nidx[d] = nfi;
            idx[t1] = nidx[t1] = a;
            if (dim == 3) idx[t2] = nidx[t2] = b2;
            const int li = idx[0] + n * idx[1] + (dim == 3 ? n * n * idx[2] : 0);
            const int ni = nidx[0] + n * nidx[1] + (dim == 3 ? n * n * nidx[2] : 0);
            const uint32_t oldg = l2g[(size_t)ci * nd + li];
            const uint32_t newg = l2g[(size_t)nbi * nd + ni];
            sub[(size_t)ci * nd + li] = newg;
            if (oldg != newg) hanging[oldg] = 1;
          }
      }
    // edges (3D): an edge none of whose two faces is constrained, with a coarser cell diagonally
    // across it (:364-453)
    if (dim == 3)
      for (int e = 0; e < 3; ++e) {
        const int d1 = (e + 1) % 3, d2 = (e + 2) % 3;
        if (face_con[d1] || face_con[d2]) {
          // edges on a constrained face are covered by the face; the remaining edges of this cell
          // along e lie on the two unconstrained faces and are checked below
        }
        for (int s1 = 0; s1 < 2; ++s1)
          for (int s2 = 0; s2 < 2; ++s2) {
            // the edge belongs to face d1 (side s1) and face d2 (side s2) of this cell
            const bool f1 = (m & FACE[d1]) && (((m & TYPE[d1]) != 0) == (s1 == 0));
            const bool f2 = (m & FACE[d2]) && (((m & TYPE[d2]) != 0) == (s2 == 0));
            if (f1 || f2) continue;
            int64_t nbc[3] = {c.c[0], c.c[1], c.c[2]};
            nbc[d1] += s1 ? 1 : -1;
            nbc[d2] += s2 ? 1 : -1;
            const int lv = T.covering_level(c.level, nbc);
            if (lv < 0 || lv >= c.level) continue;
            int64_t pc[3] = {nbc[0] >> 1, nbc[1] >> 1, nbc[2] >> 1};
            const Cell *nb = nullptr;
            if (lv != c.level - 1 || !find_cell(lv, pc, nb)) {
              set_error("internal: mesh is not one-irregular over edges");
              return MFGPU_EINVAL;
            }
            const uint32_t nbi = cell_id[ckey(nb->level, nb->c)];
            m |= EDGE_DIR[e];
            if (s1 == 0) m |= TYPE[d1];
            if (s2 == 0) m |= TYPE[d2];
            if (c.c[e] % 2 == 0) m |= TYPE[e];  // first child along the edge
            for (int a = 0; a < n; ++a) {
              int idx[3], nidx[3];
              idx[e] = nidx[e] = a;
              idx[d1] = s1 ? p : 0;
              idx[d2] = s2 ? p : 0;
              nidx[d1] = s1 ? 0 : p;  // the coarse cell's edge facing this cell
              nidx[d2] = s2 ? 0 : p;
              const int li = idx[0] + n * idx[1] + n * n * idx[2];
              const int ni = nidx[0] + n * nidx[1] + n * n * nidx[2];
              const uint32_t oldg = l2g[(size_t)ci * nd + li];
              const uint32_t newg = l2g[(size_t)nbi * nd + ni];
              sub[(size_t)ci * nd + li] = newg;
              if (oldg != newg) hanging[oldg] = 1;
            }
          }
      }
    mask[ci] = m;
    any_mask = any_mask || m != 0;
  }

  // ---- fill the mesh
  M.n_cells = nc;
  M.n_dofs = N;
  M.loc2glob = sub;
  M.constraint_mask.clear();
  if (any_mask) M.constraint_mask = mask;
  M.dof_coords = coords;
  M.constrained.clear();
  for (uint32_t g = 0; g < N; ++g)
    if (on_boundary[g] || hanging[g]) M.constrained.push_back(g);  // Dirichlet AND hanging (bmop.cu:118-124)
  M.JxW.resize((size_t)nc * nd);
  M.inv_jac.resize(nc);
  M.qpoints.resize((size_t)nc * nd * dim);
  for (uint32_t ci = 0; ci < nc; ++ci) {
    const Cell &c = cells[ci];
    const double h = 2.0 / (double)(1u << c.level);
    M.inv_jac[ci] = 1.0 / h;
    for (int q = 0; q < nd; ++q) {
      int qq = q;
      double w = 1.0;
      for (int d = 0; d < dim; ++d) {
        const int qi = qq % n;
        qq /= n;
        w *= M.wq[qi] * h;
        M.qpoints[((size_t)ci * nd + q) * dim + d] = -1.0 + h * (c.c[d] + M.xq[qi]);
      }
      M.JxW[(size_t)ci * nd + q] = w;
    }
  }
  M.cell_levels.resize((size_t)nc * 4);
  for (uint32_t ci = 0; ci < nc; ++ci) {
    M.cell_levels[4 * ci] = (uint32_t)cells[ci].level;
    for (int d = 0; d < 3; ++d) M.cell_levels[4 * ci + 1 + d] = cells[ci].c[d];
  }
  M.iface[0].clear();
  M.iface[1].clear();
  M.finalize_typed();
  return 0;
}

}  // namespace mfgpu

extern "C" {

int mfgpu_mesh_create_adaptive(int dim, int degree, int n_ref, int number_type, mfgpu_mesh **out) {
  if (!out || (dim != 2 && dim != 3) || degree < 1 || degree > 6 ||
      (number_type != MFGPU_F64 && number_type != MFGPU_F32)) {
    mfgpu::set_error("mfgpu_mesh_create_adaptive: bad argument");
    return MFGPU_EINVAL;
  }
  mfgpu_mesh *m = new mfgpu_mesh();
  m->mesh.dim = dim;
  m->mesh.degree = degree;
  m->mesh.number_type = number_type;
  int rc = mfgpu::build_adaptive(m->mesh, n_ref, false);
  if (rc) {
    delete m;
    return rc;
  }
  *out = m;
  return 0;
}

int mfgpu_mesh_create_adaptive_mg(int dim, int degree, int n_ref, int number_type, mfgpu_mesh **out) {
  if (!out || (dim != 2 && dim != 3) || degree < 1 || degree > 6 ||
      (number_type != MFGPU_F64 && number_type != MFGPU_F32)) {
    mfgpu::set_error("mfgpu_mesh_create_adaptive_mg: bad argument");
    return MFGPU_EINVAL;
  }
  mfgpu_mesh *m = new mfgpu_mesh();
  m->mesh.dim = dim;
  m->mesh.degree = degree;
  m->mesh.number_type = number_type;
  int rc = mfgpu::build_adaptive(m->mesh, n_ref, true);
  if (rc) {
    delete m;
    return rc;
  }
  *out = m;
  return 0;
}

int mfgpu_mesh_create_from_leaves(int dim, int degree, const uint32_t *leaves, uint32_t n_leaves,
                                  int number_type, mfgpu_mesh **out) {
  if (!out || !leaves || n_leaves == 0 || (dim != 2 && dim != 3) || degree < 1 || degree > 6) {
    mfgpu::set_error("mfgpu_mesh_create_from_leaves: bad argument");
    return MFGPU_EINVAL;
  }
  mfgpu_mesh *m = new mfgpu_mesh();
  m->mesh.dim = dim;
  m->mesh.degree = degree;
  m->mesh.number_type = number_type;
  std::vector<std::array<uint32_t, 4>> v(n_leaves);
  for (uint32_t i = 0; i < n_leaves; ++i) v[i] = {leaves[4 * i], leaves[4 * i + 1], leaves[4 * i + 2], leaves[4 * i + 3]};
  int rc = mfgpu::build_from_tree_leaves(m->mesh, dim, v);
  if (rc) {
    delete m;
    return rc;
  }
  *out = m;
  return 0;
}

// the offsets to the neighbours of a cell over faces and, in 3D, edges; with `vertices` over vertices too
static std::vector<std::array<int, 3>> neighbour_offsets(int dim, bool vertices) {
  std::vector<std::array<int, 3>> offsets;
  for (int ox = -1; ox <= 1; ++ox)
    for (int oy = -1; oy <= 1; ++oy)
      for (int oz = (dim == 3 ? -1 : 0); oz <= (dim == 3 ? 1 : 0); ++oz) {
        const int nz = (ox != 0) + (oy != 0) + (oz != 0);
        if (nz != 0 && (nz < dim || vertices)) offsets.push_back({ox, oy, oz});
      }
  return offsets;
}

// one-irregular: no leaf touches a leaf two or more levels coarser over one of the offsets
static bool one_irregular(const mfgpu::Tree &T, const uint32_t *leaves, uint32_t n_leaves,
                          const std::vector<std::array<int, 3>> &offsets) {
  for (uint32_t i = 0; i < n_leaves; ++i) {
    const uint32_t *l = leaves + 4 * (size_t)i;
    for (const auto &o : offsets) {
      const int64_t ci[3] = {(int64_t)l[1] + o[0], (int64_t)l[2] + o[1], (int64_t)l[3] + o[2]};
      const int lv = T.covering_level((int)l[0], ci);
      if (lv >= 0 && lv < (int)l[0] - 1) return false;
    }
  }
  return true;
}

// the cell of a ckey
static mfgpu::Cell cell_of(uint64_t k) {
  mfgpu::Cell c;
  c.level = (int)(k >> 57);
  c.c[0] = (uint32_t)(k & 0x7ffff);
  c.c[1] = (uint32_t)((k >> 19) & 0x7ffff);
  c.c[2] = (uint32_t)((k >> 38) & 0x7ffff);
  return c;
}

// does the leaf P of T touch a leaf two or more levels finer over one of the offsets?  (The rollback of
// mfgpu_mesh_coarsen_leaves and mfgpu_mesh_adapt_leaves: a new parent that does is split again.)
static bool touched_by_two_finer(const mfgpu::Tree &T, int dim, const mfgpu::Cell &P,
                                 const std::vector<std::array<int, 3>> &offsets) {
  for (const auto &o : offsets) {
    int64_t nb[3] = {(int64_t)P.c[0] + o[0], (int64_t)P.c[1] + o[1], (int64_t)P.c[2] + o[2]};
    if (T.covering_level(P.level, nb) != -1) continue;  // outside, or covered by a leaf of P's level or coarser
    // the neighbour's children at the shared face / edge / vertex: refined themselves?
    for (int k = 0; k < (1 << dim); ++k) {
      int64_t ch[3] = {0, 0, 0};
      bool at = true;
      for (int d = 0; d < dim; ++d) {
        const int b = (k >> d) & 1;
        if ((o[d] == 1 && b != 0) || (o[d] == -1 && b != 1)) at = false;
        ch[d] = 2 * nb[d] + b;
      }
      if (at && T.covering_level(P.level + 1, ch) == -1) return true;
    }
  }
  return false;
}

// replaces the families of `parents` in T by their parents; then, until nothing changes, splits every parent again that
// a leaf two or more levels finer touches.  A rollback only makes the set finer, so it can only force further rollbacks:
// the fixed point does not depend on the order.  `parents` keeps the survivors
static void coarsen_families(mfgpu::Tree &T, int dim, std::vector<mfgpu::Cell> &parents,
                             const std::vector<std::array<int, 3>> &offsets) {
  using namespace mfgpu;
  for (const Cell &P : parents) {
    for (int k = 0; k < (1 << dim); ++k) {
      uint32_t c[3] = {0, 0, 0};
      for (int d = 0; d < dim; ++d) c[d] = 2 * P.c[d] + ((k >> d) & 1);
      T.active.erase(ckey(P.level + 1, c));
    }
    T.active.insert(ckey(P.level, P.c));
  }
  for (bool changed = true; changed;) {
    changed = false;
    std::vector<Cell> kept;
    for (const Cell &P : parents) {
      if (touched_by_two_finer(T, dim, P, offsets)) {
        T.refine(P);  // back to its children
        changed = true;
      } else {
        kept.push_back(P);
      }
    }
    parents.swap(kept);
  }
}

// The checks mfgpu_mesh_coarsen_leaves and mfgpu_mesh_refine_leaves share: the leaves (level, cx, cy, cz) lie in the root
// cell, none deeper than level 18 or listed twice, they partition the root cell, and they are one-irregular over faces and,
// in 3D, edges.  Fills T with them.
static int load_leaves(const char *who, int dim, const uint32_t *leaves, uint32_t n_leaves, mfgpu::Tree &T) {
  using namespace mfgpu;
  T.dim = dim;
  const int kMaxLevel = 18;  // ckey's 19 bits per coordinate; dim * level < 64 for the volume sum
  for (uint32_t i = 0; i < n_leaves; ++i) {
    const uint32_t *l = leaves + 4 * (size_t)i;
    bool ok = l[0] <= (uint32_t)kMaxLevel;
    for (int d = 0; d < 3 && ok; ++d) ok = d < dim ? l[1 + d] < (1u << l[0]) : l[1 + d] == 0;
    if (!ok || !T.active.insert(ckey((int)l[0], l + 1)).second) {
      set_error(std::string(who) + ": a leaf outside the root cell, deeper than level 18, or listed twice");
      return MFGPU_EINVAL;
    }
    T.max_level = std::max(T.max_level, (int)l[0]);
  }
  // a partition of the root: no leaf inside another, and the volumes add up
  uint64_t volume = 0;
  for (uint32_t i = 0; i < n_leaves; ++i) {
    const uint32_t *l = leaves + 4 * (size_t)i;
    volume += (uint64_t)1 << (dim * (T.max_level - (int)l[0]));
    uint32_t c[3] = {l[1], l[2], l[3]};
    for (int ll = (int)l[0] - 1; ll >= 0; --ll) {
      for (int d = 0; d < dim; ++d) c[d] >>= 1;
      if (T.is_active(ll, c)) {
        set_error(std::string(who) + ": the leaves are not a partition (one lies inside another)");
        return MFGPU_EINVAL;
      }
    }
  }
  if (volume != (uint64_t)1 << (dim * T.max_level)) {
    set_error(std::string(who) + ": the leaves are not a partition (they do not cover the root cell)");
    return MFGPU_EINVAL;
  }
  if (!one_irregular(T, leaves, n_leaves, neighbour_offsets(dim, false))) {
    set_error(std::string(who) + ": the leaves are not one-irregular over faces and edges");
    return MFGPU_EINVAL;
  }
  return 0;
}

// One step of global coarsening.  Every complete family of sibling leaves is replaced by its
// parent; then, until nothing changes, a new parent is split again where it breaks one-irregularity: where a cell of its
// own level next to it over a face (3D: or an edge) has a child at the shared face / edge that is itself refined, so a
// leaf two or more levels finer than the parent touches it.  A rollback only makes the set finer, so it can only force
// further rollbacks: the fixed point does not depend on the order.
int64_t mfgpu_mesh_coarsen_leaves(int dim, const uint32_t *leaves, uint32_t n_leaves, uint32_t *out) {
  using namespace mfgpu;
  const char *who = "mfgpu_mesh_coarsen_leaves";
  if ((dim != 2 && dim != 3) || !leaves || !out || n_leaves == 0) {
    set_error(std::string(who) + ": bad argument (dim 2 or 3, arrays, at least one leaf)");
    return MFGPU_EINVAL;
  }
  Tree T;
  if (const int rc = load_leaves(who, dim, leaves, n_leaves, T)) return rc;
  const std::vector<std::array<int, 3>> offsets = neighbour_offsets(dim, false);
  if (T.max_level == 0) {
    set_error(std::string(who) + ": the single root cell cannot be coarsened");
    return MFGPU_EINVAL;
  }
  // the complete families
  std::unordered_map<uint64_t, int> n_children;
  for (uint32_t i = 0; i < n_leaves; ++i) {
    const uint32_t *l = leaves + 4 * (size_t)i;
    if (l[0] == 0) continue;
    const uint32_t pc[3] = {l[1] >> 1, l[2] >> 1, l[3] >> 1};
    ++n_children[ckey((int)l[0] - 1, pc)];
  }
  std::vector<Cell> parents;
  for (const auto &kv : n_children)
    if (kv.second == (1 << dim)) parents.push_back(cell_of(kv.first));
  coarsen_families(T, dim, parents, offsets);
  std::vector<uint64_t> keys(T.active.begin(), T.active.end());
  std::sort(keys.begin(), keys.end());
  for (size_t i = 0; i < keys.size(); ++i) {
    const Cell c = cell_of(keys[i]);
    out[4 * i] = (uint32_t)c.level;
    for (int d = 0; d < 3; ++d) out[4 * i + 1 + d] = c.c[d];
  }
  return (int64_t)keys.size();
}

// One step of refinement: the flagged leaves and, to stay one-irregular, every leaf that a split
// leaf of higher level touches (Tree::refine_flagged: over faces and 3D edges, with balance_vertices over vertices too)
// are replaced by their children.  The closure only ever reaches leaves coarser than the one that forces them, and the
// input is one-irregular in the relation of the closure (with balance_vertices that is checked here: over vertices too),
// so no child splits: whatever is no longer a leaf afterwards was an input leaf.
int64_t mfgpu_mesh_refine_leaves(int dim, const uint32_t *leaves, uint32_t n_leaves, const uint8_t *flags,
                                 uint32_t balance_vertices, uint32_t *out, uint64_t out_capacity) {
  using namespace mfgpu;
  const char *who = "mfgpu_mesh_refine_leaves";
  if ((dim != 2 && dim != 3) || !leaves || !flags || !out || n_leaves == 0) {
    set_error(std::string(who) + ": bad argument (dim 2 or 3, arrays, at least one leaf)");
    return MFGPU_EINVAL;
  }
  Tree T;
  if (const int rc = load_leaves(who, dim, leaves, n_leaves, T)) return rc;
  T.balance_vertices = balance_vertices != 0;
  // the closure starts at split leaves only: an input that is not balanced over vertices would stay unbalanced where
  // nothing splits, and could force a child to split where something does
  if (T.balance_vertices && !one_irregular(T, leaves, n_leaves, neighbour_offsets(dim, true))) {
    set_error(std::string(who) + ": balance_vertices needs leaves that are one-irregular over vertices too");
    return MFGPU_EINVAL;
  }
  std::vector<Cell> flagged;
  for (uint32_t i = 0; i < n_leaves; ++i) {
    if (!flags[i]) continue;
    const uint32_t *l = leaves + 4 * (size_t)i;
    if (l[0] >= 18) {
      set_error(std::string(who) + ": a child of a flagged leaf would be deeper than level 18");
      return MFGPU_EINVAL;
    }
    flagged.push_back(Cell{(int)l[0], {l[1], l[2], l[3]}});
  }
  T.refine_flagged(flagged);
  uint64_t n_out = 0;
  for (uint32_t i = 0; i < n_leaves; ++i) {
    const uint32_t *l = leaves + 4 * (size_t)i;
    n_out += T.is_active((int)l[0], l + 1) ? 1 : (1u << dim);
  }
  if (n_out > out_capacity) {
    set_error(std::string(who) + ": out_capacity " + std::to_string(out_capacity) + " is too small, the refined set has " +
              std::to_string(n_out) + " leaves");
    return MFGPU_EINVAL;
  }
  uint32_t *o = out;
  for (uint32_t i = 0; i < n_leaves; ++i) {
    const uint32_t *l = leaves + 4 * (size_t)i;
    if (T.is_active((int)l[0], l + 1)) {
      for (int j = 0; j < 4; ++j) *o++ = l[j];
      continue;
    }
    for (uint32_t k = 0; k < (1u << dim); ++k) {
      *o++ = l[0] + 1;
      for (int d = 0; d < 3; ++d) *o++ = d < dim ? 2 * l[1 + d] + ((k >> d) & 1u) : 0u;
    }
  }
  return (int64_t)n_out;
}

// Refinement and coarsening in one step.  R is what mfgpu_mesh_refine_leaves makes of the refine
// flags.  A family is a candidate when its 2^dim children are input leaves, all with a coarsen flag, none with a refine
// flag, and all still leaves of R (refinement wins).  The candidates become their parents; then mfgpu_mesh_coarsen_leaves'
// rollback runs in the relation of the closure, until no surviving parent is touched by a leaf two or more levels finer.
// A rollback only makes the set finer, so the fixed point does not depend on the order.  `new` is the result, `mid` the
// input with exactly the surviving families replaced: a surviving parent P of level l is touched by no leaf deeper than
// l + 1 in `new`, and an input leaf of level l + 2 next to it is in `new` itself, split, or coarsened with its own
// surviving family, which `mid` holds too -- so `mid` is one-irregular as well.
int64_t mfgpu_mesh_adapt_leaves(int dim, const uint32_t *leaves, uint32_t n_leaves, const uint8_t *refine_flags,
                                const uint8_t *coarsen_flags, uint32_t balance_vertices, uint32_t *out_new,
                                uint64_t new_capacity, uint32_t *out_mid, uint32_t *n_mid) {
  using namespace mfgpu;
  const char *who = "mfgpu_mesh_adapt_leaves";
  if ((dim != 2 && dim != 3) || !leaves || !refine_flags || !coarsen_flags || !out_new || !out_mid || !n_mid ||
      n_leaves == 0) {
    set_error(std::string(who) + ": bad argument (dim 2 or 3, arrays, at least one leaf)");
    return MFGPU_EINVAL;
  }
  Tree T;
  if (const int rc = load_leaves(who, dim, leaves, n_leaves, T)) return rc;
  T.balance_vertices = balance_vertices != 0;
  const std::vector<std::array<int, 3>> offsets = neighbour_offsets(dim, T.balance_vertices);
  if (T.balance_vertices && !one_irregular(T, leaves, n_leaves, offsets)) {
    set_error(std::string(who) + ": balance_vertices needs leaves that are one-irregular over vertices too");
    return MFGPU_EINVAL;
  }
  std::vector<Cell> flagged;
  for (uint32_t i = 0; i < n_leaves; ++i) {
    if (!refine_flags[i]) continue;
    const uint32_t *l = leaves + 4 * (size_t)i;
    if (l[0] >= 18) {
      set_error(std::string(who) + ": a child of a flagged leaf would be deeper than level 18");
      return MFGPU_EINVAL;
    }
    flagged.push_back(Cell{(int)l[0], {l[1], l[2], l[3]}});
  }
  T.refine_flagged(flagged);  // T holds R
  // the candidate families, by their parents
  auto parent_key = [](const uint32_t *l) {
    const uint32_t pc[3] = {l[1] >> 1, l[2] >> 1, l[3] >> 1};
    return ckey((int)l[0] - 1, pc);
  };
  std::unordered_map<uint64_t, int> n_willing;
  for (uint32_t i = 0; i < n_leaves; ++i) {
    const uint32_t *l = leaves + 4 * (size_t)i;
    if (l[0] == 0 || !coarsen_flags[i] || refine_flags[i] || !T.is_active((int)l[0], l + 1)) continue;
    ++n_willing[parent_key(l)];
  }
  std::vector<Cell> parents;
  for (const auto &kv : n_willing)
    if (kv.second == (1 << dim)) parents.push_back(cell_of(kv.first));
  coarsen_families(T, dim, parents, offsets);  // the rollback of mfgpu_mesh_coarsen_leaves, over the offsets of this call
  std::unordered_set<uint64_t> survivors;
  for (const Cell &P : parents) survivors.insert(ckey(P.level, P.c));
  // 0: the leaf stays or splits; 1: child 0 of a surviving family; 2: another child of one
  auto role = [&](const uint32_t *l) {
    if (l[0] == 0 || !survivors.count(parent_key(l))) return 0;
    return ((l[1] | l[2] | l[3]) & 1u) ? 2 : 1;
  };
  uint64_t n_new = 0;
  for (uint32_t i = 0; i < n_leaves; ++i) {
    const uint32_t *l = leaves + 4 * (size_t)i;
    const int r = role(l);
    n_new += r ? (r == 1 ? 1 : 0) : T.is_active((int)l[0], l + 1) ? 1 : (1u << dim);
  }
  if (n_new > new_capacity) {
    set_error(std::string(who) + ": new_capacity " + std::to_string(new_capacity) + " is too small, the adapted set has " +
              std::to_string(n_new) + " leaves");
    return MFGPU_EINVAL;
  }
  uint32_t *o = out_new, *m = out_mid;
  for (uint32_t i = 0; i < n_leaves; ++i) {
    const uint32_t *l = leaves + 4 * (size_t)i;
    const int r = role(l);
    if (r == 2) continue;
    if (r == 1) {
      for (uint32_t *dst : {o, m}) {
        dst[0] = l[0] - 1;
        for (int d = 0; d < 3; ++d) dst[1 + d] = l[1 + d] >> 1;
      }
      o += 4;
      m += 4;
      continue;
    }
    for (int j = 0; j < 4; ++j) *m++ = l[j];
    if (T.is_active((int)l[0], l + 1)) {
      for (int j = 0; j < 4; ++j) *o++ = l[j];
      continue;
    }
    for (uint32_t k = 0; k < (1u << dim); ++k) {
      *o++ = l[0] + 1;
      for (int d = 0; d < 3; ++d) *o++ = d < dim ? 2 * l[1 + d] + ((k >> d) & 1u) : 0u;
    }
  }
  *n_mid = (uint32_t)((m - out_mid) / 4);
  return (int64_t)n_new;
}

int mfgpu_mesh_coarsening_map(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, uint32_t *parent, uint32_t *child) {
  using namespace mfgpu;
  const char *who = "mfgpu_mesh_coarsening_map";
  if (!coarse || !fine || !parent || !child) {
    set_error(std::string(who) + ": null argument");
    return MFGPU_EINVAL;
  }
  const Mesh &C = coarse->mesh, &F = fine->mesh;
  if (C.dim != F.dim || C.cell_levels.size() != 4 * (size_t)C.n_cells || F.cell_levels.size() != 4 * (size_t)F.n_cells ||
      C.n_cells == 0 || F.n_cells == 0) {
    set_error(std::string(who) + ": needs two leaf meshes (adaptive, from leaves) of one dimension");
    return MFGPU_EINVAL;
  }
  std::unordered_map<uint64_t, uint32_t> id;
  for (uint32_t c = 0; c < C.n_cells; ++c) id[ckey((int)C.cell_levels[4 * c], &C.cell_levels[4 * c + 1])] = c;
  for (uint32_t f = 0; f < F.n_cells; ++f) {
    const uint32_t *l = &F.cell_levels[4 * (size_t)f];
    auto it = id.find(ckey((int)l[0], l + 1));
    if (it != id.end()) {
      parent[f] = it->second;
      child[f] = 0;
      continue;
    }
    const uint32_t pc[3] = {l[1] >> 1, l[2] >> 1, l[3] >> 1};
    if (l[0] == 0 || (it = id.find(ckey((int)l[0] - 1, pc))) == id.end()) {
      set_error(std::string(who) + ": a fine leaf is neither a coarse leaf nor the child of one");
      return MFGPU_EINVAL;
    }
    parent[f] = it->second;
    child[f] = 1 + ((l[1] & 1u) | ((l[2] & 1u) << 1) | ((l[3] & 1u) << 2));
  }
  return 0;
}

int64_t mfgpu_mesh_cell_levels(const mfgpu_mesh *m, const uint32_t **ptr) {
  if (!m || !ptr) return MFGPU_EINVAL;
  *ptr = m->mesh.cell_levels.data();
  return (int64_t)m->mesh.cell_levels.size();
}

}  // extern "C"
