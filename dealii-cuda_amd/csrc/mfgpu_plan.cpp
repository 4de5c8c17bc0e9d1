// Host-side planner: groups cells into batches (one workgroup each), colours the batches,
// and decides for every (batch, dof) whether the batch stores (first toucher) or adds.
//
// Replaces, MI355X-first, the reference's per-CELL graph colouring (coloring.cc:8-33,
// matrix_free_gpu.cu:157-186): a batch sums every dof shared by its own cells in LDS, so
// only dofs on batch surfaces are read-modify-written in global memory, and the first
// toucher of a dof stores instead of adding, which removes the separate `dst = 0` pass
// (laplace_operator_gpu.h:221) and the save/load constrained-row kernels
// (constraint_handler_gpu.cu:247-289) from the hot loop.
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstring>
#include <numeric>
#include <unordered_map>

#include "mfgpu_internal.h"

namespace mfgpu {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
const char *last_error() { return g_err.c_str(); }

int derive_tables(int n, const double *sv, const double *sg, std::vector<double> &S,
                  std::vector<double> &Dt) {
  // Solve S * X = G for X = Dt^T (n x n), long double Gaussian elimination with pivoting.
  std::vector<long double> A(n * n), B(n * n);
  for (int i = 0; i < n * n; ++i) {
    A[i] = sv[i];
    B[i] = sg[i];
  }
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r)
      if (fabsl(A[r * n + c]) > fabsl(A[piv * n + c])) piv = r;
    if (fabsl(A[piv * n + c]) < 1e-30L) {
      set_error("shape_values table is singular");
      return MFGPU_EINVAL;
    }
    if (piv != c)
      for (int k = 0; k < n; ++k) {
        std::swap(A[c * n + k], A[piv * n + k]);
        std::swap(B[c * n + k], B[piv * n + k]);
      }
    for (int r = 0; r < n; ++r) {
      if (r == c) continue;
      long double f = A[r * n + c] / A[c * n + c];
      for (int k = 0; k < n; ++k) {
        A[r * n + k] -= f * A[c * n + k];
        B[r * n + k] -= f * B[c * n + k];
      }
    }
  }
  S.assign(sv, sv + n * n);
  Dt.resize(n * n);
  // X[t][q] = B[t][q]/A[t][t];  Dt[q*n+t] = X[t][q]
  for (int t = 0; t < n; ++t)
    for (int q = 0; q < n; ++q) Dt[q * n + t] = (double)(B[t * n + q] / A[t * n + t]);
  return 0;
}

static void default_batch_limits(const mfgpu_desc &d, uint32_t max_chunks, uint32_t &max_cells, uint32_t &max_dofs) {
  const int p = d.degree, dim = d.dim;
  max_dofs = d.max_dofs_per_batch ? d.max_dofs_per_batch : 2304u;
  // the kernel keeps a batch's dof list and source values in registers: kGU * kBlock = 9 * 256 dofs
  if (max_dofs > 2304u) max_dofs = 2304u;
  const uint32_t nd = (uint32_t)ipow(p + 1, dim);
  if (max_dofs < nd) max_dofs = nd;
  if (d.max_cells_per_batch) {
    max_cells = d.max_cells_per_batch;
  } else {
    // the largest near-cubic box of cells (edge lengths m or m + 1) whose dofs fit: 3x3x3 at p=4, 4x4x4 at
    // p=3, 3x2x2 at p=5 (the cube 2x2x2 would leave the dof budget half empty); at low degree the chunk
    // limit below is the binding one
    int m = 1;
    while ((uint64_t)ipow((m + 1) * p + 1, dim) <= max_dofs) ++m;
    uint64_t best = (uint64_t)ipow(m, dim);
    for (int k = 1; k < dim; ++k) {  // k edges of length m + 1, dim - k of length m
      const uint64_t dofs = (uint64_t)ipow((m + 1) * p + 1, k) * (uint64_t)ipow(m * p + 1, dim - k);
      if (dofs <= max_dofs) best = (uint64_t)ipow(m + 1, k) * (uint64_t)ipow(m, dim - k);
    }
    max_cells = (uint32_t)best;
    // keep enough workgroups per launch on small meshes
    const uint32_t cap = std::max<uint32_t>(1u, d.n_cells / 4096u);
    max_cells = std::min(max_cells, cap);
  }
  // the kernel unrolls at most max_chunks chunks of CH = threads / n^(dim-1) cells per batch
  const uint32_t threads = d.max_dofs_per_batch && d.max_dofs_per_batch <= 768 ? 64u : 256u;
  const uint32_t ch = std::max<uint32_t>(1u, threads / (uint32_t)ipow(p + 1, dim - 1));
  max_cells = std::min(max_cells, max_chunks * ch);
  if (max_cells < 1) max_cells = 1;
}

void hn_cell_lines(unsigned mask, int n, std::vector<HnLine> (&lines)[3], std::vector<uint16_t> &nodes) {
  const int p = n - 1;
  const unsigned TYPE[3] = {1u << 0, 1u << 1, 1u << 2}, FACE[3] = {1u << 3, 1u << 4, 1u << 5};
  const unsigned EDGE[3] = {1u << 7, 1u << 8, 1u << 6};  // direction x: edge YZ, y: ZX, z: XY (hanging_nodes.cuh:38-50)
  const int stride[3] = {1, n, n * n};
  std::vector<uint8_t> on(n * n * n, 0);
  for (int d = 0; d < 3; ++d) {
    lines[d].clear();
    const int d1 = (d + 1) % 3, d2 = (d + 2) % 3;
    if (!(mask & (FACE[d1] | FACE[d2] | EDGE[d]))) continue;
    const int i1 = (mask & TYPE[d1]) ? 0 : p, i2 = (mask & TYPE[d2]) ? 0 : p;
    const bool typ = (mask & TYPE[d]) != 0;
    for (int a = 0; a < n; ++a)
      for (int b = 0; b < n; ++b) {
        const bool flag = ((mask & FACE[d1]) && a == i1) || ((mask & FACE[d2]) && b == i2) ||
                          ((mask & EDGE[d]) && a == i1 && b == i2);
        if (!flag) continue;
        HnLine L{};
        for (int t = 0; t < n; ++t) {
          const int node = (typ ? t : p - t) * stride[d] + a * stride[d1] + b * stride[d2];
          L.node[t] = (uint16_t)node;
          on[node] = 1;
        }
        lines[d].push_back(L);
      }
  }
  nodes.clear();
  for (int i = 0; i < n * n * n; ++i)
    if (on[i]) nodes.push_back((uint16_t)i);
}

// ---- the stages of build_plan, in the order it runs them
namespace {
constexpr uint32_t NONE = 0xffffffffu;

// The checked description as the stages read it: nd dofs per cell, constrained[g] = 1 for the constrained dofs.
struct Description {
  const uint32_t *l2g = nullptr;
  uint32_t nc = 0, nd = 0, N = 0;
  int dim = 0, n = 0;
  std::vector<uint8_t> constrained;
  const uint32_t *dofs_of(uint32_t c) const { return l2g + (uint64_t)c * nd; }
  uint32_t flagged(uint32_t g) const { return g | (constrained[g] ? 0x80000000u : 0u); }  // bit 31: constrained row
};

int check_description(const mfgpu_desc &d, Description &m) {
  if (d.dim != 2 && d.dim != 3) {
    set_error("dim must be 2 or 3");
    return MFGPU_EINVAL;
  }
  if (d.degree < 1 || d.degree > 6) {
    set_error("degree must be in 1..6");
    return MFGPU_EUNSUPPORTED;
  }
  if (!d.loc2glob || d.n_cells == 0 || d.n_dofs == 0) {
    set_error("empty description (n_cells, n_dofs and loc2glob are required)");
    return MFGPU_EINVAL;
  }
  if (d.n_constrained && !d.constrained_dofs) {
    set_error("n_constrained > 0 but constrained_dofs is NULL");
    return MFGPU_EINVAL;
  }
  m.l2g = d.loc2glob;
  m.dim = d.dim;
  m.n = d.degree + 1;
  m.nd = (uint32_t)ipow(m.n, d.dim);
  m.nc = d.n_cells;
  m.N = d.n_dofs;
  for (uint64_t i = 0; i < (uint64_t)m.nc * m.nd; ++i)
    if (m.l2g[i] >= m.N) {
      set_error("loc2glob entry out of range");
      return MFGPU_EINVAL;
    }
  m.constrained.assign(m.N, 0);
  for (uint32_t i = 0; i < d.n_constrained; ++i) {
    if (d.constrained_dofs[i] >= m.N) {
      set_error("constrained_dofs entry out of range");
      return MFGPU_EINVAL;
    }
    m.constrained[d.constrained_dofs[i]] = 1;
  }
  if (m.N >= 0x80000000u) {
    set_error("n_dofs >= 2^31 is not supported (bit 31 of the dof lists carries the constrained flag)");
    return MFGPU_EUNSUPPORTED;
  }
  return 0;
}

// The batch rules, resolved once from the description, max_chunks and the kernel's PlanLimits.  A batch holds cells of
// one CLASS: masked (cells with a hanging-node mask, under `segregate` only) or not.
struct BatchLimits {
  uint32_t max_cells = 0, max_dofs = 0;
};
struct BatchRules {
  BatchLimits plane;   // the kernel-imposed limits (plane plans), else the default limits: every batch but ...
  BatchLimits pencil;  // ... those of segregated masked cells that run in the pencil kernel: its default limits
  bool segregate = false, masked_planes = false;
  const uint32_t *mask = nullptr;     // the description's constraint_mask (segregate only)
  std::vector<uint32_t> priv_of_mask;  // mask value (9 bits) -> private entries of such a cell (masked_planes only)
  // plane plans (0 otherwise; see PlanLimits)
  uint32_t interior_max = 0, shared_max = 0, halo_stride = 0, private_max = 0;

  bool masked(uint32_t c) const { return segregate && mask[c] != 0; }
  // THE rule: do the batches of this class (masked or not) run in the plane kernel?  (segregate comes with a plane
  // kernel's limits, so a class outside the plane kernel is the masked one under the pencil kernel's limits)
  bool in_planes(bool cls) const { return interior_max != 0 && (!cls || masked_planes); }
  const BatchLimits &limits_of(bool cls) const { return cls && !in_planes(cls) ? pencil : plane; }
  // private entries of the cell's constrained nodes (0 for every cell outside the masked plane batches)
  uint32_t priv_of(uint32_t c) const { return masked_planes ? priv_of_mask[mask[c]] : 0u; }
};

int resolve_batch_rules(const mfgpu_desc &d, uint32_t max_chunks, const PlanLimits *limits, BatchRules &R) {
  const int n = d.degree + 1;
  // limits->segregate_masked (meshes with hanging nodes under apply_planes3): cells WITHOUT a hanging-node mask are
  // batched under `limits` and run in the plane kernel, which has no constraint stages; cells with a mask get batches of
  // their own under the pencil kernel's default limits (R.pencil) and run in apply_batches_x<HN>.  The plane
  // batches come first in the execution order (P.n_plane_batches of them).
  R.segregate = limits && limits->segregate_masked && (d.flags & MFGPU_HANGING_NODES) && d.constraint_mask;
  if (R.segregate) {
    R.mask = d.constraint_mask;
    default_batch_limits(d, max_chunks, R.pencil.max_cells, R.pencil.max_dofs);
  }
  // masked cells in plane batches of their own (apply_planes3<HN>): the plane limits, plus the private entries of the
  // cells' constrained nodes (counted per mask value)
  R.masked_planes = R.segregate && limits->masked_planes && limits->max_cells && limits->max_dofs;
  if (R.masked_planes) {
    R.priv_of_mask.assign(512, 0u);
    std::vector<HnLine> ln[3];
    std::vector<uint16_t> nodes;
    for (unsigned m = 1; m < 512; ++m) {
      hn_cell_lines(m, n, ln, nodes);
      R.priv_of_mask[m] = (uint32_t)nodes.size();
    }
    for (uint32_t c = 0; c < d.n_cells; ++c)
      if (d.constraint_mask[c] >= 512) {
        set_error("constraint_mask has bits beyond the nine of hanging_nodes.cuh:38-50");
        return MFGPU_EINVAL;
      }
  }
  if (limits && limits->max_cells && limits->max_dofs) {
    // kernel-imposed limits; the caller's knobs may only tighten them
    R.plane.max_cells = d.max_cells_per_batch ? std::min(d.max_cells_per_batch, limits->max_cells) : limits->max_cells;
    R.plane.max_dofs = d.max_dofs_per_batch ? std::min(d.max_dofs_per_batch, limits->max_dofs) : limits->max_dofs;
    if (R.plane.max_dofs < (uint32_t)ipow(n, d.dim)) {
      set_error("max_dofs_per_batch is smaller than one cell");
      return MFGPU_EINVAL;
    }
  } else {
    default_batch_limits(d, max_chunks, R.plane.max_cells, R.plane.max_dofs);
  }
  if (limits) {
    R.interior_max = limits->interior_max;
    R.shared_max = limits->shared_max;
    R.halo_stride = limits->halo_stride;
    R.private_max = limits->private_max;
  }
  assert(!R.segregate || R.interior_max);  // (in_planes, limits_of: segregation comes with a plane kernel's limits)
  return 0;
}

// dof -> cells incidence (CSR)
struct Incidence {
  std::vector<uint32_t> off, cells;
  uint32_t count(uint32_t g) const { return off[g + 1] - off[g]; }
};

Incidence dof_cell_incidence(const Description &m) {
  Incidence inc;
  std::vector<uint32_t> &dc_off = inc.off, &dc = inc.cells;
  dc_off.assign(m.N + 1, 0);
  for (uint64_t i = 0; i < (uint64_t)m.nc * m.nd; ++i) dc_off[m.l2g[i] + 1]++;
  for (uint32_t g = 0; g < m.N; ++g) dc_off[g + 1] += dc_off[g];
  dc.resize(dc_off[m.N]);
  std::vector<uint32_t> pos(dc_off.begin(), dc_off.end() - 1);
  for (uint32_t c = 0; c < m.nc; ++c)
    for (uint32_t i = 0; i < m.nd; ++i) dc[pos[m.dofs_of(c)[i]]++] = c;
  // a cell that lists one dof twice (substituted / degenerate loc2glob) counts once: the cells of a dof are
  // in ascending order, so duplicates are adjacent
  uint32_t w = 0;
  for (uint32_t g = 0; g < m.N; ++g) {
    const uint32_t beg = dc_off[g], end = dc_off[g + 1];
    dc_off[g] = w;
    for (uint32_t k = beg; k < end; ++k)
      if (k == beg || dc[k] != dc[k - 1]) dc[w++] = dc[k];
  }
  dc_off[m.N] = w;
  dc.resize(w);
  return inc;
}

// Face neighbours by direction (plane plans, n >= 3): the cell across face (axis, side) is the other cell of a dof in
// the interior of that face, provided it lists the dof at the mirrored position (same size, same orientation; a
// hanging-node face, whose entries were substituted, has no neighbour in this sense).  They let a batch start as a
// box a x b x c: on a mesh whose extent is no multiple of the natural box (64 cells: 21 boxes of 3 and one cell over)
// greedy growth alone wraps around the row ends and fills the mesh with irregular 9-11-cell batches whose surface
// exceeds the dof list (n = 64: 23 340 batches where 21 845 would do; profiles/r03_notes.md section 9).
std::vector<uint32_t> face_neighbours(const Description &m, const Incidence &inc) {
  std::vector<uint32_t> nbr((size_t)m.nc * 6, NONE);
  const uint32_t n_ = (uint32_t)m.n, mid = 1;
  for (uint32_t c = 0; c < m.nc; ++c)
    for (uint32_t axis = 0; axis < 3; ++axis)
      for (uint32_t side = 0; side < 2; ++side) {
        uint32_t ijk[3] = {mid, mid, mid}, opp[3] = {mid, mid, mid};
        ijk[axis] = side ? n_ - 1 : 0;
        opp[axis] = side ? 0 : n_ - 1;
        const uint32_t li = ijk[0] + n_ * ijk[1] + n_ * n_ * ijk[2], lo = opp[0] + n_ * opp[1] + n_ * n_ * opp[2];
        const uint32_t g = m.dofs_of(c)[li];
        if (inc.count(g) != 2) continue;
        const uint32_t c2 = inc.cells[inc.off[g]] == c ? inc.cells[inc.off[g] + 1] : inc.cells[inc.off[g]];
        if (c2 != c && m.dofs_of(c2)[lo] == g) nbr[(size_t)c * 6 + 2 * axis + side] = c2;
      }
  return nbr;
}

// box shapes a x b x c (cells along x, y, z) up to the cell limit: most cells first, then the most compact
struct Shape {
  uint32_t a, b, c;
};
std::vector<Shape> box_shapes(uint32_t Bmax) {
  std::vector<Shape> shapes;
  for (uint32_t a = 1; a <= Bmax; ++a)
    for (uint32_t b2 = 1; a * b2 <= Bmax; ++b2)
      for (uint32_t c2 = 1; a * b2 * c2 <= Bmax; ++c2)
        if (a * b2 * c2 == Bmax) shapes.push_back({a, b2, c2});  // (smaller boxes fragment irregular meshes: the growth does better)
  auto spread = [](const Shape &s2) { return std::max(s2.a, std::max(s2.b, s2.c)) * 4 + s2.a + s2.b + s2.c; };
  std::stable_sort(shapes.begin(), shapes.end(), [&](const Shape &x, const Shape &y) {
    const uint32_t vx = x.a * x.b * x.c, vy = y.a * y.b * y.c;
    if (vx != vy) return vx > vy;
    if (spread(x) != spread(y)) return spread(x) < spread(y);
    return x.a != y.a ? x.a > y.a : x.b > y.b;  // the long side along x: the dofs of a batch are x-runs
  });
  return shapes;
}

// ---- batching.  A batch starts at the lowest unassigned cell -- as a BOX of cells where the mesh offers one (plane
// plans; see below) -- and grows greedily: always the candidate that shares most dofs with the batch (ties: earliest
// discovered), until a limit is hit.  With limits->interior_max (plane kernels) a batch must also keep its SURFACE
// within the pass-2 slots of the dof list: surface = dofs with an incident cell outside the batch, or constrained,
// plus the interior dofs beyond interior_max.  The surface is not monotone in the number of cells, so growth runs to
// the cell / dof limit and the batch is then cut back to the longest prefix of its growth order that satisfied the
// bound.
//
// The grower owns the state of the batch under construction for the whole plan; `stamp` changes with every (re)build,
// so nothing is ever cleared (and nothing is allocated per batch).
class BatchGrower {
 public:
  BatchGrower(const Description &m, const Incidence &inc, const BatchRules &R)
      : m_(m), inc_(inc), R_(R), cell_batch_(m.nc, NONE), dof_stamp_(m.N, NONE), inc_cnt_(R.interior_max ? m.N : 0, 0),
        gain_(m.nc, 0), gain_stamp_(m.nc, NONE) {}
  // (plans whose batches start as boxes; they have one class of cells)
  void use_boxes(std::vector<uint32_t> nbr, std::vector<Shape> shapes) {
    nbr_ = std::move(nbr);
    shapes_ = std::move(shapes);
  }
  uint32_t batch_of(uint32_t c) const { return cell_batch_[c]; }

  // batch number b into `cells` (empty), from the lowest unassigned cell
  void build(uint32_t seed, uint32_t b, std::vector<uint32_t> &cells) {
    b_ = b;
    cells_ = &cells;
    cls_ = R_.masked(seed);
    bound_surface_ = R_.in_planes(cls_);
    lim_ = R_.limits_of(cls_);
    const bool boxed = !shapes_.empty() && try_box(seed);
    if (!boxed) begin();
    cut_back(grow(boxed ? NONE : seed, boxed ? cells.size() : 0));
  }

 private:
  bool surface_ok() const {
    return !bound_surface_ || ndofs_ - std::min(n_enclosed_, R_.interior_max) <= R_.shared_max;
  }
  void begin() {
    for (uint32_t c : *cells_) cell_batch_[c] = NONE;
    cells_->clear();
    cand_.clear();
    ++stamp_;
    ndofs_ = n_enclosed_ = npriv_ = 0;
  }
  void add_cell(uint32_t c) {
    cell_batch_[c] = b_;
    cells_->push_back(c);
    npriv_ += R_.priv_of(c);
    const uint32_t *l2g = m_.dofs_of(c);
    for (uint32_t i = 0; i < m_.nd; ++i) {
      const uint32_t g = l2g[i];
      const bool first = dof_stamp_[g] != stamp_;
      if (bound_surface_) {
        // (a cell listing one dof twice counts once: compare with the previous entries of this cell)
        bool dup = false;
        for (uint32_t i2 = 0; i2 < i && !dup; ++i2) dup = l2g[i2] == g;
        if (!dup) {
          if (first) inc_cnt_[g] = 0;
          if (++inc_cnt_[g] == inc_.count(g) && !m_.constrained[g]) ++n_enclosed_;
        }
      }
      if (!first) continue;
      dof_stamp_[g] = stamp_;
      ++ndofs_;
      if (lim_.max_cells == 1) continue;
      for (uint32_t k = inc_.off[g]; k < inc_.off[g + 1]; ++k) {
        const uint32_t c2 = inc_.cells[k];
        if (cell_batch_[c2] != NONE || R_.masked(c2) != cls_) continue;
        if (gain_stamp_[c2] != stamp_) {
          gain_stamp_[c2] = stamp_;
          gain_[c2] = 0;
          cand_.push_back(c2);
        }
        gain_[c2]++;
      }
    }
  }
  // ---- the box the batch starts as: the first shape whose cells exist from the seed in +x, +y, +z, are unassigned
  // and of the seed's kind, and which keeps every bound.  On a periodic mesh a walk can come back to a cell it has
  // already taken (a ring of 2 cells under a shape 3 cells long): cell_batch_ is only set by add_cell, so such a
  // shape is rejected against box_ itself (at most max_cells entries).
  bool try_box(uint32_t seed) {
    for (const Shape &sh : shapes_) {
      box_.clear();
      bool ok = true;
      uint32_t cz = seed;
      for (uint32_t k = 0; k < sh.c && ok; ++k) {
        uint32_t cy = cz;
        for (uint32_t j = 0; j < sh.b && ok; ++j) {
          uint32_t cx = cy;
          for (uint32_t i = 0; i < sh.a && ok; ++i) {
            if (cx == NONE || cell_batch_[cx] != NONE || R_.masked(cx) != cls_ ||
                std::find(box_.begin(), box_.end(), cx) != box_.end()) {
              ok = false;
              break;
            }
            box_.push_back(cx);
            cx = nbr_[(size_t)cx * 6 + 1];
          }
          cy = cy == NONE ? NONE : nbr_[(size_t)cy * 6 + 3];
          if (cy == NONE && j + 1 < sh.b) ok = false;
        }
        cz = cz == NONE ? NONE : nbr_[(size_t)cz * 6 + 5];
        if (cz == NONE && k + 1 < sh.c) ok = false;
      }
      if (!ok) continue;
      begin();
      for (uint32_t c : box_) add_cell(c);
      if (ndofs_ <= lim_.max_dofs && surface_ok() && npriv_ <= R_.private_max) return true;
    }
    return false;
  }
  // ---- greedy growth (from the seed `next`, or on from the box); returns the longest prefix that kept the bound
  size_t grow(uint32_t next, size_t last_ok) {
    std::vector<uint32_t> &cells = *cells_;
    while (true) {
      if (next != NONE) {
        add_cell(next);
        if (surface_ok()) last_ok = cells.size();
      }
      if (cells.size() >= lim_.max_cells) break;
      // pick best candidate
      uint32_t best = NONE, best_gain = 0;
      size_t w = 0;
      for (size_t k = 0; k < cand_.size(); ++k) {
        const uint32_t c2 = cand_[k];
        if (cell_batch_[c2] != NONE) continue;  // was taken
        cand_[w++] = c2;
        if (gain_[c2] > best_gain) {
          best_gain = gain_[c2];
          best = c2;
        }
      }
      cand_.resize(w);
      if (best == NONE) break;
      if (ndofs_ + (m_.nd - best_gain) > lim_.max_dofs) break;
      if (npriv_ + R_.priv_of(best) > R_.private_max) break;
      next = best;
    }
    return last_ok;
  }
  void cut_back(size_t last_ok) {
    std::vector<uint32_t> &cells = *cells_;
    if (last_ok == 0) last_ok = 1;  // (a single cell over the bound is reported by the classification below)
    for (size_t k = last_ok; k < cells.size(); ++k) cell_batch_[cells[k]] = NONE;
    cells.resize(last_ok);
  }

  const Description &m_;
  const Incidence &inc_;
  const BatchRules &R_;
  std::vector<uint32_t> nbr_;
  std::vector<Shape> shapes_;
  std::vector<uint32_t> cell_batch_;
  std::vector<uint32_t> dof_stamp_;  // stamp of the build that already contains this dof
  std::vector<uint32_t> inc_cnt_;    // incident cells of the dof inside the current batch (plane plans)
  std::vector<uint32_t> gain_, gain_stamp_;
  std::vector<uint32_t> cand_, box_;
  uint32_t stamp_ = 0;
  // the batch under construction
  uint32_t b_ = 0;
  std::vector<uint32_t> *cells_ = nullptr;
  bool cls_ = false, bound_surface_ = false;
  BatchLimits lim_;
  uint32_t ndofs_ = 0, n_enclosed_ = 0, npriv_ = 0;
};

struct Batches {
  std::vector<std::vector<uint32_t>> cells;
  std::vector<uint8_t> masked;  // per batch: class of its cells (segregate only)
};

Batches make_batches(const Description &m, const Incidence &inc, const BatchRules &R) {
  BatchGrower grower(m, inc, R);
  // (conforming meshes only: on the octree meshes with hanging nodes, cells in Morton order and two kinds of cells,
  // boxes anchored at the lowest unassigned cell leave more single-cell leftovers than they fill batches -- 17 899
  // against 17 777 batches on C3)
  if (R.interior_max && !R.segregate && m.dim == 3 && m.n >= 3 && R.plane.max_cells >= 4)
    grower.use_boxes(face_neighbours(m, inc), box_shapes(R.plane.max_cells));
  Batches B;
  uint32_t seed = 0;
  while (true) {
    while (seed < m.nc && grower.batch_of(seed) != NONE) ++seed;
    if (seed >= m.nc) break;
    const uint32_t b = (uint32_t)B.cells.size();
    B.cells.emplace_back();
    B.masked.push_back(R.masked(seed));
    grower.build(seed, b, B.cells.back());
    if (seed < m.nc && grower.batch_of(seed) != b) seed = 0;  // defensive: the seed is the first cell of its batch
  }
  return B;
}

// ---- batch reordering
void plane_batches_first(Batches &B) {  // (stable)
  std::vector<uint32_t> idx(B.cells.size());
  std::iota(idx.begin(), idx.end(), 0u);
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b2) { return B.masked[a] < B.masked[b2]; });
  Batches sorted{std::vector<std::vector<uint32_t>>(idx.size()), std::vector<uint8_t>(idx.size())};
  for (size_t k = 0; k < idx.size(); ++k) {
    sorted.cells[k] = std::move(B.cells[idx[k]]);
    sorted.masked[k] = B.masked[idx[k]];
  }
  B = std::move(sorted);
}

// cells with a hanging-node mask first: the kernel takes the extra interpolation stages for a whole
// chunk of cells as soon as one of them is masked, so masked cells should share chunks
void masked_cells_first(Batches &B, const uint32_t *constraint_mask) {
  for (auto &cells : B.cells)
    std::stable_partition(cells.begin(), cells.end(), [&](uint32_t c) { return constraint_mask[c] != 0; });
}

// ---- per batch: unique dofs, ordered [interior ascending | shared] where interior = touched by this
// batch only (the shared part is re-ordered by toucher group below)
//
// A dof takes the pass-2 route ("shared") if two or more batches touch it.  With limits->interior_max
// (apply_planes3: fixed slot structure of the batch dof list, no per-lane case distinction in the scatter) more
// dofs are DEMOTED to that route although only this batch touches them (one partial sum; pass 2 copies it):
// constrained dofs -- pass 2 writes the identity row of every constrained dof it lists, so the cell loop never
// stores to one --, the interior dofs beyond interior_max, and one dof if the batch would otherwise have no pass-2
// dof at all (the padding entries of the interior slots store a zero to a pass-2 dof of the batch).  A batch with
// more than shared_max pass-2 dofs (the growth above only bounds the total) is split in two and everything is
// classified again.
struct Classified {
  std::vector<std::vector<uint32_t>> bd;  // per batch: its dofs [interior | shared]
  std::vector<uint32_t> ntouch, nint;     // per dof: batches touching it; per batch: interior dofs
  std::vector<uint8_t> shared_flag;
};

int classify_dofs(const Description &m, const BatchRules &R, Batches &B, Classified &C) {
  std::vector<std::vector<uint32_t>> &batches = B.cells, &bd = C.bd;
  std::vector<uint8_t> &batch_masked = B.masked, &shared_flag = C.shared_flag;
  std::vector<uint32_t> &ntouch = C.ntouch, &nint = C.nint;
  for (;;) {
    const uint32_t nb = (uint32_t)batches.size();
    bd.assign(nb, {});
    ntouch.assign(m.N, 0);
    for (uint32_t b = 0; b < nb; ++b) {
      std::vector<uint32_t> &v = bd[b];
      v.reserve(batches[b].size() * m.nd);
      for (uint32_t c : batches[b]) v.insert(v.end(), m.dofs_of(c), m.dofs_of(c) + m.nd);
      std::sort(v.begin(), v.end());
      v.erase(std::unique(v.begin(), v.end()), v.end());
      if (v.size() > R.limits_of(batch_masked[b]).max_dofs || v.size() > 8191u) {
        // (the greedy estimate nd - gain under-counts a cell that lists one dof twice; the kernels hold a batch's
        // dofs in a fixed number of register / LDS slots and byte offsets of batch-local ids in 16 bits)
        set_error("internal: batch exceeds the kernel's dof slots (degenerate loc2glob?)");
        return MFGPU_EINVAL;
      }
      for (uint32_t g : v) ntouch[g]++;
    }
    shared_flag.assign(m.N, 0);
    for (uint32_t g = 0; g < m.N; ++g) shared_flag[g] = ntouch[g] >= 2;
    // constrained dofs a single PLANE batch touches are demoted (the pencil kernel writes its own)
    for (uint32_t b = 0; b < nb; ++b)
      if (R.in_planes(batch_masked[b]))
        for (uint32_t g : bd[b])
          if (ntouch[g] == 1 && m.constrained[g]) shared_flag[g] = 1;
    nint.assign(nb, 0);
    std::vector<uint32_t> too_big;
    for (uint32_t b = 0; b < nb; ++b) {
      std::vector<uint32_t> &v = bd[b];
      std::stable_partition(v.begin(), v.end(), [&](uint32_t g) { return !shared_flag[g]; });
      uint32_t k = 0;
      while (k < v.size() && !shared_flag[v[k]]) ++k;
      if (R.in_planes(batch_masked[b])) {
        uint32_t keep = std::min(k, R.interior_max);
        if (keep == v.size() && keep > 0) --keep;
        for (uint32_t t = keep; t < k; ++t) shared_flag[v[t]] = 1;
        k = keep;
        if (v.size() - k > R.shared_max) too_big.push_back(b);
      }
      nint[b] = k;
    }
    if (too_big.empty()) break;
    for (size_t i = too_big.size(); i-- > 0;) {  // back to front: indices stay valid
      const uint32_t b = too_big[i];
      if (batches[b].size() < 2) {
        set_error("one cell has more pass-2 dofs than the plane kernel's dof-list slots hold");
        return MFGPU_EUNSUPPORTED;
      }
      const size_t half = batches[b].size() / 2;
      std::vector<uint32_t> second(batches[b].begin() + half, batches[b].end());
      batches[b].resize(half);
      batches.insert(batches.begin() + b + 1, std::move(second));
      batch_masked.insert(batch_masked.begin() + b + 1, batch_masked[b]);
    }
  }
  return 0;
}

// ---- greedy colouring of batches (conflict = shared dof), and the execution order
int colour_and_order(const std::vector<std::vector<uint32_t>> &bd, uint32_t N, bool colored,
                     std::vector<uint32_t> &order, std::vector<uint32_t> &color_batch_off) {
  const uint32_t nb = (uint32_t)bd.size();
  std::vector<uint64_t> dof_colors(N, 0);
  std::vector<uint32_t> bcolor(nb, 0);
  uint32_t ncolors = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    uint64_t forbidden = 0;
    for (uint32_t g : bd[b]) forbidden |= dof_colors[g];
    uint32_t c = 0;
    while (c < 64 && (forbidden >> c) & 1) ++c;
    if (c >= 64) {
      set_error("more than 64 batch colours needed");
      return MFGPU_EUNSUPPORTED;
    }
    bcolor[b] = c;
    ncolors = std::max(ncolors, c + 1);
    for (uint32_t g : bd[b]) dof_colors[g] |= (1ull << c);
  }
  // execution order.  Coloured scatter: colour-major, stable (one launch per colour).  Two-pass scatter
  // has no inter-batch dependency: the batches keep their creation order, which follows the caller's
  // cell order and is therefore spatially coherent -- batches that run at the same time on one XCD are
  // mesh neighbours and share the 128-byte lines of src that their dof runs straddle (a colour-major
  // order puts every neighbour into a different colour, i.e. as far apart in time as possible).
  order.resize(nb);
  std::iota(order.begin(), order.end(), 0u);
  if (colored) {
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b2) { return bcolor[a] < bcolor[b2]; });
    color_batch_off.assign(ncolors + 1, 0);
    for (uint32_t b = 0; b < nb; ++b) color_batch_off[bcolor[b] + 1]++;
    for (uint32_t c = 0; c < ncolors; ++c) color_batch_off[c + 1] += color_batch_off[c];
  } else {
    color_batch_off.assign({0u, nb});
  }
  return 0;
}

// ---- shared dofs, grouped by toucher set.  All dofs that are shared by the same set of batches (the
// interior of a face between two batches, of an edge between four, a vertex between eight) form a
// GROUP.  The global shared list (pass 2 walks it) is sorted by (toucher sequence in execution order,
// global id) and every batch lists its shared dofs in that same order, so a group occupies ONE
// contiguous run of halo slots in each of its touchers, with identical dof order: pass 2 reads the
// partial sums of a group as k coalesced runs and needs no per-partial index.
struct SharedGroups {
  std::vector<uint32_t> ids;               // the shared dofs, ascending
  std::vector<uint32_t> t_off, touchers;   // CSR: per entry of ids its touchers' execution positions, ascending
  std::vector<uint32_t> sorder;            // the grouped shared list, as indices into ids
  std::vector<uint32_t> spos;              // global id -> position in the grouped shared list
  bool same_group(uint32_t a, uint32_t b2) const {  // a, b2: indices into ids
    const uint32_t la = t_off[a + 1] - t_off[a], lb = t_off[b2 + 1] - t_off[b2];
    return la == lb && std::equal(&touchers[t_off[a]], &touchers[t_off[a]] + la, &touchers[t_off[b2]]);
  }
};

// (sorts the shared part of every batch's dofs in C.bd into the grouped order)
SharedGroups group_shared_dofs(Classified &C, const std::vector<uint32_t> &order, uint32_t N) {
  SharedGroups G;
  const uint32_t nb = (uint32_t)C.bd.size();
  for (uint32_t g = 0; g < N; ++g)
    if (C.shared_flag[g]) G.ids.push_back(g);
  const size_t ns = G.ids.size();
  std::vector<uint32_t> sid(N, NONE);
  std::vector<uint32_t> &t_off = G.t_off, &touchers = G.touchers;
  t_off.assign(ns + 1, 0);
  for (size_t i = 0; i < ns; ++i) {
    sid[G.ids[i]] = (uint32_t)i;
    t_off[i + 1] = t_off[i] + C.ntouch[G.ids[i]];
  }
  touchers.resize(t_off[ns]);
  {
    std::vector<uint32_t> fill(t_off.begin(), t_off.end() - 1);
    for (uint32_t k = 0; k < nb; ++k)  // ascending execution position
      for (size_t t = C.nint[order[k]]; t < C.bd[order[k]].size(); ++t) touchers[fill[sid[C.bd[order[k]][t]]]++] = k;
  }
  auto seq_less = [&](uint32_t a, uint32_t b2) {  // a, b2: indices into ids
    const uint32_t la = t_off[a + 1] - t_off[a], lb = t_off[b2 + 1] - t_off[b2];
    const uint32_t *pa = &touchers[t_off[a]], *pb = &touchers[t_off[b2]];
    for (uint32_t i = 0; i < la && i < lb; ++i)
      if (pa[i] != pb[i]) return pa[i] < pb[i];
    if (la != lb) return la < lb;
    return a < b2;  // same group: ascending global id
  };
  G.sorder.resize(ns);
  std::iota(G.sorder.begin(), G.sorder.end(), 0u);
  std::sort(G.sorder.begin(), G.sorder.end(), seq_less);
  G.spos.assign(N, NONE);
  for (size_t i = 0; i < ns; ++i) G.spos[G.ids[G.sorder[i]]] = (uint32_t)i;
  for (uint32_t b = 0; b < nb; ++b)
    std::sort(C.bd[b].begin() + C.nint[b], C.bd[b].end(), [&](uint32_t x, uint32_t y) { return G.spos[x] < G.spos[y]; });
  return G;
}

// ---- emit the per-batch arrays in execution order, and the orphans
void emit_batches(Plan &P, const Description &m, const BatchRules &R, const Batches &B, const Classified &C,
                  const std::vector<uint32_t> &order) {
  const uint32_t nb = (uint32_t)order.size();
  P.cell_order.clear();
  P.cell_order.reserve(m.nc);
  P.batch_cell_off.assign(1, 0);
  P.batch_dof_off.assign(1, 0);
  P.bdofs.clear();
  P.bflags.clear();
  P.lmap.assign((size_t)m.nc * m.nd, 0);
  std::vector<uint8_t> touched(m.N, 0);
  std::vector<uint16_t> pos_in_batch(m.N, 0);
  P.max_batch_dofs = P.max_batch_cells = 0;
  P.n_first = P.n_add = 0;
  P.batch_nint.clear();
  P.halo_off.assign(1, 0);
  for (uint32_t k = 0; k < nb; ++k) {
    const uint32_t b = order[k];
    const std::vector<uint32_t> &v = C.bd[b];
    P.batch_nint.push_back(C.nint[b]);
    // (apply_planes3: every batch owns a fixed number of halo slots, so a slot index follows from the batch index)
    P.halo_off.push_back(P.halo_off.back() +
                         (R.in_planes(B.masked[b]) ? R.halo_stride : (uint32_t)(v.size() - C.nint[b])));
    for (uint32_t g : v) {
      uint8_t f = 0;
      if (m.constrained[g]) f |= kFlagConstrained;
      if (touched[g]) {
        f |= kFlagAdd;
        ++P.n_add;
      } else {
        touched[g] = 1;
        ++P.n_first;
      }
      P.bdofs.push_back(m.flagged(g));
      P.bflags.push_back(f);
    }
    for (size_t t = 0; t < v.size(); ++t) pos_in_batch[v[t]] = (uint16_t)t;  // valid for this batch's dofs only
    for (uint32_t c : B.cells[b]) {
      const size_t pos = P.cell_order.size();
      P.cell_order.push_back(c);
      for (uint32_t i = 0; i < m.nd; ++i) P.lmap[pos * m.nd + i] = pos_in_batch[m.dofs_of(c)[i]];
    }
    P.batch_cell_off.push_back((uint32_t)P.cell_order.size());
    P.batch_dof_off.push_back((uint32_t)P.bdofs.size());
    P.max_batch_dofs = std::max<uint32_t>(P.max_batch_dofs, (uint32_t)v.size());
    P.max_batch_cells = std::max<uint32_t>(P.max_batch_cells, (uint32_t)B.cells[b].size());
  }
  P.orphans.clear();
  for (uint32_t g = 0; g < m.N; ++g)
    if (!touched[g]) P.orphans.push_back(m.flagged(g));
}

void count_plane_batches(Plan &P, const BatchRules &R, const std::vector<uint8_t> &batch_masked) {
  P.n_plane_batches = P.n_plain_plane_batches = 0;
  for (const uint8_t cls : batch_masked)
    if (R.in_planes(cls)) {
      ++P.n_plane_batches;
      P.n_plain_plane_batches += cls ? 0u : 1u;
    }
  // masked_planes: the two kinds are interleaved, every plane batch runs in the <HN> instantiation
  if (P.n_plain_plane_batches < P.n_plane_batches) P.n_plain_plane_batches = 0;
}

// ---- second pass.  sdofs: the grouped shared list.  (s_off, s_idx): CSR of the halo slots of every
// shared dof in ascending execution order of the batches -- the generic form, used by the host-side
// checks and by reduce_shared when the groups are too small to pay (irregular meshes).
void emit_pass2_csr(Plan &P, const Description &m, const std::vector<uint32_t> &ntouch, const SharedGroups &G) {
  const size_t ns = G.ids.size(), nb = P.batch_nint.size();
  P.sdofs.resize(ns);
  for (size_t i = 0; i < ns; ++i) P.sdofs[i] = m.flagged(G.ids[G.sorder[i]]);
  P.s_off.assign(ns + 1, 0);
  for (size_t i = 0; i < ns; ++i) P.s_off[i + 1] = P.s_off[i] + ntouch[P.sdofs[i] & 0x7fffffffu];
  P.s_idx.assign(P.s_off[ns], 0);
  std::vector<uint32_t> fill(P.s_off.begin(), P.s_off.end() - 1);
  for (size_t k = 0; k < nb; ++k) {
    const uint32_t ni = P.batch_nint[k];
    const uint32_t d0 = P.batch_dof_off[k], d1 = P.batch_dof_off[k + 1];
    for (uint32_t t = d0 + ni; t < d1; ++t) {
      const uint32_t g = P.bdofs[t] & 0x7fffffffu;
      P.s_idx[fill[G.spos[g]]++] = P.halo_off[k] + (t - d0 - ni);
    }
  }
}

// HOST ONLY (no device code reads it; mfgpu_plan_array_u32 ids 11 and 12, checked by the host tests).  (chunks,
// gstarts): the grouped form -- a chunk is up to 64 consecutive dofs of one group; its k partial sums
// per dof sit at gstarts[tstart + t] + offset + lane, t = 0..k-1.
void emit_pass2_groups(Plan &P, const SharedGroups &G) {
  const size_t ns = G.ids.size();
  P.chunks.clear();
  P.gstarts.clear();
  for (size_t i = 0; i < ns;) {
    size_t j = i + 1;
    while (j < ns && G.same_group(G.sorder[i], G.sorder[j])) ++j;
    const uint32_t k = P.s_off[i + 1] - P.s_off[i], tstart = (uint32_t)P.gstarts.size();
    for (uint32_t t = 0; t < k; ++t) P.gstarts.push_back(P.s_idx[P.s_off[i] + t]);  // first dof's slots
    for (size_t o = i; o < j; o += 64) {
      const uint32_t cnt = (uint32_t)std::min<size_t>(64, j - o);
      P.chunks.push_back((uint32_t)o);
      P.chunks.push_back(cnt | (k << 16));
      P.chunks.push_back(tstart);
      P.chunks.push_back((uint32_t)(o - i));
    }
    i = j;
  }
}
}  // namespace

int build_plan(const mfgpu_desc &d, Plan &P, uint32_t max_chunks, const PlanLimits *limits) {
  int rc;
  Description m;
  if ((rc = check_description(d, m))) return rc;
  P.dim = d.dim;
  P.degree = d.degree;
  P.n = m.n;
  P.nd = (int)m.nd;
  P.n_dofs = d.n_dofs;
  P.n_cells = d.n_cells;
  BatchRules R;
  if ((rc = resolve_batch_rules(d, max_chunks, limits, R))) return rc;
  const Incidence inc = dof_cell_incidence(m);
  Batches B = make_batches(m, inc, R);
  // the batches of a class that runs in the pencil kernel go behind the plane batches
  if (R.segregate && !R.in_planes(true)) plane_batches_first(B);
  if ((d.flags & MFGPU_HANGING_NODES) && d.constraint_mask) masked_cells_first(B, d.constraint_mask);
  Classified C;
  if ((rc = classify_dofs(m, R, B, C))) return rc;
  std::vector<uint32_t> order;  // execution position -> batch
  if ((rc = colour_and_order(C.bd, m.N, (d.flags & MFGPU_COLORED_SCATTER) != 0, order, P.color_batch_off))) return rc;
  const SharedGroups G = group_shared_dofs(C, order, m.N);
  emit_batches(P, m, R, B, C, order);
  count_plane_batches(P, R, B.masked);
  emit_pass2_csr(P, m, C.ntouch, G);
  emit_pass2_groups(P, G);
  return 0;
}

// Fixed-size per-batch records of apply_planes3.  Dof list: p_ji slots of interior dofs, padded with a pass-2 dof
// of the batch (the padding lanes store the zero their never-touched accumulator slot holds, or old + 0, to a dof
// pass 2 rewrites), then p_hs slots of pass-2 dofs, padded with the last one.  Index runs: per task (cell c, plane
// k) the n*n slot numbers of the xy-plane z = k as byte offsets (slot * 8) packed two per word, stored
// [word][task] so that a wave reads consecutive words; the tasks of cells a ragged batch does not have point at
// the list's last slot, which is padding in every batch the planner accepts.
// (constraint_mask: the description's, caller's cell order; nullptr on conforming meshes)
int build_plane_records(Plan &P, const uint32_t *constraint_mask) {
  const int n = P.n, n2 = n * n, NT = p_cells_per_wave(n) * n, NIW = (n2 + 1) / 2;
  const int JI = p_ji(n) * 64, NB = p_kgu(n) * 64;
  const size_t nbat = P.n_plane_batches;
  const uint32_t dummy = 8u * (uint32_t)(NB - 1);
  std::vector<uint32_t> &bd = P.pr_dofs, &ix = P.pr_idx;
  bd.assign((size_t)NB * nbat, 0u);
  ix.assign((size_t)NIW * NT * nbat, dummy | (dummy << 16));
  std::vector<uint32_t> slot_of;  // batch-local id (position in P.bdofs) -> slot
  // batches of cells WITH a hanging-node mask (<HN> instantiation; anywhere behind the first n_plain_plane_batches): the
  // constrained nodes of a cell (those on a line one of the interpolation passes of hanging_nodes.cuh:617-696
  // touches) get PRIVATE positions behind the dof list; the cell's index runs point there.  Per batch: a copy list
  // (private position <- position of the node's dof in the list) and per direction the line operations, each the n
  // private positions of a line in the order the plain weight matrix applies to (hn_cell_lines).
  const int HROWS = p_hn_rows(n), CR = p_priv_max(n) / 64;
  std::vector<uint32_t> &hnrec = P.pr_hn;
  hnrec.clear();
  P.pr_hn_slot.assign(nbat, 0xffffffffu);
  std::vector<HnLine> lines[3];
  std::vector<uint16_t> pnodes;
  std::vector<uint32_t> priv_pos((size_t)P.nd);
  for (size_t b = 0; b < nbat; ++b) {
    const uint32_t c0 = P.batch_cell_off[b], nc = P.batch_cell_off[b + 1] - c0;
    const uint32_t d0 = P.batch_dof_off[b], nbd = P.batch_dof_off[b + 1] - d0, ni = P.batch_nint[b];
    if ((int)nc * n > NT || (int)ni > JI || (int)(nbd - ni) >= NB - JI || nbd == ni) {
      set_error("internal: batch does not fit the plane kernel's dof-list slots");
      return MFGPU_EINVAL;
    }
    slot_of.assign(nbd, 0u);
    for (uint32_t t = 0; t < nbd; ++t) slot_of[t] = t < ni ? t : (uint32_t)JI + (t - ni);
    for (int t = 0; t < NB; ++t) {
      uint32_t src_t;
      if (t < JI) src_t = (uint32_t)t < ni ? (uint32_t)t : ni;  // padding: the first pass-2 dof
      else src_t = std::min<uint32_t>(ni + (uint32_t)(t - JI), nbd - 1);
      bd[b * NB + t] = P.bdofs[d0 + src_t];
    }
    bool hnb = false;  // (a batch holds masked cells only or unmasked cells only)
    if (constraint_mask && b >= P.n_plain_plane_batches)
      for (uint32_t c = 0; c < nc; ++c) hnb = hnb || constraint_mask[P.cell_order[c0 + c]] != 0;
    uint32_t next_priv = (uint32_t)NB;
    std::vector<uint32_t> copies, ops_d[3];
    for (uint32_t c = 0; c < nc; ++c) {
      const unsigned mask = hnb ? constraint_mask[P.cell_order[c0 + c]] : 0u;
      std::fill(priv_pos.begin(), priv_pos.end(), 0xffffffffu);
      if (mask) {
        hn_cell_lines(mask, n, lines, pnodes);
        for (uint16_t node : pnodes) {
          if (next_priv >= (uint32_t)NB + (uint32_t)p_priv_max(n)) {  // (the planner budgets them)
            set_error("internal: batch exceeds the plane kernel's private hanging-node entries");
            return MFGPU_EINVAL;
          }
          priv_pos[node] = next_priv;
          copies.push_back((next_priv << 16) | slot_of[P.lmap[(size_t)(c0 + c) * P.nd + node]]);
          ++next_priv;
        }
        for (int dir = 0; dir < 3; ++dir)
          for (const HnLine &L : lines[dir]) {
            uint32_t w[3] = {0u, 0u, 0u};
            for (int t = 0; t < n; ++t) w[t >> 1] |= priv_pos[L.node[t]] << (16 * (t & 1));
            ops_d[dir].insert(ops_d[dir].end(), w, w + 3);
          }
      }
      for (int k = 0; k < n; ++k)
        for (int i = 0; i < n2; ++i) {
          const int node = i + n2 * k;
          const uint32_t pos = priv_pos[node] != 0xffffffffu ? priv_pos[node] : slot_of[P.lmap[(size_t)(c0 + c) * P.nd + node]];
          const uint32_t off = 8u * pos;
          uint32_t &w = ix[(b * NIW + i / 2) * NT + c * n + k];
          w = (i & 1) ? ((w & 0xffffu) | (off << 16)) : ((w & 0xffff0000u) | off);
        }
    }
    if (hnb) {
      P.pr_hn_slot[b] = (uint32_t)(hnrec.size() / ((size_t)HROWS * 64));
      hnrec.resize(hnrec.size() + (size_t)HROWS * 64, 0u);
      uint32_t *rec = hnrec.data() + (size_t)P.pr_hn_slot[b] * HROWS * 64;
      for (size_t e = 0; e < copies.size(); ++e) rec[e] = copies[e];  // rows 0 .. CR-1, entry e at [e / 64][e % 64]
      for (int dir = 0; dir < 3; ++dir) {
        const size_t nops = ops_d[dir].size() / 3;
        if (nops > (size_t)kHnOpRounds * 64) {
          set_error("internal: more hanging-node lines in a batch than the plane kernel's record holds");
          return MFGPU_EINVAL;
        }
        for (size_t e = 0; e < nops; ++e)
          for (int w = 0; w < 3; ++w)
            rec[(size_t)(CR + (dir * kHnOpRounds + (int)(e / 64)) * 3 + w) * 64 + e % 64] = ops_d[dir][e * 3 + w];
      }
      const uint32_t h0 = (uint32_t)copies.size() | ((uint32_t)(ops_d[0].size() / 3) << 16);
      const uint32_t h1 = (uint32_t)(ops_d[1].size() / 3) | ((uint32_t)(ops_d[2].size() / 3) << 16);
      for (int l = 0; l < 64; ++l) {
        rec[(size_t)(HROWS - 2) * 64 + l] = h0;
        rec[(size_t)(HROWS - 1) * 64 + l] = h1;
      }
    }
  }
  share_plane_records(P);
  share_pass2_records(P);
  return 0;
}

namespace {
// FNV-1a over 32-bit words
uint64_t hash_words(const uint32_t *w, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ w[i]) * 1099511628211ull;
  return h;
}

// Appends rec[0 .. len) to table unless an equal record (same length, same words) is there already (hash, then
// compare); returns the record's word offset in table.  Records of one fixed length: offset / len is the record's number.
using SeenRecords = std::unordered_multimap<uint64_t, std::pair<size_t, size_t>>;  // hash -> (offset, length)
size_t intern_record(std::vector<uint32_t> &table, SeenRecords &seen, const uint32_t *rec, size_t len) {
  const uint64_t h = hash_words(rec, len);
  const auto range = seen.equal_range(h);
  for (auto it = range.first; it != range.second; ++it)
    if (it->second.second == len && !std::memcmp(table.data() + it->second.first, rec, len * sizeof(uint32_t)))
      return it->second.first;
  const size_t off = table.size();
  table.insert(table.end(), rec, rec + len);
  seen.emplace(h, std::make_pair(off, len));
  return off;
}
}  // namespace

void share_plane_records(Plan &P) {
  const int n = P.n, NT = p_cells_per_wave(n) * n, NIW = (n * n + 1) / 2;
  const size_t NB = (size_t)p_kgu(n) * 64, NX = (size_t)NIW * NT, nbat = P.n_plane_batches;
  P.sh_dofs.clear();
  P.sh_idx.clear();
  P.sh_batch.assign(nbat * kShBatchWords, 0u);
  SeenRecords seen_d, seen_x;
  std::vector<uint32_t> rel(NB);
  for (size_t b = 0; b < nbat; ++b) {
    const uint32_t *g = P.pr_dofs.data() + b * NB;
    uint32_t base = 0x7fffffffu;
    for (size_t t = 0; t < NB; ++t) base = std::min(base, g[t] & 0x7fffffffu);
    for (size_t t = 0; t < NB; ++t) rel[t] = g[t] - base;  // (bit 31 survives: the low 31 bits are >= base)
    uint32_t *e = P.sh_batch.data() + b * kShBatchWords;
    e[0] = base;
    e[1] = (uint32_t)(intern_record(P.sh_dofs, seen_d, rel.data(), NB) / NB);
    e[2] = (uint32_t)(intern_record(P.sh_idx, seen_x, P.pr_idx.data() + b * NX, NX) / NX);
  }
  const size_t shared = P.sh_dofs.size() + P.sh_idx.size() + P.sh_batch.size();
  const size_t expanded = P.pr_dofs.size() + P.pr_idx.size();
  P.sh_use = nbat > 0 && P.pr_hn.empty() && (double)shared <= kShareMaxFraction * (double)expanded;
}

void share_pass2_records(Plan &P) {
  P.sh_p2rec.clear();
  P.sh_p2tab.clear();
  P.sh_p2_use = false;
  const size_t nb = P.batch_cell_off.size() - 1;
  const uint32_t hs = (uint32_t)p_hs(P.n) * 64u;
  if (nb == 0 || P.n_plane_batches != nb || P.halo_off.size() != nb + 1 || hs > (1u << kP2SlotBits)) return;
  for (size_t b = 0; b <= nb; ++b)
    if (P.halo_off[b] != (uint64_t)b * hs) return;  // (plane plans: every batch owns hs halo slots)
  std::vector<std::vector<uint32_t>> owned(nb);
  size_t expanded = 0;
  for (size_t i = 0; i < P.sdofs.size(); ++i) {
    const uint32_t k = P.s_off[i + 1] - P.s_off[i];
    expanded += 1 + (k ? k : 1);
    if (k == 0) continue;  // (stays with reduce_classes)
    if (k > (uint32_t)kP2MaxK) return;
    const uint32_t owner = P.s_idx[P.s_off[i]] / hs;
    for (uint32_t t = 0; t < k; ++t) {  // ascending toucher order, batch deltas that fit the packed word
      const uint32_t tb = P.s_idx[P.s_off[i] + t] / hs;
      if (tb >= nb || tb < owner || tb - owner >= (1u << (32 - kP2SlotBits))) return;
    }
    owned[owner].push_back((uint32_t)i);
  }
  P.sh_p2tab.assign(2 * nb, 0u);
  SeenRecords seen;
  std::vector<uint32_t> rec;
  for (size_t b = 0; b < nb; ++b) {
    std::vector<uint32_t> &m = owned[b];
    auto k_of = [&](uint32_t i) { return P.s_off[i + 1] - P.s_off[i]; };
    std::stable_sort(m.begin(), m.end(), [&](uint32_t x, uint32_t y) { return k_of(x) > k_of(y); });
    const uint32_t base = P.sh_batch[b * kShBatchWords], ne = (uint32_t)m.size(), kmax = ne ? k_of(m[0]) : 0u;
    auto pad = [](uint32_t x) { return (x + 63u) & ~63u; };
    const uint32_t e0 = pad(ne);
    rec.assign(kP2Header, 0u);
    rec[0] = ne;
    rec[1] = e0;
    rec[2] = kmax;
    rec.resize(kP2Header + 2 * (size_t)e0, 0u);
    for (uint32_t e = 0; e < e0; ++e) rec[kP2Header + e] = e < ne ? P.sdofs[m[e]] - base : 0xffffffffu;
    for (uint32_t e = 0; e < ne; ++e) rec[kP2Header + e0 + e] = k_of(m[e]);
    for (uint32_t t = 0; t < kmax; ++t) {
      uint32_t cnt = 0;  // (sorted by k descending: the entries with k > t are a prefix)
      while (cnt < ne && k_of(m[cnt]) > t) ++cnt;
      rec[3 + t] = (uint32_t)rec.size();
      rec.resize(rec.size() + pad(cnt), 0u);
      for (uint32_t e = 0; e < cnt; ++e) {
        const uint32_t slot = P.s_idx[P.s_off[m[e]] + t], tb = slot / hs;
        rec[rec[3 + t] + e] = ((tb - (uint32_t)b) << kP2SlotBits) | (slot - tb * hs);
      }
    }
    P.sh_p2tab[2 * b] = base;
    P.sh_p2tab[2 * b + 1] = (uint32_t)intern_record(P.sh_p2rec, seen, rec.data(), rec.size());
  }
  const size_t shared = P.sh_p2rec.size() + P.sh_p2tab.size();
  P.sh_p2_use = (double)shared <= kShareMaxFraction * (double)expanded;
}

int choose_kernel_and_plan(const mfgpu_desc &d, PlaneKernel &pk, BatchKernel &bk, Plan &plan) {
  const bool general = !(d.flags & MFGPU_UNIFORM_J0), hn = (d.flags & MFGPU_HANGING_NODES) != 0;
  const bool colored = (d.flags & MFGPU_COLORED_SCATTER) != 0;
  if (d.kernel > MFGPU_KERNEL_PLANES_2W) {
    set_error("unknown mfgpu_desc.kernel");
    return MFGPU_EINVAL;
  }
  // (with hanging nodes: the cells without a mask run in the plane kernel, the masked ones in apply_batches_x)
  const bool pk_ok = d.dim == 3 && !general && !colored && d.degree >= 2 && d.degree <= 6 &&
                     d.n_dofs < (1u << 29);  // (vectors are addressed base + 32-bit byte offset)
  const bool xk_ok = d.dim == 3 && !general && !colored;
  const bool want_planes = d.kernel == MFGPU_KERNEL_PLANES || d.kernel == MFGPU_KERNEL_PLANES_2W;
  if ((want_planes && !pk_ok) || (d.kernel == MFGPU_KERNEL_PENCILS_X && !xk_ok) ||
      (d.kernel == MFGPU_KERNEL_PENCILS && general)) {
    set_error("mfgpu_desc.kernel: this kernel family does not cover the description (see include/mfgpu.h)");
    return MFGPU_EUNSUPPORTED;
  }
  // which plane kernel: apply_planes4 on request, at p = 5, 6 (the only one that fits), and by default at p = 3 in
  // double; apply_planes3 otherwise (p = 4: equal in double, faster in float)
  const bool planes4 = d.kernel == MFGPU_KERNEL_PLANES_2W || d.degree >= 5 ||
                       (d.kernel == MFGPU_KERNEL_AUTO && d.degree == 3 && d.number_type == MFGPU_F64);
  const PlaneKernel plane_kind = planes4 ? PlaneKernel::planes4 : PlaneKernel::planes3;
  const bool mass = d.mass_coefficient != nullptr;
  auto plane_kernel_exists = [&](bool with_hn) {
    return kernel_exists(plane_kind, d.degree + 1, d.number_type, with_hn, false, mass);
  };
  // mass term: where that plane kernel has no MASS instantiation (kernel_exists), the degree runs in the pencil kernel,
  // whose plan is the one of MFGPU_KERNEL_PENCILS_X, and a request for the plane family is refused
  const bool mass_without_planes = mass && pk_ok && !plane_kernel_exists(false);
  if (mass_without_planes && want_planes) {
    set_error("mfgpu_desc.kernel: this plane kernel has no mass-term instantiation at this degree (apply_planes4w at "
              "p = 5, 6; apply_planes4 at p = 4 in double); use MFGPU_KERNEL_AUTO or MFGPU_KERNEL_PENCILS_X");
    return MFGPU_EUNSUPPORTED;
  }
  // by default the plane kernel serves p = 4 only: at p = 2, 3 the pencil kernel measures faster
  // (on meshes with hanging nodes also p = 3: 0.174 instead of 0.256 ms on the bmop ADAPTIVE_GRID mesh, n_ref = 6)
  // p = 5, 6: apply_planes4 with one wave per SIMD (apply_planes3's two transpose arrays do not fit the LDS there)
  // p = 3: apply_planes4 with two waves per SIMD (16 cells per wave) measures 9 % faster than the pencil kernel per
  // vmult (0.222 vs 0.243 ms at 10^7 dofs; profiles/r03_notes.md); p = 2: the pencil kernel stays ahead
  // (in float the pencil kernel is ahead at p = 3 on conforming meshes: 0.152 vs 0.179 ms)
  bool planes = pk_ok && !mass_without_planes && (want_planes || (d.kernel == MFGPU_KERNEL_AUTO &&
                                     (d.degree >= 4 || (d.degree == 3 && (hn || d.number_type == MFGPU_F64)))));
  bool pencils_x = xk_ok && !planes && d.kernel != MFGPU_KERNEL_PENCILS;
  PlanLimits lim;
  if (planes) {
    lim.max_cells = (uint32_t)p_cells_per_wave(d.degree + 1);
    lim.max_dofs = (uint32_t)p_kgu(d.degree + 1) * 64u - 1u;
    lim.interior_max = (uint32_t)p_ji(d.degree + 1) * 64u;
    lim.halo_stride = (uint32_t)p_hs(d.degree + 1) * 64u;
    lim.shared_max = lim.halo_stride - 1u;  // the list's last slot stays padding (idle tasks)
    lim.segregate_masked = hn;
    // cells with a hanging-node mask run in the plane kernel too (apply_planes3<HN>), in batches of their own
    lim.masked_planes = hn && plane_kernel_exists(true);  // (else masked cells stay in the pencil kernel: p = 5, 6)
    lim.private_max = (uint32_t)p_priv_max(d.degree + 1);
  }
  // apply_batches_x unrolls 4 chunks at p=3 (64-cell batches = 13^3 dofs like p=4); everything else 3
  int rc = build_plan(d, plan, (pencils_x && d.degree == 3) ? 4u : 3u, planes ? &lim : nullptr);
  if (rc == MFGPU_EUNSUPPORTED && planes && d.kernel == MFGPU_KERNEL_AUTO && xk_ok) {
    // a cell with more surface dofs than the plane kernel's dof-list slots hold (cannot happen on conforming
    // hexahedral meshes): the pencil kernel has no such limit
    planes = false;
    pencils_x = true;
    plan = Plan();
    rc = build_plan(d, plan, d.degree == 3 ? 4u : 3u, nullptr);
  }
  if (!rc && planes) {
    const uint32_t nbat = (uint32_t)plan.batch_cell_off.size() - 1;
    pencils_x = plan.n_plane_batches < nbat;  // the masked cells' batches
    if (plan.n_plane_batches == 0) planes = false;
  }
  pk = planes ? plane_kind : PlaneKernel::none;
  bk = pencils_x ? BatchKernel::x : general ? (d.dim == 2 ? BatchKernel::g2 : BatchKernel::g)
                                   : planes ? BatchKernel::none : BatchKernel::batches;
  assert(rc || (pk != PlaneKernel::none) == (plan.n_plane_batches > 0));
  return rc;
}

}  // namespace mfgpu

namespace mfgpu {
std::vector<uint32_t> multi_groups(uint32_t n_vectors, const std::vector<uint32_t> &widths) {
  std::vector<uint32_t> groups;
  uint32_t left = n_vectors;
  for (uint32_t w : widths)
    for (; w > 1 && left >= w; left -= w) groups.push_back(w);
  groups.insert(groups.end(), left, 1u);
  return groups;
}

// Lane -> pencil maps of the y- and z-stage (see apply_batches_x).  LDS rules (MI355X_MICROARCH.md): a
// ds_read_b64 is served in 32-lane groups, a double occupies slot (index mod 32); ds_write_b64 / ds_read2_b64
// in 16-lane groups, slot (index mod 16).  All n elements of a pencil shift its base by the same stride, so
// only the bases matter: the pencil whose base has residue r mod 32 gets lane 32 k + r (k-th pencil with that
// residue) -- distinct slots in every 32-lane group, and in each of its 16-lane halves.  Residue classes with
// more than 8 pencils (4 pencils at p=4 in the y-stage, 2 in the z-stage) overflow into the idle lanes, which
// all sit in the last group.
std::vector<uint16_t> x_lane_permutation(int n) {
  const int n2 = n * n, PP = n2, CH = 256 / PP, ndl = n2 * n;
  std::vector<uint16_t> perm(512, 0xffff);
  for (int layout = 0; layout < 2; ++layout) {
    uint16_t *lanes = perm.data() + 256 * layout;
    std::vector<int> fill(32, 0), overflow;
    for (int q = 0; q < CH * PP; ++q) {
      const int cell = q / PP, pen = q % PP, a = pen % n, b = pen / n;
      const int base = cell * ndl + (layout == 0 ? a + n2 * b : a + n * b);
      const int r = base & 31;
      if (fill[r] < 8) lanes[32 * fill[r]++ + r] = (uint16_t)q;
      else overflow.push_back(q);
    }
    for (int l = 255; l >= 0 && !overflow.empty(); --l)
      if (lanes[l] == 0xffff) {
        lanes[l] = (uint16_t)overflow.back();
        overflow.pop_back();
      }
  }
  return perm;
}

std::vector<uint16_t> x_pencil_runs(const std::vector<uint16_t> &lmap, int n_) {
  const size_t n = (size_t)n_, np = (n + 1) & ~(size_t)1, runs = lmap.size() / n;
  std::vector<uint16_t> lx(runs * np, 0);
  for (size_t r = 0; r < runs; ++r)
    for (size_t i = 0; i < n; ++i) lx[r * np + i] = lmap[r * n + i];
  return lx;
}

int pass2_groups(const Plan &P, const std::vector<uint32_t> &seg_end, const uint32_t *priority, uint32_t n_priority,
                 bool shared, std::vector<Pass2Group> &groups) {
  std::vector<uint8_t> prio(P.n_dofs, 0);
  for (uint32_t i = 0; i < n_priority; ++i) {
    if (priority[i] >= P.n_dofs) {
      set_error("priority dof out of range");
      return MFGPU_EINVAL;
    }
    prio[priority[i]] = 1;
  }
  groups.assign(1 + seg_end.size(), Pass2Group());
  auto add = [&](uint32_t dof, const uint32_t *slots, uint32_t k, size_t seg) {
    Pass2Group &g = groups[prio[dof & 0x7fffffffu] ? 0 : 1 + seg];
    g.dofs.push_back(dof);
    g.slots.insert(g.slots.end(), slots, slots + k);
    g.offsets.push_back((uint32_t)g.slots.size());
  };
  for (size_t i = 0; i < P.sdofs.size(); ++i) {
    // the slots of a dof are listed in ascending batch order: the last one belongs to its last toucher
    size_t seg = 0;
    if (shared && P.s_off[i + 1] > P.s_off[i]) continue;  // (in its owner batch's record)
    if (P.s_off[i + 1] > P.s_off[i]) {
      const uint32_t slot = P.s_idx[P.s_off[i + 1] - 1];
      const uint32_t batch = (uint32_t)(std::upper_bound(P.halo_off.begin(), P.halo_off.end(), slot) - P.halo_off.begin()) - 1;
      seg = (size_t)(std::upper_bound(seg_end.begin(), seg_end.end(), batch) - seg_end.begin());
      if (seg >= seg_end.size()) seg = seg_end.size() - 1;
    }
    add(P.sdofs[i], P.s_idx.data() + P.s_off[i], P.s_off[i + 1] - P.s_off[i], seg);
  }
  const uint32_t zero_slot = P.halo_off.empty() ? 0u : P.halo_off.back();
  for (uint32_t orph : P.orphans) add(orph, &zero_slot, 1, 0);  // depend on no batch
  return 0;
}
}  // namespace mfgpu

extern "C" {

const char *mfgpu_last_error(void) { return mfgpu::last_error(); }

int mfgpu_plan_create(const mfgpu_desc *desc, mfgpu_plan **out) {
  if (!desc || !out) {
    mfgpu::set_error("null argument");
    return MFGPU_EINVAL;
  }
  mfgpu_plan *p = new mfgpu_plan();
  mfgpu::PlaneKernel pk;
  mfgpu::BatchKernel bk;
  mfgpu_desc d = *desc;
  d.mass_coefficient = nullptr;  // the plan is the Laplace operator's, with or without a mass term
  int rc = mfgpu::choose_kernel_and_plan(d, pk, bk, p->plan);
  if (!rc && pk != mfgpu::PlaneKernel::none) rc = mfgpu::build_plane_records(p->plan, desc->constraint_mask);
  if (rc) {
    delete p;
    return rc;
  }
  *out = p;
  return 0;
}

void mfgpu_plan_destroy(mfgpu_plan *p) { delete p; }

size_t mfgpu_desc_size(void) { return sizeof(mfgpu_desc); }

int mfgpu_suggest_renumbering(const mfgpu_desc *desc, uint32_t *new_index) {
  if (!desc || !new_index) {
    mfgpu::set_error("null argument");
    return MFGPU_EINVAL;
  }
  mfgpu::Plan P;
  mfgpu::PlaneKernel pk;
  mfgpu::BatchKernel bk;
  mfgpu_desc d = *desc;
  d.mass_coefficient = nullptr;  // (as mfgpu_plan_create)
  int rc = mfgpu::choose_kernel_and_plan(d, pk, bk, P);
  if (rc) return rc;
  // batch-major: the dofs a batch owns alone, batch after batch (one contiguous run per batch: coalesced gathers and
  // stores of the cell loop), then the dofs several batches share in the order pass 2 walks them (grouped by the set
  // of batches: whole lines for pass 2 instead of isolated entries of a lexicographic numbering), then the dofs no
  // cell touches
  const uint32_t NONE = 0xffffffffu;
  std::fill(new_index, new_index + desc->n_dofs, NONE);
  uint32_t next = 0;
  const size_t nb = P.batch_cell_off.size() - 1;
  for (size_t b = 0; b < nb; ++b) {
    const uint32_t d0 = P.batch_dof_off[b];
    // coloured mode has no interior / shared split: a dof goes with the first batch that lists it
    const uint32_t ni = P.batch_nint.empty() ? P.batch_dof_off[b + 1] - d0 : P.batch_nint[b];
    for (uint32_t t = 0; t < ni; ++t) {
      const uint32_t g = P.bdofs[d0 + t] & 0x7fffffffu;
      if (new_index[g] == NONE) new_index[g] = next++;
    }
  }
  for (uint32_t e : P.sdofs) {
    const uint32_t g = e & 0x7fffffffu;
    if (new_index[g] == NONE) new_index[g] = next++;
  }
  for (uint32_t g = 0; g < desc->n_dofs; ++g)
    if (new_index[g] == NONE) new_index[g] = next++;
  if (next != desc->n_dofs) {
    mfgpu::set_error("internal: renumbering is not a permutation");
    return MFGPU_EINVAL;
  }
  return 0;
}

int64_t mfgpu_plan_array_u32(const mfgpu_plan *p, int what, const uint32_t **ptr) {
  if (!p || !ptr) return MFGPU_EINVAL;
  const std::vector<uint32_t> *v = nullptr;
  switch (what) {
    case 0: v = &p->plan.batch_cell_off; break;
    case 1: v = &p->plan.batch_dof_off; break;
    case 2: v = &p->plan.color_batch_off; break;
    case 3: v = &p->plan.cell_order; break;
    case 4: v = &p->plan.bdofs; break;
    case 5: v = &p->plan.orphans; break;
    case 6: v = &p->plan.batch_nint; break;
    case 7: v = &p->plan.halo_off; break;
    case 8: v = &p->plan.sdofs; break;
    case 9: v = &p->plan.s_off; break;
    case 10: v = &p->plan.s_idx; break;
    case 11: v = &p->plan.chunks; break;
    case 12: v = &p->plan.gstarts; break;
    case 13: v = &p->plan.pr_dofs; break;
    case 14: v = &p->plan.pr_idx; break;
    case 15: v = &p->plan.pr_hn; break;
    case 16: v = &p->plan.pr_hn_slot; break;
    case 17: v = &p->plan.sh_dofs; break;
    case 18: v = &p->plan.sh_idx; break;
    case 19: v = &p->plan.sh_batch; break;
    case 20: v = &p->plan.sh_p2rec; break;
    case 21: v = &p->plan.sh_p2tab; break;
    default: mfgpu::set_error("bad array id"); return MFGPU_EINVAL;
  }
  *ptr = v->data();
  return (int64_t)v->size();
}

int mfgpu_plan_multi_groups(uint32_t n_vectors, const uint32_t *widths, uint32_t n_widths, uint32_t *groups,
                            uint32_t capacity) {
  if ((!widths && n_widths) || (!groups && capacity)) return MFGPU_EINVAL;
  const std::vector<uint32_t> g = mfgpu::multi_groups(n_vectors, std::vector<uint32_t>(widths, widths + n_widths));
  for (size_t i = 0; i < g.size() && i < capacity; ++i) groups[i] = g[i];
  return (int)g.size();
}

int mfgpu_plan_shares_records(const mfgpu_plan *p) {
  return p ? (p->plan.sh_use ? 1 : 0) | (p->plan.sh_p2_use ? 2 : 0) : 0;
}

int64_t mfgpu_plan_lmap(const mfgpu_plan *p, const uint16_t **ptr) {
  if (!p || !ptr) return MFGPU_EINVAL;
  *ptr = p->plan.lmap.data();
  return (int64_t)p->plan.lmap.size();
}

int64_t mfgpu_plan_bflags(const mfgpu_plan *p, const uint8_t **ptr) {
  if (!p || !ptr) return MFGPU_EINVAL;
  *ptr = p->plan.bflags.data();
  return (int64_t)p->plan.bflags.size();
}

}  // extern "C"
