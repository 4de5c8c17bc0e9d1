// Host-side builder of the multigrid transfers (mfgpu_transfer_build.h): checks, index format, owner rule, default
// matrices.  Plain C++; mfgpu_transfer.hip uploads what build_transfer_image returns.
#include "mfgpu_transfer_build.h"

#include <cmath>
#include <cstring>
#include <string>

#include "mfgpu_hn_flags.h"
#include "mfgpu_mesh.h"

namespace mfgpu {

namespace {

int refuse(const char *who, const char *what) {
  set_error(std::string(who) + ": " + what);
  return MFGPU_EINVAL;
}

}  // namespace

bool valid_degree_pair(int pc, int pf) { return pc >= 1 && pf <= 6 && pc < pf; }

bool valid_mask(int dim, uint32_t m) { return !(m & ~(dim == 3 ? 0x1ffu : 0x1bu)); }

bool constrained_position(int dim, int n, uint32_t m, int t) {
  bool type;
  int q;
  for (int dir = 0; dir < dim; ++dir)
    if (hn_flag_at(dim, n, m, dir, t, type, q)) return true;
  return false;
}

int owner_list(const char *who, int dim, int n, uint32_t n_cells, const uint32_t *fine_cell_dofs, const uint32_t *mask,
               uint32_t n_fine_dofs, uint32_t *out, size_t &covered) {
  const size_t N = (size_t)ipow(n, dim);
  std::vector<uint8_t> seen(n_fine_dofs, 0);  // 1: listed, 2: owned
  std::vector<uint8_t> con;                   // the constrained positions of the current cell's mask
  uint32_t con_mask = 0;
  covered = 0;
  size_t listed = 0;
  for (uint32_t c = 0; c < n_cells; ++c) {
    const uint32_t m = mask ? mask[c] : 0u;
    if (!valid_mask(dim, m))
      return refuse(who, "a constraint mask has bits outside the defined ones (9 in 3D; TYPE x, y and FACE x, y in 2D)");
    if (m && (con.empty() || m != con_mask)) {
      con.resize(N);
      for (size_t i = 0; i < N; ++i) con[i] = constrained_position(dim, n, m, (int)i);
      con_mask = m;
    }
    for (size_t i = 0; i < N; ++i) {
      const uint32_t g = fine_cell_dofs[c * N + i];
      if (g >= n_fine_dofs) return refuse(who, "fine dof out of range");
      const bool owns = seen[g] < 2 && !(m && con[i]);
      out[c * N + i] = g | (owns ? 0u : kTransferSkip);
      if (!seen[g]) ++listed;
      if (owns) ++covered;
      seen[g] = owns ? 2 : (seen[g] ? seen[g] : 1);
    }
  }
  if (covered != listed)
    return refuse(who, "a fine dof is listed only at constrained positions, so no cell owns it (the masks and "
                       "fine_cell_dofs do not belong together)");
  return 0;
}

void default_prolongation_1d(int p, std::vector<double> &P1) {
  std::vector<double> nodes, val, der;
  gll_01(p, nodes);
  const int nc = p + 1, nf = 2 * p + 1;
  P1.assign((size_t)nf * nc, 0.0);
  for (int X = 0; X < nf; ++X) {
    const double xi = X <= p ? 0.5 * nodes[X] : 0.5 + 0.5 * nodes[X - p];
    lagrange_eval(nodes, xi, val, der);
    for (int x = 0; x < nc; ++x) P1[(size_t)X * nc + x] = val[x];
  }
  // exact zeros / ones where a child node coincides with a parent node
  for (double &v : P1)
    if (std::fabs(v) < 1e-15) v = 0.0;
    else if (std::fabs(v - 1.0) < 1e-15) v = 1.0;
}

void p_prolongation_1d(int pc, int pf, std::vector<double> &P1) {
  std::vector<double> cn, fn, val, der;
  gll_01(pc, cn);
  gll_01(pf, fn);
  const int nc = pc + 1, nf = pf + 1;
  P1.assign((size_t)nf * nc, 0.0);
  for (int X = 0; X < nf; ++X) {
    int same = -1;  // a fine node that is a coarse node (the end points; 1/2 when both degrees are even): exact 0 / 1
    for (int x = 0; x < nc; ++x)
      if (std::fabs(fn[X] - cn[x]) < 1e-14) same = x;
    if (same >= 0) {
      P1[(size_t)X * nc + same] = 1.0;
      continue;
    }
    lagrange_eval(cn, fn[X], val, der);
    for (int x = 0; x < nc; ++x) P1[(size_t)X * nc + x] = val[x];
  }
}

void default_interpolation_1d(int p, std::vector<double> &J1) {
  std::vector<double> nodes, val, der;
  gll_01(p, nodes);
  const int n = p + 1;
  J1.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) {
    const double xi = i <= p / 2 ? 2.0 * nodes[i] : 2.0 * nodes[i] - 1.0;  // the nodes are symmetric: i <= p/2 <=> xi_i <= 1/2
    lagrange_eval(nodes, xi, val, der);
    for (int j = 0; j < n; ++j) J1[(size_t)i * n + j] = val[j];
  }
  // exact zeros / ones where a coarse node is a node of the child (every node at p = 1, 2)
  for (double &v : J1)
    if (std::fabs(v) < 1e-15) v = 0.0;
    else if (std::fabs(v - 1.0) < 1e-15) v = 1.0;
}

namespace {

// the interpolation image of a kind H_HN pair (mfgpu_transfer_build.h), after the rest of the image was checked
int build_interpolation_image(const TransferInput &in, TransferImage &img) {
  const int dim = in.dim, n = in.degree + 1;
  const uint32_t nk = 1u << dim;
  img.interp_kids.assign((size_t)in.n_coarse_cells * nk, 0u);
  std::vector<uint32_t> seen(in.n_coarse_cells, 0u);  // bit k: child k was met; bit 2^dim: the cell itself
  for (uint32_t f = 0; f < in.n_fine_cells; ++f) {
    const uint32_t c = in.parent[f], ch = in.child[f], bit = ch ? 1u << (ch - 1) : 1u << nk;
    if ((seen[c] & bit) || (ch ? seen[c] >> nk : seen[c]) != 0u)
      return refuse(in.who, "a coarse cell is listed as the parent of the same child twice, or both as an unchanged cell "
                            "and as a refined one");
    seen[c] |= bit;
    img.interp_kids[(size_t)c * nk + (ch ? ch - 1 : 0)] = ch ? f : f | kTransferSkip;
  }
  for (uint32_t c = 0; c < in.n_coarse_cells; ++c)
    if (seen[c] != (1u << nk) && seen[c] != (1u << nk) - 1u)
      return refuse(in.who, "a coarse cell is neither one fine cell (child = 0) nor all its 2^dim children: there is "
                            "nothing to interpolate from");
  img.interp_fine_mask.assign(in.n_fine_cells, 0u);
  if (in.fine_mask) img.interp_fine_mask.assign(in.fine_mask, in.fine_mask + in.n_fine_cells);
  img.interp_coarse.resize((size_t)in.n_coarse_cells * img.coarse_per_cell);
  size_t owned;
  if (const int rc = owner_list(in.who, dim, n, in.n_coarse_cells, in.coarse_cell_dofs, in.coarse_mask, in.n_coarse_dofs,
                                img.interp_coarse.data(), owned))
    return rc;
  img.interp_covered = 0;
  for (size_t i = 0; i < img.interp_coarse.size(); ++i) {
    img.interp_coarse[i] |= img.coarse[i] & kTransferSkip;  // the Dirichlet dofs of the coarse side
    if (!(img.interp_coarse[i] >> 31)) ++img.interp_covered;
  }
  if (in.interpolation_1d)
    img.J1.assign(in.interpolation_1d, in.interpolation_1d + (size_t)n * n);
  else
    default_interpolation_1d(in.degree, img.J1);
  return 0;
}

}  // namespace

int build_transfer_image(const TransferInput &in, TransferImage &img) {
  const bool p_kind = in.kind == TRANSFER_KIND_P, h_hn = in.kind == TRANSFER_KIND_H_HN;
  const int dim = in.dim;
  if ((dim != 2 && dim != 3) || (p_kind ? !valid_degree_pair(in.degree_coarse, in.degree) : in.degree < 1 || in.degree > 6) ||
      (in.n_coarse_cells && !in.coarse_cell_dofs) || (in.n_fine_cells && !in.fine_cell_dofs) ||
      (h_hn && in.n_fine_cells && (!in.parent || !in.child)) || (in.n_coarse_dirichlet && !in.coarse_dirichlet) ||
      (in.number_type != MFGPU_F64 && in.number_type != MFGPU_F32) || in.n_coarse_dofs >= (1u << 31) ||
      in.n_fine_dofs >= (1u << 31))
    return refuse(in.who, "bad argument (dim 2 or 3, 1 <= degree <= 6, a p-transfer 1 <= degree_coarse < degree_fine <= 6, "
                          "number type, dof counts < 2^31, arrays)");
  if (in.interpolation && !h_hn)
    return refuse(in.who, "the interpolation image exists for the transfer between two leaf meshes only");
  // entries per direction of a cell's coarse list, of its fine list, and rows of P1
  const int pc = p_kind ? in.degree_coarse : in.degree;
  const int nc = pc + 1, nf = in.kind == TRANSFER_KIND_H ? 2 * in.degree + 1 : in.degree + 1;
  const int p1_rows = p_kind ? nf : 2 * in.degree + 1;
  img.coarse_per_cell = ipow(nc, dim);
  img.fine_per_cell = ipow(nf, dim);

  std::vector<uint8_t> dirichlet(in.n_coarse_dofs, 0);
  for (uint32_t i = 0; i < in.n_coarse_dirichlet; ++i) {
    if (in.coarse_dirichlet[i] >= in.n_coarse_dofs) return refuse(in.who, "Dirichlet dof out of range");
    dirichlet[in.coarse_dirichlet[i]] = 1;
  }
  img.coarse.resize((size_t)in.n_coarse_cells * img.coarse_per_cell);
  for (size_t i = 0; i < img.coarse.size(); ++i) {
    const uint32_t g = in.coarse_cell_dofs[i];
    if (g >= in.n_coarse_dofs) return refuse(in.who, "coarse dof out of range");
    img.coarse[i] = g | (dirichlet[g] ? kTransferSkip : 0u);
  }
  if (h_hn) {
    for (uint32_t c = 0; c < in.n_coarse_cells; ++c)
      if (in.coarse_mask && !valid_mask(dim, in.coarse_mask[c]))
        return refuse(in.who, "a coarse constraint mask has bits outside the defined ones (9 in 3D; TYPE x, y and FACE x, y "
                              "in 2D)");
    img.words.resize(in.n_fine_cells);
    for (uint32_t f = 0; f < in.n_fine_cells; ++f) {
      if (in.parent[f] >= in.n_coarse_cells || in.child[f] > (1u << dim))
        return refuse(in.who, "parent out of range or child > 2^dim");
      img.words[f] = transfer_word(in.coarse_mask ? in.coarse_mask[in.parent[f]] : 0u, in.child[f]);
    }
    img.parent.assign(in.parent, in.parent + in.n_fine_cells);
  } else if (in.coarse_mask) {  // kind P: the cells' own masks, checked by the owner rule
    img.words.assign(in.coarse_mask, in.coarse_mask + in.n_coarse_cells);
  }
  img.fine.resize((size_t)in.n_fine_cells * img.fine_per_cell);
  if (const int rc = owner_list(in.who, dim, nf, in.n_fine_cells, in.fine_cell_dofs, in.fine_mask, in.n_fine_dofs,
                                img.fine.data(), img.covered))
    return rc;

  if (in.prolongation_1d)
    img.P1.assign(in.prolongation_1d, in.prolongation_1d + (size_t)p1_rows * nc);
  else if (p_kind)
    p_prolongation_1d(pc, in.degree, img.P1);
  else
    default_prolongation_1d(in.degree, img.P1);
  img.hanging_nodes = h_hn || in.coarse_mask;
  if (img.hanging_nodes && in.constraint_weights)
    img.W.assign(in.constraint_weights, in.constraint_weights + (size_t)nc * nc);
  else if (img.hanging_nodes)
    fe_q_constraint_weights(pc, img.W);
  return in.interpolation ? build_interpolation_image(in, img) : 0;
}

}  // namespace mfgpu

extern "C" {

int mfgpu_transfer_p_prolongation_1d(int degree_coarse, int degree_fine, double *p1) {
  using namespace mfgpu;
  if (!p1 || !valid_degree_pair(degree_coarse, degree_fine))
    return refuse("mfgpu_transfer_p_prolongation_1d", "needs 1 <= degree_coarse < degree_fine <= 6 and an output array");
  std::vector<double> P1;
  p_prolongation_1d(degree_coarse, degree_fine, P1);
  std::memcpy(p1, P1.data(), P1.size() * sizeof(double));
  return 0;
}

int mfgpu_transfer_p_owner_list(int dim, int degree_fine, uint32_t n_cells, const uint32_t *fine_cell_dofs,
                                const uint32_t *constraint_mask, uint32_t n_fine_dofs, uint32_t *out) {
  using namespace mfgpu;
  const char *who = "mfgpu_transfer_p_owner_list";
  if ((dim != 2 && dim != 3) || degree_fine < 1 || degree_fine > 6 || (n_cells && (!fine_cell_dofs || !out)) ||
      n_fine_dofs >= (1u << 31))
    return refuse(who, "bad argument (1 <= degree_fine <= 6, dim 2 or 3, dof count < 2^31, arrays)");
  size_t covered;
  return owner_list(who, dim, degree_fine + 1, n_cells, fine_cell_dofs, constraint_mask, n_fine_dofs, out, covered);
}

}  // extern "C"
