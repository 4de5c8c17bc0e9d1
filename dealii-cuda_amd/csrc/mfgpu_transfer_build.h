// Host-side builder of the multigrid transfers (plain C++, no HIP): from the arrays a caller hands to one of the
// mfgpu_transfer_create* calls to the image that is uploaded as it stands.  The three kinds -- between two refinement
// levels at one degree, between two degrees on one mesh, between two leaf meshes with hanging nodes at one degree -- share
// the checks, the owner rule and THE INDEX FORMAT, which is defined here and read by the kernels of mfgpu_transfer*.hip:
//   coarse list  per coarse cell its dofs; bit 31: a Dirichlet dof of the coarse side (read as 0, never written)
//   fine list    per fine cell (kind H: per coarse cell, the patch of its children) its dofs; bit 31: another cell owns
//                the dof, or the position is a constrained one of a cell with hanging nodes (neither read nor written)
//   words        kind P with masks: per cell its constraint mask.  Kind H_HN: per FINE cell the parent's coarse mask in
//                bits 0..8 and `child` in bits 16..19 (transfer_word)
//   parent       kind H_HN: per fine cell the index of its coarse cell
// Kind H_HN with TransferInput::interpolation also carries the interpolation image (mfgpu_transfer_interpolate):
//   interp_coarse     per coarse cell its dofs; bit 31: another coarse cell owns the dof (the owner rule with the coarse
//                     lists and the COARSE mask), or it is a Dirichlet dof of the coarse side (never written)
//   interp_kids       per coarse cell 2^dim fine cell indices, entry k its child k; an unchanged cell: entry 0 the fine
//                     cell that it is, with bit 31 as the marker, the other entries 0
//   interp_fine_mask  per fine cell its own (fine) constraint mask
//   J1                [(p+1) * (p+1)], row i: the child's basis at the coarse node i (default_interpolation_1d)
// Owner rule: the owner of a fine dof is the first cell, in cell order, that lists it at a position its mask does not
// constrain (no mask: the first that lists it).  Every fine dof is stored by its owner alone and enters a restriction
// through its owner alone.
#ifndef MFGPU_TRANSFER_BUILD_H
#define MFGPU_TRANSFER_BUILD_H

#include <cstddef>
#include <cstdint>
#include <vector>

namespace mfgpu {

enum TransferKind {
  TRANSFER_KIND_H = 0,     // mfgpu_transfer_create: coarse cells and the patches of their children
  TRANSFER_KIND_P = 1,     // mfgpu_transfer_create_p(_hn): degree_coarse -> degree on the same cells
  TRANSFER_KIND_H_HN = 2,  // mfgpu_transfer_create_h_hn: fine leaves, each the same cell as or a child of a coarse leaf
};

constexpr uint32_t kTransferSkip = 0x80000000u;  // bit 31 of an index list entry
constexpr uint32_t transfer_word(uint32_t coarse_mask, uint32_t child) { return coarse_mask | child << 16; }
constexpr uint32_t transfer_word_mask(uint32_t word) { return word & 0x1ffu; }
constexpr uint32_t transfer_word_child(uint32_t word) { return word >> 16; }

// What a creator was given.  Arrays may be null where their count is 0 or the call says so.
struct TransferInput {
  const char *who = "";  // the C-ABI function, for messages
  int kind = TRANSFER_KIND_H, dim = 0, degree = 0, number_type = 0;
  int degree_coarse = 0;  // kind P only
  uint32_t n_coarse_cells = 0, n_fine_cells = 0;  // kinds H and P: one fine list per coarse cell, equal counts
  uint32_t n_coarse_dofs = 0, n_fine_dofs = 0;
  const uint32_t *coarse_cell_dofs = nullptr, *fine_cell_dofs = nullptr;
  const uint32_t *coarse_dirichlet = nullptr;
  uint32_t n_coarse_dirichlet = 0;
  const double *prolongation_1d = nullptr;  // null: the kind's default
  // kind P: the cells' one mask in both; kind H_HN: the two meshes' masks.  Null: no cell has hanging nodes
  const uint32_t *coarse_mask = nullptr, *fine_mask = nullptr;
  const double *constraint_weights = nullptr;  // of the coarse degree; null: FE_Q's
  const uint32_t *parent = nullptr, *child = nullptr;  // kind H_HN
  bool interpolation = false;                // kind H_HN: build the interpolation image too
  const double *interpolation_1d = nullptr;  // null: default_interpolation_1d
};

struct TransferImage {
  int coarse_per_cell = 0, fine_per_cell = 0;  // entries of one cell's lists
  std::vector<uint32_t> coarse, fine, words, parent;
  std::vector<double> P1, W;  // W: empty unless hanging_nodes
  bool hanging_nodes = false;  // the kernels resolve hanging nodes on the coarse side (words and W are present)
  size_t covered = 0;          // the number of fine dofs with an owner
  // the interpolation image; empty unless TransferInput::interpolation
  std::vector<uint32_t> interp_coarse, interp_kids, interp_fine_mask;
  std::vector<double> J1;
  size_t interp_covered = 0;  // the number of coarse dofs that interpolate stores
};

// Validates `in` and fills `img`.  0, or MFGPU_EINVAL with a message that begins with in.who.
int build_transfer_image(const TransferInput &in, TransferImage &img);

bool valid_degree_pair(int degree_coarse, int degree_fine);
// the 9 bits of a constraint mask; in 2D only TYPE x, y and FACE x, y
bool valid_mask(int dim, uint32_t m);
// can resolve_hanging_nodes with mask m write local position t of a cell of n^dim entries?
bool constrained_position(int dim, int n, uint32_t m, int t);
// The owner rule: `out` is the fine list of n_cells cells of n^dim entries each with bit 31 on every entry but the
// owner's.  MFGPU_EINVAL for a bad mask, a dof out of range, and a dof that is listed only at constrained positions: the
// kernels would drop it without a word.
int owner_list(const char *who, int dim, int n, uint32_t n_cells, const uint32_t *fine_cell_dofs, const uint32_t *mask,
               uint32_t n_fine_dofs, uint32_t *out, size_t &covered);
// FE_Q(p) on Gauss-Lobatto nodes: P1[X * (p+1) + x] = phi_x(xi_X), xi_X the 2p+1 child nodes on the parent's [0,1]
void default_prolongation_1d(int p, std::vector<double> &P1);
// P1[X * (pc+1) + x] = phi_x(xi_X): the FE_Q(pc) Lagrange basis on its Gauss-Lobatto nodes at the FE_Q(pf) nodes
void p_prolongation_1d(int pc, int pf, std::vector<double> &P1);
// J1[i * (p+1) + j] = phi_j(2 xi_i - b(i)), b(i) = 0 if xi_i <= 1/2 else 1: the basis of the child that holds the coarse
// node xi_i, at that node.  Rows 0..p/2 belong to the lower child, the others to the upper one
void default_interpolation_1d(int p, std::vector<double> &J1);

}  // namespace mfgpu

#endif
