// The transfer object behind mfgpu_transfer_* (mfgpu_transfer.hip: between two refinement levels at one degree;
// mfgpu_transfer_p.hip: between two degrees on one mesh; mfgpu_transfer_h.hip: between two leaf meshes with hanging
// nodes at one degree).  All kinds share the index layout -- per cell its coarse dofs (bit 31: Dirichlet) and its fine
// dofs (bit 31: another cell owns the dof, or the position is a constrained one of a cell with hanging nodes) -- and the
// three entry points, which dispatch on `kind`.
#ifndef MFGPU_TRANSFER_H
#define MFGPU_TRANSFER_H

#include <hip/hip_runtime.h>

#include "mfgpu_device.h"

namespace mfgpu {
enum TransferKind {
  TRANSFER_KIND_H = 0,     // mfgpu_transfer_create: coarse cells and the patches of their children
  TRANSFER_KIND_P = 1,     // mfgpu_transfer_create_p(_hn): degree_coarse -> degree on the same cells
  TRANSFER_KIND_H_HN = 2,  // mfgpu_transfer_create_h_hn: fine leaves, each the same cell as or a child of a coarse leaf
};
}

struct mfgpu_transfer {
  int kind = mfgpu::TRANSFER_KIND_H;
  int dim = 0, degree = 0, number_type = MFGPU_F64;
  int degree_coarse = 0;  // kind P: the coarse degree; otherwise 0
  uint32_t n_coarse_cells = 0, n_coarse_dofs = 0, n_fine_dofs = 0;
  // h: [cells][(p+1)^dim], [cells][(2p+1)^dim]; p: [cells][(pc+1)^dim], [cells][(pf+1)^dim];
  // h_hn: [coarse cells][(p+1)^dim], [fine cells][(p+1)^dim]
  mfgpu::DeviceArray<uint32_t> d_coarse, d_fine;
  mfgpu::DeviceArray<void> d_p1;  // h, h_hn: P1[(2p+1) * (p+1)]; p: P1[(pf+1) * (pc+1)]; fine index major
  // p-transfer on cells with hanging nodes (mfgpu_transfer_create_p_hn with a mask): the cells' constraint masks and the
  // weight matrix W[(pc+1)^2] of the COARSE degree in number_type; the fine side's constrained positions are plain
  // bit-31 entries of d_fine.  h_hn: d_weights is W[(p+1)^2] and d_mask holds one word per FINE cell, the parent's
  // coarse mask in bits 0..8 and `child` in bits 16..19
  bool hanging_nodes = false;
  mfgpu::DeviceArray<uint32_t> d_mask;
  mfgpu::DeviceArray<void> d_weights;
  // h_hn only: the fine cells' count and the index of each one's coarse cell
  uint32_t n_fine_cells = 0;
  mfgpu::DeviceArray<uint32_t> d_parent;
  bool covers_all = true;                         // every fine dof is listed by some cell
  size_t device_bytes = 0;
};

namespace mfgpu {

enum TransferMode { TRANSFER_PROLONGATE = 0, TRANSFER_PROLONGATE_ADD = 1, TRANSFER_RESTRICT_ADD = 2 };
// the p-transfer's kernel for t->number_type (mfgpu_transfer_p.hip); enqueues only
hipError_t launch_p_transfer(const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, hipStream_t st);
// the same for the h-transfer between two leaf meshes (mfgpu_transfer_h.hip)
hipError_t launch_h_hn_transfer(const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, hipStream_t st);

// (mfgpu_transfer_p.hip) the 9 bits of a constraint mask; in 2D only TYPE x, y and FACE x, y
bool valid_mask(int dim, uint32_t m);
// (mfgpu_transfer_p.hip) the fine index list as it is uploaded, bit 31 on every entry but the owner's; `covered` = the
// number of fine dofs with an owner; MFGPU_EINVAL for a bad mask, a dof out of range, a listed dof nobody owns
int p_owner_list(const char *who, int dim, int degree_fine, uint32_t n_cells, const uint32_t *fine_cell_dofs,
                 const uint32_t *mask, uint32_t n_fine_dofs, uint32_t *out, size_t &covered);

}  // namespace mfgpu

#endif
