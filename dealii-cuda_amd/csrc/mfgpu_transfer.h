// The transfer object behind mfgpu_transfer_* (mfgpu_transfer.hip: between two refinement levels at one degree;
// mfgpu_transfer_p.hip: between two degrees on one mesh).  Both kinds share the index layout -- per cell its coarse
// dofs (bit 31: Dirichlet) and its fine dofs (bit 31: another cell owns the dof, or the position is a constrained one of
// a cell with hanging nodes) -- and the three entry points.
#ifndef MFGPU_TRANSFER_H
#define MFGPU_TRANSFER_H

#include <hip/hip_runtime.h>

#include "mfgpu_device.h"

struct mfgpu_transfer {
  int dim = 0, degree = 0, number_type = MFGPU_F64;
  int degree_coarse = 0;  // 0: h-transfer at `degree`; > 0: p-transfer from degree_coarse to `degree` on the same cells
  uint32_t n_coarse_cells = 0, n_coarse_dofs = 0, n_fine_dofs = 0;
  mfgpu::DeviceArray<uint32_t> d_coarse, d_fine;  // h: [cells][(p+1)^dim], [cells][(2p+1)^dim]; p: [cells][(pc+1)^dim], [cells][(pf+1)^dim]
  mfgpu::DeviceArray<void> d_p1;                  // h: P1[(2p+1) * (p+1)]; p: P1[(pf+1) * (pc+1)]; fine index major
  // p-transfer on cells with hanging nodes (mfgpu_transfer_create_p_hn with a mask): the cells' constraint masks and the
  // weight matrix W[(pc+1)^2] of the COARSE degree in number_type; the fine side's constrained positions are plain
  // bit-31 entries of d_fine
  bool hanging_nodes = false;
  mfgpu::DeviceArray<uint32_t> d_mask;
  mfgpu::DeviceArray<void> d_weights;
  bool covers_all = true;                         // every fine dof is listed by some cell
  size_t device_bytes = 0;
};

namespace mfgpu {

enum TransferMode { TRANSFER_PROLONGATE = 0, TRANSFER_PROLONGATE_ADD = 1, TRANSFER_RESTRICT_ADD = 2 };
// the p-transfer's kernel for t->number_type (mfgpu_transfer_p.hip); enqueues only
hipError_t launch_p_transfer(const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, hipStream_t st);

}  // namespace mfgpu

#endif
