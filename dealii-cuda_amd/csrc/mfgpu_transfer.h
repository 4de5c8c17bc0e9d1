// The transfer object behind mfgpu_transfer_* and what its three kernel files share on the host: the modes of the one
// entry path and the dispatch on them (mfgpu_transfer.hip: creators, entry points and the kernel between two refinement
// levels at one degree; mfgpu_transfer_p.hip: between two degrees on one mesh; mfgpu_transfer_h.hip: between two leaf
// meshes with hanging nodes at one degree).  The device arrays are a TransferImage as uploaded: the index format and the
// owner rule are mfgpu_transfer_build.h's.
#ifndef MFGPU_TRANSFER_H
#define MFGPU_TRANSFER_H

#include <hip/hip_runtime.h>

#include <type_traits>

#include "mfgpu_device.h"
#include "mfgpu_transfer_build.h"

struct mfgpu_transfer {
  int kind = mfgpu::TRANSFER_KIND_H;
  int dim = 0, degree = 0, number_type = MFGPU_F64;
  int degree_coarse = 0;  // kind P: the coarse degree; otherwise 0
  uint32_t n_coarse_cells = 0, n_coarse_dofs = 0, n_fine_dofs = 0;
  // h: [cells][(p+1)^dim], [cells][(2p+1)^dim]; p: [cells][(pc+1)^dim], [cells][(pf+1)^dim];
  // h_hn: [coarse cells][(p+1)^dim], [fine cells][(p+1)^dim]
  mfgpu::DeviceArray<uint32_t> d_coarse, d_fine;
  mfgpu::DeviceArray<void> d_p1;  // h, h_hn: P1[(2p+1) * (p+1)]; p: P1[(pf+1) * (pc+1)]; fine index major
  // hanging_nodes (p with a mask, h_hn): TransferImage::words and the weight matrix W of the COARSE degree in number_type
  bool hanging_nodes = false;
  mfgpu::DeviceArray<uint32_t> d_mask;
  mfgpu::DeviceArray<void> d_weights;
  uint32_t n_fine_cells = 0;               // the fine lists' count (h, p: n_coarse_cells)
  mfgpu::DeviceArray<uint32_t> d_parent;   // h_hn only: the index of each fine cell's coarse cell
  bool covers_all = true;  // every fine dof is listed by some cell
  // the interpolation image (h_hn from an _interp creator only; TransferImage::interp_*): the coarse list with owner
  // marking, the fine cells of each coarse cell, the fine masks, J1[(p+1)^2] in number_type
  bool interpolation = false;
  bool interp_covers_all = true;  // interpolate stores every coarse dof
  mfgpu::DeviceArray<uint32_t> d_interp_coarse, d_interp_kids, d_interp_fine_mask;
  mfgpu::DeviceArray<void> d_j1;
  size_t device_bytes = 0;
};

namespace mfgpu {

constexpr int ipow_c(int a, int e) { return e == 0 ? 1 : a * ipow_c(a, e - 1); }

enum TransferMode { TRANSFER_PROLONGATE = 0, TRANSFER_PROLONGATE_ADD = 1, TRANSFER_RESTRICT_ADD = 2 };

// f(RESTRICT, ADD) with the mode's two kernel template arguments as std::integral_constants
template <typename F>
hipError_t dispatch_mode(TransferMode mode, F f) {
  switch (mode) {
    case TRANSFER_PROLONGATE: return f(std::false_type(), std::false_type());
    case TRANSFER_PROLONGATE_ADD: return f(std::false_type(), std::true_type());
    case TRANSFER_RESTRICT_ADD: return f(std::true_type(), std::false_type());
  }
  return hipErrorInvalidValue;
}
// f(dim, degree) as std::integral_constants for dim 2, 3 and degree MIN_DEGREE..6
template <int MIN_DEGREE, typename F>
hipError_t dispatch_dim_degree(int dim, int degree, F f) {
#define MFGPU_TR_CASE(D, P)                                                                      \
  case D * 10 + P:                                                                               \
    if constexpr (P >= MIN_DEGREE) return f(std::integral_constant<int, D>(), std::integral_constant<int, P>()); \
    break;
  switch (dim * 10 + degree) {
    MFGPU_TR_CASE(2, 1) MFGPU_TR_CASE(2, 2) MFGPU_TR_CASE(2, 3) MFGPU_TR_CASE(2, 4) MFGPU_TR_CASE(2, 5) MFGPU_TR_CASE(2, 6)
    MFGPU_TR_CASE(3, 1) MFGPU_TR_CASE(3, 2) MFGPU_TR_CASE(3, 3) MFGPU_TR_CASE(3, 4) MFGPU_TR_CASE(3, 5) MFGPU_TR_CASE(3, 6)
  }
#undef MFGPU_TR_CASE
  return hipErrorInvalidValue;
}

// f(dim, degree, RESTRICT, ADD): the template arguments of t's kernel for a mode
template <int MIN_DEGREE, typename F>
hipError_t dispatch_kernel(const mfgpu_transfer *t, TransferMode mode, F f) {
  return dispatch_mode(mode, [&](auto restrict_, auto add) {
    return dispatch_dim_degree<MIN_DEGREE>(t->dim, t->degree, [&](auto dim, auto degree) {
      return f(dim, degree, decltype(restrict_)(), decltype(add)());
    });
  });
}

// The wave-per-cell kernels of t for number type T (HN: on cells with hanging nodes); each enqueues only.  Defined and
// instantiated for double and float in mfgpu_transfer_p.hip and mfgpu_transfer_h.hip.
template <typename T, bool HN>
hipError_t launch_p_transfer(const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, hipStream_t st);
template <typename T>
hipError_t launch_h_hn_transfer(const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, hipStream_t st);
// mfgpu_transfer_interpolate of an h_hn object with the interpolation image (mfgpu_transfer_h.hip)
template <typename T>
hipError_t launch_h_hn_interpolate(const mfgpu_transfer *t, void *dst, const void *src, hipStream_t st);

}  // namespace mfgpu

#endif
