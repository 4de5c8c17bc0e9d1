// Level operator of a multigrid hierarchy with refinement edges: LaplaceOperatorGpu::reinit(dof_handler,
// mg_constrained_dofs, level) and the interface ("edge") matrices vmult_interface_down / vmult_interface_up
// (reference laplace_operator_gpu.h:154-186, 306-352) that deal.II's Multigrid applies on adaptively refined meshes
// (mg.set_edge_matrices, poisson_mg.cu:375).
//
// The reference keeps ONE matrix-free structure per level without constraints and brackets its cell loop with index
// kernels of ConstraintHandlerGpu (save / zero / copy_edge_values / load).  Here the operator fuses its constrained
// rows into the cell loop, so a level holds two operators over the same level mesh:
//   A  : constrained rows = the level's Dirichlet dofs AND its refinement-edge dofs (what vmult / the smoother see)
//   Ab : K itself, NO constrained rows -- the reference's cell loop runs on a structure without constraints (:174-176)
//        (built only if the level has edge dofs)
// and the interface matrices are compositions (C = Dirichlet + edge, E = edge):
//   down: dst = 0 except dst[E] = (K (src with C zeroed))[E]                                          (:306-330)
//   up  : dst = K (src restricted to E), then dst[C] = 0                                              (:332-352)
// An edge dof may also be a Dirichlet dof (a refinement edge that reaches the domain boundary): down then returns
// (K x)[E] on it and up includes src[E] there, as the reference does; identity rows in Ab would lose both.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "mfgpu_device.h"
#include "mfgpu_kernels.h"

using namespace mfgpu;

struct mfgpu_level {
  mfgpu_handle *A = nullptr, *Ab = nullptr;
  DeviceArray<uint32_t> d_c, d_e;  // C = Dirichlet + edge, E = edge (device index lists)
  uint32_t n_c = 0, n_e = 0, n_dofs = 0;
  int number_type = MFGPU_F64;
  DeviceArray<void> tmp_x, tmp_y;
};

// index pairs on the device: copy_to_mg / copy_from_mg (mg_transfer_matrix_free_gpu.cu:690-760, copy_indices)
struct mfgpu_index_pairs {
  DeviceArray<uint32_t> d_dst, d_src;
  uint32_t n = 0;
};

namespace {

template <typename T>
__global__ void copy_pairs_kernel(T *dst, const T *src, const uint32_t *di, const uint32_t *si, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[di[i]] = src[si[i]];
}

// copy_to_mg / copy_from_mg across number types (deal.II's OtherNumber): dst[di[i]] = (D) src[si[i]]
template <typename D, typename S>
__global__ void __launch_bounds__(256)
copy_pairs_convert_kernel(D *dst, const S *src, const uint32_t *di, const uint32_t *si, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[di[i]] = (D)src[si[i]];
}

template <typename T>
__global__ void set_indexed_kernel(T *v, const uint32_t *idx, uint32_t n, T value) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[idx[i]] = value;
}
template <typename T>
__global__ void copy_indexed_kernel(T *dst, const T *src, const uint32_t *idx, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[idx[i]] = src[idx[i]];
}

template <typename T>
int interface_typed(mfgpu_level *L, bool down, T *dst, const T *src, hipStream_t st) {
  // The zero fills are fill_launch, not hipMemsetAsync: with the HIP runtime this was written against, a captured memset
  // node zeroes its target on the first replay of a graph only and leaves stale bytes there from the second replay on
  // (tests/test_gpu_streams.py, the replayed level cases); a kernel node replays like every other launch of the call
  const size_t bytes = (size_t)L->n_dofs * sizeof(T);
  T *x = L->tmp_x.as<T>(), *y = L->tmp_y.as<T>();
  const uint32_t *c = L->d_c.get(), *e = L->d_e.get();
  const unsigned gc = (L->n_c + 255) / 256, ge = (L->n_e + 255) / 256;
  if (L->n_e == 0) {  // no refinement edge on this level: both matrices are zero
    HIP_TRY(fill_launch<T>(dst, L->n_dofs, T(0), st));
    return 0;
  }
  if (down) {
    // x = src with C zeroed (constraint_handler.save_constrained_values, :315); y = K x; dst = 0, dst[E] = y[E]
    HIP_TRY(hipMemcpyAsync(x, src, bytes, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(set_indexed_kernel<T>, dim3(gc), dim3(256), 0, st, x, c, L->n_c, T(0));
    if (const int rc = mfgpu_vmult(L->Ab, y, x, st)) return rc;
    HIP_TRY(fill_launch<T>(dst, L->n_dofs, T(0), st));
    hipLaunchKernelGGL(copy_indexed_kernel<T>, dim3(ge), dim3(256), 0, st, dst, (const T *)y, e, L->n_e);
  } else {
    // x = 0 except the edge values of src (copy_edge_values, :343); dst = K x; dst[C] = 0 (:351)
    HIP_TRY(fill_launch<T>(x, L->n_dofs, T(0), st));
    hipLaunchKernelGGL(copy_indexed_kernel<T>, dim3(ge), dim3(256), 0, st, x, src, e, L->n_e);
    if (const int rc = mfgpu_vmult(L->Ab, dst, x, st)) return rc;
    hipLaunchKernelGGL(set_indexed_kernel<T>, dim3(gc), dim3(256), 0, st, dst, c, L->n_c, T(0));
  }
  return hip_check(hipGetLastError(), "level interface kernels");
}

}  // namespace

extern "C" {

int mfgpu_level_create(const mfgpu_desc *desc, const uint32_t *edge_dofs, uint32_t n_edge, mfgpu_level **out) {
  if (!desc || !out || (n_edge && !edge_dofs)) {
    set_error("mfgpu_level_create: null argument");
    return MFGPU_EINVAL;
  }
  if (desc->flags & MFGPU_HANGING_NODES) {
    set_error("mfgpu_level_create: level meshes have no hanging nodes (laplace_operator_gpu.h:174-176)");
    return MFGPU_EINVAL;
  }
  std::vector<uint32_t> e(edge_dofs, edge_dofs + n_edge), c(desc->constrained_dofs, desc->constrained_dofs + desc->n_constrained);
  for (uint32_t g : e)
    if (g >= desc->n_dofs) {
      set_error("mfgpu_level_create: edge dof out of range");
      return MFGPU_EINVAL;
    }
  std::sort(e.begin(), e.end());
  e.erase(std::unique(e.begin(), e.end()), e.end());
  c.insert(c.end(), e.begin(), e.end());
  std::sort(c.begin(), c.end());
  c.erase(std::unique(c.begin(), c.end()), c.end());
  std::unique_ptr<mfgpu_level, decltype(&mfgpu_level_destroy)> L(new mfgpu_level(), mfgpu_level_destroy);
  L->n_dofs = desc->n_dofs;
  L->number_type = desc->number_type;
  L->n_e = (uint32_t)e.size();
  L->n_c = (uint32_t)c.size();
  mfgpu_desc da = *desc;
  da.constrained_dofs = c.data();
  da.n_constrained = (uint32_t)c.size();
  int rc = mfgpu_create(&da, &L->A);
  if (rc) return rc;
  if (L->n_e) {
    mfgpu_desc db = *desc;
    db.constrained_dofs = nullptr;
    db.n_constrained = 0;
    if ((rc = mfgpu_create(&db, &L->Ab))) return rc;
    const size_t vec_bytes = (size_t)L->n_dofs * esize(desc->number_type);
    if ((rc = L->d_c.upload(c.data(), c.size())) || (rc = L->d_e.upload(e.data(), e.size())) ||
        (rc = L->tmp_x.alloc(vec_bytes)) || (rc = L->tmp_y.alloc(vec_bytes)))
      return rc;
  }
  *out = L.release();
  return 0;
}

mfgpu_handle *mfgpu_level_operator(mfgpu_level *L) { return L ? L->A : nullptr; }

int mfgpu_level_update_coefficients(mfgpu_level *L, const void *coefficient_dev, const void *mass_coefficient_dev,
                                    void *stream) {
  if (!L) {
    set_error("mfgpu_level_update_coefficients: null argument");
    return MFGPU_EINVAL;
  }
  // A first: it refuses what Ab (made from a copy of the same description) would refuse, before anything is written
  if (const int rc = mfgpu_update_coefficients(L->A, coefficient_dev, mass_coefficient_dev, stream)) return rc;
  return L->Ab ? mfgpu_update_coefficients(L->Ab, coefficient_dev, mass_coefficient_dev, stream) : 0;
}

int mfgpu_level_vmult_interface_down(mfgpu_level *L, void *dst, const void *src, void *stream) {
  if (!L || !dst || !src || dst == src) {
    set_error("mfgpu_level_vmult_interface_down: null or aliasing argument");
    return MFGPU_EINVAL;
  }
  return L->number_type == MFGPU_F64 ? interface_typed<double>(L, true, (double *)dst, (const double *)src, (hipStream_t)stream)
                                     : interface_typed<float>(L, true, (float *)dst, (const float *)src, (hipStream_t)stream);
}

int mfgpu_level_vmult_interface_up(mfgpu_level *L, void *dst, const void *src, void *stream) {
  if (!L || !dst || !src || dst == src) {
    set_error("mfgpu_level_vmult_interface_up: null or aliasing argument");
    return MFGPU_EINVAL;
  }
  return L->number_type == MFGPU_F64 ? interface_typed<double>(L, false, (double *)dst, (const double *)src, (hipStream_t)stream)
                                     : interface_typed<float>(L, false, (float *)dst, (const float *)src, (hipStream_t)stream);
}

int mfgpu_index_pairs_create(const uint32_t *dst_idx, const uint32_t *src_idx, uint32_t n, mfgpu_index_pairs **out) {
  if (!out || (n && (!dst_idx || !src_idx))) {
    set_error("mfgpu_index_pairs_create: null argument");
    return MFGPU_EINVAL;
  }
  std::unique_ptr<mfgpu_index_pairs> p(new mfgpu_index_pairs());
  p->n = n;
  int rc;
  if ((rc = p->d_dst.upload(dst_idx, n)) || (rc = p->d_src.upload(src_idx, n))) return rc;
  *out = p.release();
  return 0;
}

int mfgpu_vec_copy_pairs(const mfgpu_index_pairs *p, void *dst, const void *src, int number_type, void *stream) {
  if (!p || !dst || !src) {
    set_error("mfgpu_vec_copy_pairs: null argument");
    return MFGPU_EINVAL;
  }
  if (p->n == 0) return 0;
  const unsigned grid = (p->n + 255) / 256;
  if (number_type == MFGPU_F64)
    hipLaunchKernelGGL(copy_pairs_kernel<double>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (double *)dst,
                       (const double *)src, p->d_dst.get(), p->d_src.get(), p->n);
  else
    hipLaunchKernelGGL(copy_pairs_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (float *)dst,
                       (const float *)src, p->d_dst.get(), p->d_src.get(), p->n);
  return hip_check(hipGetLastError(), "copy_pairs_kernel");
}

int mfgpu_vec_copy_pairs_convert(const mfgpu_index_pairs *p, void *dst, int dst_type, const void *src, int src_type,
                                 void *stream) {
  if (!valid_number_type(dst_type) || !valid_number_type(src_type)) {
    set_error("mfgpu_vec_copy_pairs_convert: number type must be MFGPU_F64 or MFGPU_F32");
    return MFGPU_EINVAL;
  }
  if (!p || !dst || !src) {
    set_error("mfgpu_vec_copy_pairs_convert: null argument");
    return MFGPU_EINVAL;
  }
  if (p->n == 0) return 0;
  const unsigned grid = (p->n + 255) / 256;
  const hipStream_t st = (hipStream_t)stream;
#define CPC(D, S)                                                                                                  \
  hipLaunchKernelGGL((copy_pairs_convert_kernel<D, S>), dim3(grid), dim3(256), 0, st, (D *)dst, (const S *)src, \
                     p->d_dst.get(), p->d_src.get(), p->n)
  if (dst_type == MFGPU_F64 && src_type == MFGPU_F64)
    CPC(double, double);
  else if (dst_type == MFGPU_F64)
    CPC(double, float);
  else if (src_type == MFGPU_F64)
    CPC(float, double);
  else
    CPC(float, float);
#undef CPC
  return hip_check(hipGetLastError(), "copy_pairs_convert_kernel");
}

void mfgpu_index_pairs_destroy(mfgpu_index_pairs *p) { delete p; }

void mfgpu_level_destroy(mfgpu_level *L) {
  if (!L) return;
  mfgpu_destroy(L->A);
  mfgpu_destroy(L->Ab);
  delete L;
}

}  // extern "C"
