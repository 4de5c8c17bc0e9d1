// Multigrid level transfer: MGTransferMatrixFreeGpu::prolongate / restrict_and_add
// (reference matrix_free_gpu/mg_transfer_matrix_free_gpu.cu:391-660) between two globally refined levels.
//
// Semantics (what the reference's weighted, atomically accumulated cell loops add up to):
//   prolongate        dst_fine    = P (src_coarse with the coarse level's Dirichlet dofs read as 0)        (:595-627)
//   restrict_and_add  dst_coarse += Z P^T src_fine,  Z = zero on the coarse level's Dirichlet dofs          (:631-660)
// with P the embedding of the coarse FE space into the fine one: per coarse cell the tensor product of the 1D
// matrix P1[(2p+1) x (p+1)] (the coarse cell's 1D basis at the 2p+1 nodes of its two children).
//
// Re-design for one pass each and no scratch vectors:
//  * every fine dof has ONE owner patch (the first coarse cell whose children list it; bit 31 of a fine patch entry
//    marks "not the owner").  Prolongation is consistent across patches (the spaces are conforming), so the owner
//    alone stores the value with a plain store: no dst = 0 pass, no 3^dim weights, no atomics (reference: :417-435,
//    :375-386).  Restriction counts every fine dof once for the same reason: non-owned entries read as 0.
//  * Dirichlet dofs of the coarse level are flagged in the coarse cell's dof list (bit 31): read as 0 in
//    prolongate (no src copy + set_mg_constrained_dofs, :607-608), skipped in restrict (no increment vector, :642-657).
//  * restriction accumulates into the coarse vector with hardware floating-point atomics (several coarse cells share
//    a coarse dof), as the reference does; prolongation is deterministic.
//  * prolongate_add (dst_fine += P src_coarse, the V-cycle's coarse-grid correction) is the prolongation kernel with the
//    ADD flag: the owner's plain store becomes a plain read-modify-write.  One owner per fine dof, so still no atomics,
//    and a transfer that does not cover the fine level simply leaves the other entries alone (no zero pass).
// One 256-thread workgroup per coarse cell at a time (grid-stride); the three 1D contractions go through LDS.
// Bound: HBM (one read of the fine vector + index lists); small next to the smoother's operator applies.
// The same object and entry points also serve the transfer between two DEGREES on one mesh (p-multigrid; kernels in
// mfgpu_transfer_p.hip, one wave per cell) and the transfer between two leaf meshes with hanging nodes (global
// coarsening; kernels in mfgpu_transfer_h.hip).  All creators are here: each describes what it was given as a
// TransferInput, build_transfer_image (mfgpu_transfer_build.cpp, plain C++) checks it and makes the host image, and
// upload_transfer turns the image into the object.  The three entry points go through launch_transfer; the fourth,
// mfgpu_transfer_interpolate, exists for leaf-mesh objects made with the interpolation image (interpolate_transfer).
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "mfgpu_device.h"
#include "mfgpu_mesh.h"
#include "mfgpu_transfer.h"

namespace mfgpu {

namespace {

// sizes of the intermediate arrays: after contracting directions 0..k-1 the array is nf^k x nc^(dim-k)
template <int dim, int p, typename T, bool RESTRICT, bool ADD>
__global__ void __launch_bounds__(256)
transfer_kernel(T *__restrict__ dst, const T *__restrict__ src, const uint32_t *__restrict__ coarse,
                const uint32_t *__restrict__ fine, const T *__restrict__ p1, uint32_t n_cells) {
  constexpr int nc = p + 1, nf = 2 * p + 1;
  constexpr int NC = ipow_c(nc, dim), NF = ipow_c(nf, dim);
  __shared__ T A[NF], B[NF], P[nf * nc];
  const int tid = threadIdx.x;
  for (int t = tid; t < nf * nc; t += 256) P[t] = p1[t];
  for (uint32_t cell = blockIdx.x; cell < n_cells; cell += gridDim.x) {
    const uint32_t *cd = coarse + (size_t)cell * NC, *fd = fine + (size_t)cell * NF;
    __syncthreads();
    if (!RESTRICT) {
      for (int t = tid; t < NC; t += 256) {
        const uint32_t g = cd[t];
        A[t] = (g >> 31) ? T(0) : src[g];  // set_mg_constrained_dofs(src, to_level - 1, 0), :607-608
      }
    } else {
      for (int t = tid; t < NF; t += 256) {
        const uint32_t g = fd[t];
        A[t] = (g >> 31) ? T(0) : src[g];  // a fine dof enters through its owner patch only
      }
    }
    __syncthreads();
    T *in = A, *out = B;
#pragma unroll
    for (int k = 0; k < dim; ++k) {
      // prolongate: direction k goes nc -> nf; directions < k are already nf long, directions > k still nc
      // restrict  : direction k goes nf -> nc; directions < k are already nc long, directions > k still nf
      const int lo = RESTRICT ? ipow_c(nc, k) : ipow_c(nf, k);            // product of the sizes below k
      const int hi = RESTRICT ? ipow_c(nf, dim - 1 - k) : ipow_c(nc, dim - 1 - k);  // ... above k
      const int n_in = RESTRICT ? nf : nc, n_out = RESTRICT ? nc : nf;
      const int total = lo * n_out * hi;
      for (int t = tid; t < total; t += 256) {
        const int a = t % lo, o = (t / lo) % n_out, b = t / (lo * n_out);
        const T *v = in + a + (size_t)b * lo * n_in;
        T s = T(0);
        for (int i = 0; i < n_in; ++i) s += (RESTRICT ? P[i * nc + o] : P[o * nc + i]) * v[i * lo];
        out[t] = s;
      }
      __syncthreads();
      T *tmp = in;
      in = out;
      out = tmp;
    }
    if (!RESTRICT) {
      for (int t = tid; t < NF; t += 256) {
        const uint32_t g = fd[t];
        if (!(g >> 31)) dst[g] = ADD ? dst[g] + in[t] : in[t];
      }
    } else {
      for (int t = tid; t < NC; t += 256) {
        const uint32_t g = cd[t];
        if (!(g >> 31)) atomicAdd(dst + g, in[t]);  // several coarse cells share the dof (:515-519)
      }
    }
  }
}

template <typename T>
hipError_t launch_level_transfer(const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, hipStream_t st) {
  const uint32_t n = t->n_coarse_cells;
  if (n == 0) return hipSuccess;
  const unsigned grid = n < 8192u ? n : 8192u;
  return dispatch_kernel<1>(t, mode, [&](auto D, auto P, auto R, auto A) {
    hipLaunchKernelGGL((transfer_kernel<D(), P(), T, R(), A()>), dim3(grid), dim3(256), 0, st, (T *)dst, (const T *)src,
                       t->d_coarse.get(), t->d_fine.get(), t->d_p1.as<const T>(), n);
    return hipGetLastError();
  });
}

template <typename T>
__global__ void zero_kernel(T *v, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) v[i] = T(0);
}

// the image as device arrays: P1 and W in number_type, every array that is present, device_bytes their sum
int upload_transfer(const TransferInput &in, const TransferImage &img, mfgpu_transfer **out) {
  std::unique_ptr<mfgpu_transfer> t(new mfgpu_transfer());
  t->kind = in.kind;
  t->dim = in.dim;
  t->degree = in.degree;
  t->degree_coarse = in.kind == TRANSFER_KIND_P ? in.degree_coarse : 0;
  t->number_type = in.number_type;
  t->n_coarse_cells = in.n_coarse_cells;
  t->n_fine_cells = in.n_fine_cells;
  t->n_coarse_dofs = in.n_coarse_dofs;
  t->n_fine_dofs = in.n_fine_dofs;
  t->hanging_nodes = img.hanging_nodes;
  t->covers_all = img.covered == in.n_fine_dofs;
  t->interpolation = in.interpolation;
  t->interp_covers_all = img.interp_covered == in.n_coarse_dofs;
  auto upload_numbers = [&](DeviceArray<void> &d, const std::vector<double> &v) {
    if (in.number_type == MFGPU_F64) return d.upload(v.data(), v.size() * sizeof(double));
    const std::vector<float> f(v.begin(), v.end());
    return d.upload(f.data(), f.size() * sizeof(float));
  };
  int rc;
  if ((rc = t->d_coarse.upload(img.coarse.data(), img.coarse.size())) || (rc = t->d_fine.upload(img.fine.data(), img.fine.size())) ||
      (rc = t->d_parent.upload(img.parent.data(), img.parent.size())) || (rc = t->d_mask.upload(img.words.data(), img.words.size())) ||
      (rc = upload_numbers(t->d_p1, img.P1)) || (rc = upload_numbers(t->d_weights, img.W)))
    return rc;
  t->device_bytes = t->d_coarse.bytes() + t->d_fine.bytes() + t->d_parent.bytes() + t->d_mask.bytes() + t->d_p1.bytes() +
                    t->d_weights.bytes();
  if (in.interpolation) {  // the interpolation image; an object without it uploads and counts nothing more
    if ((rc = t->d_interp_coarse.upload(img.interp_coarse.data(), img.interp_coarse.size())) ||
        (rc = t->d_interp_kids.upload(img.interp_kids.data(), img.interp_kids.size())) ||
        (rc = t->d_interp_fine_mask.upload(img.interp_fine_mask.data(), img.interp_fine_mask.size())) ||
        (rc = upload_numbers(t->d_j1, img.J1)))
      return rc;
    t->device_bytes += t->d_interp_coarse.bytes() + t->d_interp_kids.bytes() + t->d_interp_fine_mask.bytes() + t->d_j1.bytes();
  }
  *out = t.release();
  return 0;
}

int create_transfer(const TransferInput &in, mfgpu_transfer **out) {
  if (!out) {
    set_error(std::string(in.who) + ": bad argument (null out)");
    return MFGPU_EINVAL;
  }
  TransferImage img;
  if (const int rc = build_transfer_image(in, img)) return rc;
  return upload_transfer(in, img, out);
}

hipError_t launch_transfer(const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, hipStream_t st) {
  const bool f64 = t->number_type == MFGPU_F64;
  switch (t->kind) {
    case TRANSFER_KIND_H:
      return f64 ? launch_level_transfer<double>(t, dst, src, mode, st) : launch_level_transfer<float>(t, dst, src, mode, st);
    case TRANSFER_KIND_P:
      if (t->hanging_nodes)
        return f64 ? launch_p_transfer<double, true>(t, dst, src, mode, st) : launch_p_transfer<float, true>(t, dst, src, mode, st);
      return f64 ? launch_p_transfer<double, false>(t, dst, src, mode, st) : launch_p_transfer<float, false>(t, dst, src, mode, st);
    case TRANSFER_KIND_H_HN:
      return f64 ? launch_h_hn_transfer<double>(t, dst, src, mode, st) : launch_h_hn_transfer<float>(t, dst, src, mode, st);
  }
  return hipErrorInvalidValue;
}

// the three entry points; `who` is the C-ABI function.  A prolongation that does not cover the fine side zeroes dst first
// (a kernel on the caller's stream, so that a captured graph holds kernel nodes only)
int apply_transfer(const char *who, const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, void *stream) {
  if (!t || !dst || !src) {
    set_error(std::string(who) + ": null argument");
    return MFGPU_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  if (mode == TRANSFER_PROLONGATE && !t->covers_all) {
    if (t->number_type == MFGPU_F64)
      hipLaunchKernelGGL(zero_kernel<double>, dim3(2048), dim3(256), 0, st, (double *)dst, (size_t)t->n_fine_dofs);
    else
      hipLaunchKernelGGL(zero_kernel<float>, dim3(2048), dim3(256), 0, st, (float *)dst, (size_t)t->n_fine_dofs);
  }
  HIP_TRY(launch_transfer(t, dst, src, mode, st));
  return 0;
}

// mfgpu_transfer_interpolate of an object with the image.  Coarse Dirichlet dofs and dofs that no coarse cell owns are
// stored by nobody: dst is zeroed first, by a kernel on the caller's stream as in apply_transfer
int interpolate_transfer(const mfgpu_transfer *t, void *dst, const void *src, hipStream_t st) {
  const bool f64 = t->number_type == MFGPU_F64;
  if (!t->interp_covers_all) {
    if (f64)
      hipLaunchKernelGGL(zero_kernel<double>, dim3(2048), dim3(256), 0, st, (double *)dst, (size_t)t->n_coarse_dofs);
    else
      hipLaunchKernelGGL(zero_kernel<float>, dim3(2048), dim3(256), 0, st, (float *)dst, (size_t)t->n_coarse_dofs);
  }
  HIP_TRY(f64 ? launch_h_hn_interpolate<double>(t, dst, src, st) : launch_h_hn_interpolate<float>(t, dst, src, st));
  return 0;
}

}  // namespace

void transfer_sizes(const mfgpu_transfer *t, uint32_t *n_coarse_dofs, uint32_t *n_fine_dofs, int *number_type) {
  *n_coarse_dofs = t->n_coarse_dofs;
  *n_fine_dofs = t->n_fine_dofs;
  *number_type = t->number_type;
}

}  // namespace mfgpu

extern "C" {

int mfgpu_transfer_create(int dim, int degree, int number_type, uint32_t n_coarse_cells, const uint32_t *coarse_cell_dofs,
                          const uint32_t *fine_patch_dofs, uint32_t n_coarse_dofs, uint32_t n_fine_dofs,
                          const uint32_t *coarse_dirichlet, uint32_t n_coarse_dirichlet, const double *prolongation_1d,
                          mfgpu_transfer **out) {
  mfgpu::TransferInput in;
  in.who = "mfgpu_transfer_create";
  in.kind = mfgpu::TRANSFER_KIND_H;
  in.dim = dim;
  in.degree = degree;
  in.number_type = number_type;
  in.n_coarse_cells = in.n_fine_cells = n_coarse_cells;
  in.coarse_cell_dofs = coarse_cell_dofs;
  in.fine_cell_dofs = fine_patch_dofs;
  in.n_coarse_dofs = n_coarse_dofs;
  in.n_fine_dofs = n_fine_dofs;
  in.coarse_dirichlet = coarse_dirichlet;
  in.n_coarse_dirichlet = n_coarse_dirichlet;
  in.prolongation_1d = prolongation_1d;
  return mfgpu::create_transfer(in, out);
}

int mfgpu_transfer_create_from_meshes(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, mfgpu_transfer **out) {
  using namespace mfgpu;
  if (!coarse || !fine || !out) {
    set_error("mfgpu_transfer_create_from_meshes: null argument");
    return MFGPU_EINVAL;
  }
  std::vector<uint32_t> cd, fd;
  int rc = mesh_transfer_patches(coarse->mesh, fine->mesh, cd, fd);
  if (rc) return rc;
  return mfgpu_transfer_create(coarse->mesh.dim, coarse->mesh.degree, fine->mesh.number_type, coarse->mesh.n_cells, cd.data(),
                               fd.data(), coarse->mesh.n_dofs, fine->mesh.n_dofs, coarse->mesh.constrained.data(),
                               (uint32_t)coarse->mesh.constrained.size(), nullptr, out);
}

int mfgpu_transfer_create_p(int dim, int degree_coarse, int degree_fine, int number_type, uint32_t n_cells,
                            const uint32_t *coarse_cell_dofs, const uint32_t *fine_cell_dofs, uint32_t n_coarse_dofs,
                            uint32_t n_fine_dofs, const uint32_t *coarse_dirichlet, uint32_t n_coarse_dirichlet,
                            const double *prolongation_1d, mfgpu_transfer **out) {
  return mfgpu_transfer_create_p_hn(dim, degree_coarse, degree_fine, number_type, n_cells, coarse_cell_dofs, fine_cell_dofs,
                                    n_coarse_dofs, n_fine_dofs, coarse_dirichlet, n_coarse_dirichlet, prolongation_1d, nullptr,
                                    nullptr, out);
}

int mfgpu_transfer_create_p_hn(int dim, int degree_coarse, int degree_fine, int number_type, uint32_t n_cells,
                               const uint32_t *coarse_cell_dofs, const uint32_t *fine_cell_dofs, uint32_t n_coarse_dofs,
                               uint32_t n_fine_dofs, const uint32_t *coarse_dirichlet, uint32_t n_coarse_dirichlet,
                               const double *prolongation_1d, const uint32_t *constraint_mask,
                               const double *coarse_constraint_weights, mfgpu_transfer **out) {
  mfgpu::TransferInput in;
  in.who = "mfgpu_transfer_create_p_hn";
  in.kind = mfgpu::TRANSFER_KIND_P;
  in.dim = dim;
  in.degree_coarse = degree_coarse;
  in.degree = degree_fine;
  in.number_type = number_type;
  in.n_coarse_cells = in.n_fine_cells = n_cells;
  in.coarse_cell_dofs = coarse_cell_dofs;
  in.fine_cell_dofs = fine_cell_dofs;
  in.n_coarse_dofs = n_coarse_dofs;
  in.n_fine_dofs = n_fine_dofs;
  in.coarse_dirichlet = coarse_dirichlet;
  in.n_coarse_dirichlet = n_coarse_dirichlet;
  in.prolongation_1d = prolongation_1d;
  in.coarse_mask = in.fine_mask = constraint_mask;  // (NULL: the conforming object, the HN = false kernels)
  in.constraint_weights = coarse_constraint_weights;
  return mfgpu::create_transfer(in, out);
}

int mfgpu_transfer_create_p_from_meshes(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, mfgpu_transfer **out) {
  using namespace mfgpu;
  if (!coarse || !fine || !out) {
    set_error("mfgpu_transfer_create_p_from_meshes: null argument");
    return MFGPU_EINVAL;
  }
  const Mesh &C = coarse->mesh, &F = fine->mesh;
  if (C.cells_kind < 0 || F.cells_kind < 0 || !C.constraint_mask.empty() || !F.constraint_mask.empty()) {
    set_error("mfgpu_transfer_create_p_from_meshes: meshes with hanging nodes (adaptive, from leaves) are not supported");
    return MFGPU_EUNSUPPORTED;
  }
  bool same = C.dim == F.dim && C.cells_kind == F.cells_kind && C.n_cells == F.n_cells;
  if (same && C.cells_kind == 0)
    for (int d = 0; d < 3; ++d) same = same && C.nper[d] == F.nper[d];
  same = same && C.slab[0] == F.slab[0] && C.slab[1] == F.slab[1] && C.n_ref == F.n_ref;
  if (!same) {
    set_error("mfgpu_transfer_create_p_from_meshes: the two meshes are not the same cells (dimension, kind, cells per "
              "direction and slab or n_ref, cell count)");
    return MFGPU_EINVAL;
  }
  return mfgpu_transfer_create_p(C.dim, C.degree, F.degree, F.number_type, C.n_cells, C.loc2glob.data(), F.loc2glob.data(),
                                 C.n_dofs, F.n_dofs, C.constrained.data(), (uint32_t)C.constrained.size(), nullptr, out);
}

int mfgpu_transfer_create_p_hn_from_meshes(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, mfgpu_transfer **out) {
  using namespace mfgpu;
  if (!coarse || !fine || !out) {
    set_error("mfgpu_transfer_create_p_hn_from_meshes: null argument");
    return MFGPU_EINVAL;
  }
  const Mesh &C = coarse->mesh, &F = fine->mesh;
  if (C.cells_kind >= 0 && F.cells_kind >= 0 && C.constraint_mask.empty() && F.constraint_mask.empty())
    return mfgpu_transfer_create_p_from_meshes(coarse, fine, out);
  // adaptive meshes and meshes from leaves: the same leaves in the same order; the masks are geometric, so equal too
  if (C.cells_kind != -1 || F.cells_kind != -1 || C.dim != F.dim || C.n_cells != F.n_cells || C.cell_levels.empty() ||
      C.cell_levels != F.cell_levels || C.constraint_mask != F.constraint_mask) {
    set_error("mfgpu_transfer_create_p_hn_from_meshes: the two meshes are not the same cells (dimension, cell count, the "
              "leaves and their order, constraint masks)");
    return MFGPU_EINVAL;
  }
  return mfgpu_transfer_create_p_hn(C.dim, C.degree, F.degree, F.number_type, C.n_cells, C.loc2glob.data(), F.loc2glob.data(),
                                    C.n_dofs, F.n_dofs, C.constrained.data(), (uint32_t)C.constrained.size(), nullptr,
                                    C.constraint_mask.empty() ? nullptr : C.constraint_mask.data(), C.weights.data(), out);
}

// the two creators of the kind H_HN object; `interpolation`: with the interpolation image
static int create_h_hn(const char *who, bool interpolation, int dim, int degree, int number_type, uint32_t n_coarse_cells,
                       uint32_t n_fine_cells, const uint32_t *coarse_cell_dofs, const uint32_t *fine_cell_dofs,
                       const uint32_t *parent, const uint32_t *child, uint32_t n_coarse_dofs, uint32_t n_fine_dofs,
                       const uint32_t *coarse_dirichlet, uint32_t n_coarse_dirichlet, const double *prolongation_1d,
                       const uint32_t *coarse_mask, const uint32_t *fine_mask, const double *constraint_weights,
                       const double *interpolation_1d, mfgpu_transfer **out) {
  mfgpu::TransferInput in;
  in.who = who;
  in.kind = mfgpu::TRANSFER_KIND_H_HN;
  in.dim = dim;
  in.degree = degree;
  in.number_type = number_type;
  in.n_coarse_cells = n_coarse_cells;
  in.n_fine_cells = n_fine_cells;
  in.coarse_cell_dofs = coarse_cell_dofs;
  in.fine_cell_dofs = fine_cell_dofs;
  in.parent = parent;
  in.child = child;
  in.n_coarse_dofs = n_coarse_dofs;
  in.n_fine_dofs = n_fine_dofs;
  in.coarse_dirichlet = coarse_dirichlet;
  in.n_coarse_dirichlet = n_coarse_dirichlet;
  in.prolongation_1d = prolongation_1d;
  in.coarse_mask = coarse_mask;
  in.fine_mask = fine_mask;
  in.constraint_weights = constraint_weights;
  in.interpolation = interpolation;
  in.interpolation_1d = interpolation_1d;
  return mfgpu::create_transfer(in, out);
}

int mfgpu_transfer_create_h_hn(int dim, int degree, int number_type, uint32_t n_coarse_cells, uint32_t n_fine_cells,
                               const uint32_t *coarse_cell_dofs, const uint32_t *fine_cell_dofs, const uint32_t *parent,
                               const uint32_t *child, uint32_t n_coarse_dofs, uint32_t n_fine_dofs,
                               const uint32_t *coarse_dirichlet, uint32_t n_coarse_dirichlet, const double *prolongation_1d,
                               const uint32_t *coarse_mask, const uint32_t *fine_mask, const double *constraint_weights,
                               mfgpu_transfer **out) {
  return create_h_hn("mfgpu_transfer_create_h_hn", false, dim, degree, number_type, n_coarse_cells, n_fine_cells,
                     coarse_cell_dofs, fine_cell_dofs, parent, child, n_coarse_dofs, n_fine_dofs, coarse_dirichlet,
                     n_coarse_dirichlet, prolongation_1d, coarse_mask, fine_mask, constraint_weights, nullptr, out);
}

int mfgpu_transfer_create_h_hn_interp(int dim, int degree, int number_type, uint32_t n_coarse_cells, uint32_t n_fine_cells,
                                      const uint32_t *coarse_cell_dofs, const uint32_t *fine_cell_dofs,
                                      const uint32_t *parent, const uint32_t *child, uint32_t n_coarse_dofs,
                                      uint32_t n_fine_dofs, const uint32_t *coarse_dirichlet, uint32_t n_coarse_dirichlet,
                                      const double *prolongation_1d, const uint32_t *coarse_mask, const uint32_t *fine_mask,
                                      const double *constraint_weights, const double *interpolation_1d,
                                      mfgpu_transfer **out) {
  return create_h_hn("mfgpu_transfer_create_h_hn_interp", true, dim, degree, number_type, n_coarse_cells, n_fine_cells,
                     coarse_cell_dofs, fine_cell_dofs, parent, child, n_coarse_dofs, n_fine_dofs, coarse_dirichlet,
                     n_coarse_dirichlet, prolongation_1d, coarse_mask, fine_mask, constraint_weights, interpolation_1d, out);
}

static int create_h_hn_from_meshes(const char *who, bool interpolation, const mfgpu_mesh *coarse, const mfgpu_mesh *fine,
                                   mfgpu_transfer **out) {
  using namespace mfgpu;
  if (!coarse || !fine || !out) {
    set_error(std::string(who) + ": null argument");
    return MFGPU_EINVAL;
  }
  const Mesh &C = coarse->mesh, &F = fine->mesh;
  if (C.cells_kind != -1 || F.cells_kind != -1 || C.cell_levels.empty() || F.cell_levels.empty() || C.dim != F.dim ||
      C.degree != F.degree) {
    set_error(std::string(who) + ": needs two leaf meshes (adaptive, from leaves) of one dimension and one degree");
    return MFGPU_EINVAL;
  }
  std::vector<uint32_t> parent(F.n_cells), child(F.n_cells);
  int rc = mfgpu_mesh_coarsening_map(coarse, fine, parent.data(), child.data());
  if (rc) return rc;
  return create_h_hn(interpolation ? "mfgpu_transfer_create_h_hn_interp" : "mfgpu_transfer_create_h_hn", interpolation, C.dim,
                     C.degree, F.number_type, C.n_cells, F.n_cells, C.loc2glob.data(), F.loc2glob.data(), parent.data(),
                     child.data(), C.n_dofs, F.n_dofs, C.constrained.data(), (uint32_t)C.constrained.size(), nullptr,
                     C.constraint_mask.empty() ? nullptr : C.constraint_mask.data(),
                     F.constraint_mask.empty() ? nullptr : F.constraint_mask.data(), C.weights.data(), nullptr, out);
}

int mfgpu_transfer_create_h_hn_from_meshes(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, mfgpu_transfer **out) {
  return create_h_hn_from_meshes("mfgpu_transfer_create_h_hn_from_meshes", false, coarse, fine, out);
}

int mfgpu_transfer_create_h_hn_interp_from_meshes(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, mfgpu_transfer **out) {
  return create_h_hn_from_meshes("mfgpu_transfer_create_h_hn_interp_from_meshes", true, coarse, fine, out);
}

int mfgpu_transfer_interpolate(mfgpu_transfer *t, void *dst_coarse, const void *src_fine, void *stream) {
  using namespace mfgpu;
  const char *who = "mfgpu_transfer_interpolate";
  if (!t || !dst_coarse || !src_fine) {
    set_error(std::string(who) + ": null argument");
    return MFGPU_EINVAL;
  }
  if (t->kind != TRANSFER_KIND_H_HN || !t->interpolation) {
    set_error(std::string(who) + ": the object has no interpolation image (make it with mfgpu_transfer_create_h_hn_interp or "
                                 "mfgpu_transfer_create_h_hn_interp_from_meshes)");
    return MFGPU_EINVAL;
  }
  return interpolate_transfer(t, dst_coarse, src_fine, (hipStream_t)stream);
}

int mfgpu_transfer_prolongate(mfgpu_transfer *t, void *dst_fine, const void *src_coarse, void *stream) {
  return mfgpu::apply_transfer("mfgpu_transfer_prolongate", t, dst_fine, src_coarse, mfgpu::TRANSFER_PROLONGATE, stream);
}

int mfgpu_transfer_prolongate_add(mfgpu_transfer *t, void *dst_fine, const void *src_coarse, void *stream) {
  return mfgpu::apply_transfer("mfgpu_transfer_prolongate_add", t, dst_fine, src_coarse, mfgpu::TRANSFER_PROLONGATE_ADD, stream);
}

int mfgpu_transfer_restrict_and_add(mfgpu_transfer *t, void *dst_coarse, const void *src_fine, void *stream) {
  return mfgpu::apply_transfer("mfgpu_transfer_restrict_and_add", t, dst_coarse, src_fine, mfgpu::TRANSFER_RESTRICT_ADD, stream);
}

size_t mfgpu_transfer_memory_consumption(const mfgpu_transfer *t) { return t ? t->device_bytes : 0; }

void mfgpu_transfer_destroy(mfgpu_transfer *t) { delete t; }

}  // extern "C"
