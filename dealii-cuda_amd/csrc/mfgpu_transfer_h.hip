// Global-coarsening h-transfer: prolongate / prolongate_add / restrict_and_add between two LEAF
// meshes with hanging nodes at ONE degree p, the fine mesh's leaves each either a leaf of the coarse mesh (child = 0) or
// child k of one (child = 1 + k, bit d of k: the upper half in direction d).  What deal.II's MGTransferGlobalCoarsening
// does between two members of create_geometric_coarsening_sequence.  The object is an mfgpu_transfer (mfgpu_transfer.h,
// kind H_HN); the semantics are section 19's with two masks:
//   owner of a fine dof   the first fine cell that lists it at a position its FINE mask does not constrain (p_owner_list)
//   prolongate            for the owner F with parent K:  dst[fine(F, i)] = [ E(child_F) C_p(coarse_mask_K) gather_K(src) ]_i,
//                         coarse Dirichlet dofs read as 0; plain store (prolongate_add: plain read-modify-write)
//   restrict_and_add      the exact transpose: owned entries, E^T, C_p^T (z, y, x), floating-point atomics that skip the
//                         coarse Dirichlet dofs
// E(child) is the tensor product of one HALF of P1[(2p+1) x (p+1)] per direction: rows 0..p the lower half, rows p..2p the
// upper one (they share row p, so P1 as uploaded for the level h-transfer holds both); for child = 0 it is the identity
// and the contractions are skipped, so an unchanged cell without a coarse mask passes its values through bit for bit.  An
// unchanged cell may carry a coarse mask it does not have in the fine mesh (its neighbour was coarsened): C_p handles it.
//
// Mapping: p_transfer_kernel's (mfgpu_transfer_p.hip).  One wave per FINE cell, four per 256-thread workgroup, grid-stride
// with the 2048-workgroup cap; the index lists are requested one cell ahead; the two ping-pong arrays of a cell sit in
// the wave's own LDS slice with wave_sync() between the stages; P1 (both halves) and W are staged in LDS once per
// workgroup.  pc = pf = p, so every extent is the compile-time n = p + 1, and the matrix half of a direction is picked by
// a wave-uniform bit of `child` (a scalar offset).
//
// Where the coarse list comes from -- byte model per fine cell (N = n^dim, T = 8 or 4 bytes):
//   both variants    4 N fine indices, N T vector entries at either end (the owned part on the fine side)
//   through parent   4 (parent) + 4 (child and the parent's mask in one word) + 4 N coarse indices that the 2^dim children
//                    of a refined parent read one after the other (Morton order: the same wave or its neighbours), so
//                    HBM sees 4 N / 2^dim of them and L2 the rest; device memory 4 N n_coarse + 8 n_fine
//   per-fine copies  4 (word) + 4 N coarse indices from HBM for every fine cell; device memory 4 N n_fine + 4 n_fine
// At p = 4 in 3D (N = 125) on a pair where most fine cells are children: 500 + 8 + 63 B of index traffic against
// 500 + 4 + 500 B, and 1/8 of the coarse index memory.  So the list is indexed THROUGH PARENT.  The extra dependent load
// (parent -> coarse index -> value) is hidden by requesting the parent word TWO cells ahead: when the lists of the next
// cell are requested its parent has been in a register for a whole cell.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mfgpu_device.h"
#include "mfgpu_mesh.h"
#include "mfgpu_transfer.h"
#include "mfgpu_transfer_hn.h"

namespace mfgpu {

namespace {

constexpr int ipow_c(int a, int e) { return e == 0 ? 1 : a * ipow_c(a, e - 1); }
constexpr int kWaves = 4;            // fine cells per workgroup pass
constexpr unsigned kMaxGrid = 2048;  // workgroups: 8 per CU on 256 CUs; more cells than 4 * kMaxGrid take further passes

template <int dim, int p, typename T, bool RESTRICT, bool ADD>
__global__ void __launch_bounds__(64 * kWaves)
h_hn_transfer_kernel(T *__restrict__ dst, const T *__restrict__ src, const uint32_t *__restrict__ coarse,
                     const uint32_t *__restrict__ fine, const uint32_t *__restrict__ parent,
                     const uint32_t *__restrict__ words, const T *__restrict__ p1, const T *__restrict__ hn_weights,
                     uint32_t n_cells) {
  constexpr int n = p + 1, N = ipow_c(n, dim), NP = (2 * p + 1) * n;
  __shared__ T buf[kWaves][2][N], P[NP + n * n];  // P1 (lower half: rows 0..p, upper: rows p..2p), then W[n * n]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = threadIdx.x; t < NP; t += 64 * kWaves) P[t] = p1[t];
  for (int t = threadIdx.x; t < n * n; t += 64 * kWaves) P[NP + t] = hn_weights[t];
  const T *W = P + NP;
  __syncthreads();
  // Both index lists of a cell sit in registers (entry lane + 64 j in slot j; past the end: bit 31, "skip") and are
  // requested one cell ahead, the parent index and the child / mask word two cells ahead (file header)
  constexpr int KF = (N + 63) / 64;
  constexpr uint32_t kSkip = 0x80000000u;
  const uint64_t stride = (uint64_t)gridDim.x * kWaves;
  uint64_t cell = (uint64_t)blockIdx.x * kWaves + wave;
  uint32_t word = cell < n_cells ? words[cell] : 0u;
  uint32_t gc[KF], gf[KF];
  {
    const uint64_t par = cell < n_cells ? parent[cell] : 0u;
#pragma unroll
    for (int j = 0; j < KF; ++j) {
      const int t = lane + 64 * j;
      gc[j] = (cell < n_cells && t < N) ? coarse[par * N + t] : kSkip;
      gf[j] = (cell < n_cells && t < N) ? fine[cell * N + t] : kSkip;
    }
  }
  uint32_t next_par = cell + stride < n_cells ? parent[cell + stride] : 0u;
  uint32_t next_word = cell + stride < n_cells ? words[cell + stride] : 0u;
  for (; cell < n_cells; cell += stride) {
    T *in = buf[wave][0], *out = buf[wave][1];
    wave_sync();  // the previous cell's last reads of its arrays come first
#pragma unroll
    for (int j = 0; j < KF; ++j) {
      const int t = lane + 64 * j;
      const uint32_t g = RESTRICT ? gf[j] : gc[j];  // coarse Dirichlet dofs read as 0; a fine dof enters through its owner
      if (t < N) in[t] = (g >> 31) ? T(0) : src[g];
    }
    const uint64_t next = cell + stride, after = next + stride;
    const uint32_t after_par = after < n_cells ? parent[after] : 0u;
    const uint32_t after_word = after < n_cells ? words[after] : 0u;
    uint32_t next_gc[KF], next_gf[KF];
#pragma unroll
    for (int j = 0; j < KF; ++j) {
      const int t = lane + 64 * j;
      next_gc[j] = (next < n_cells && t < N) ? coarse[(uint64_t)next_par * N + t] : kSkip;
      next_gf[j] = (next < n_cells && t < N) ? fine[next * N + t] : kSkip;
    }
    // one wave owns one cell: the word is the same in all lanes, say so (scalar branches and a scalar matrix offset)
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)word);
    const uint32_t m = w & 0x1ffu, child = w >> 16;
    wave_sync();
    if (!RESTRICT && m) hn_resolve_wave<dim, false, KF>(in, W, n, m, lane);  // C_p on the gathered coarse values
    if (child) {  // (uniform) child = 0: the same cell, E is the identity
#pragma unroll
      for (int k = 0; k < dim; ++k) {
        const int lo = k == 0 ? 1 : k == 1 ? n : n * n;  // (compile-time once the loop over k is unrolled)
        const T *rows = P + (((child - 1) >> k) & 1u) * (p * n);  // the lower or the upper half of P1
#pragma unroll
        for (int j = 0; j < KF; ++j) {
          const int t = lane + 64 * j;
          if (t < N) {
            const int o = (t / lo) % n;
            const T *v = in + (t - o * lo);
            T s = T(0);
#pragma unroll
            for (int i = 0; i < n; ++i) s += (RESTRICT ? rows[i * n + o] : rows[o * n + i]) * v[i * lo];
            out[t] = s;
          }
        }
        wave_sync();
        T *tmp = in;
        in = out;
        out = tmp;
      }
    }
    if (RESTRICT && m) hn_resolve_wave<dim, true, KF>(in, W, n, m, lane);  // C_p^T before the atomics
#pragma unroll
    for (int j = 0; j < KF; ++j) {
      const int t = lane + 64 * j;
      if (!RESTRICT) {
        const uint32_t g = gf[j];
        if (t < N && !(g >> 31)) dst[g] = ADD ? dst[g] + in[t] : in[t];  // one owner per fine dof: no atomics
      } else {
        const uint32_t g = gc[j];
        if (t < N && !(g >> 31)) atomicAdd(dst + g, in[t]);  // several cells share the coarse dof; Dirichlet dofs are skipped
      }
      gc[j] = next_gc[j];
      gf[j] = next_gf[j];
    }
    word = next_word;
    next_par = after_par;
    next_word = after_word;
  }
}

template <typename T, bool RESTRICT, bool ADD>
hipError_t launch_h(const mfgpu_transfer *t, T *dst, const T *src, hipStream_t st) {
  const uint32_t n = t->n_fine_cells;
  if (n == 0) return hipSuccess;
  const unsigned groups = (n + kWaves - 1) / kWaves;
  const unsigned grid = groups < kMaxGrid ? groups : kMaxGrid;
#define TRH_CASE(D, PP)                                                                                               \
  case D * 10 + PP:                                                                                                   \
    hipLaunchKernelGGL((h_hn_transfer_kernel<D, PP, T, RESTRICT, ADD>), dim3(grid), dim3(64 * kWaves), 0, st, dst, src,  \
                       t->d_coarse.get(), t->d_fine.get(), t->d_parent.get(), t->d_mask.get(), t->d_p1.as<const T>(), \
                       t->d_weights.as<const T>(), n);                                                                \
    break;
  switch (t->dim * 10 + t->degree) {
    TRH_CASE(2, 1) TRH_CASE(2, 2) TRH_CASE(2, 3) TRH_CASE(2, 4) TRH_CASE(2, 5) TRH_CASE(2, 6)
    TRH_CASE(3, 1) TRH_CASE(3, 2) TRH_CASE(3, 3) TRH_CASE(3, 4) TRH_CASE(3, 5) TRH_CASE(3, 6)
    default: return hipErrorInvalidValue;
  }
#undef TRH_CASE
  return hipGetLastError();
}

template <typename T>
hipError_t launch_mode(const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, hipStream_t st) {
  switch (mode) {
    case TRANSFER_PROLONGATE: return launch_h<T, false, false>(t, (T *)dst, (const T *)src, st);
    case TRANSFER_PROLONGATE_ADD: return launch_h<T, false, true>(t, (T *)dst, (const T *)src, st);
    case TRANSFER_RESTRICT_ADD: return launch_h<T, true, false>(t, (T *)dst, (const T *)src, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_h_hn_transfer(const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, hipStream_t st) {
  return t->number_type == MFGPU_F64 ? launch_mode<double>(t, dst, src, mode, st) : launch_mode<float>(t, dst, src, mode, st);
}

}  // namespace mfgpu

extern "C" {

int mfgpu_transfer_create_h_hn(int dim, int degree, int number_type, uint32_t n_coarse_cells, uint32_t n_fine_cells,
                               const uint32_t *coarse_cell_dofs, const uint32_t *fine_cell_dofs, const uint32_t *parent,
                               const uint32_t *child, uint32_t n_coarse_dofs, uint32_t n_fine_dofs,
                               const uint32_t *coarse_dirichlet, uint32_t n_coarse_dirichlet, const double *prolongation_1d,
                               const uint32_t *coarse_mask, const uint32_t *fine_mask, const double *constraint_weights,
                               mfgpu_transfer **out) {
  using namespace mfgpu;
  const char *who = "mfgpu_transfer_create_h_hn";
  if (!out || (dim != 2 && dim != 3) || degree < 1 || degree > 6 || (n_coarse_cells && !coarse_cell_dofs) ||
      (n_fine_cells && (!fine_cell_dofs || !parent || !child)) || (n_coarse_dirichlet && !coarse_dirichlet) ||
      !valid_number_type(number_type) || n_coarse_dofs >= (1u << 31) || n_fine_dofs >= (1u << 31)) {
    set_error(std::string(who) + ": bad argument (1 <= degree <= 6, dim 2 or 3, dof counts < 2^31, arrays)");
    return MFGPU_EINVAL;
  }
  const int n = degree + 1;
  const size_t N = (size_t)ipow(n, dim);
  std::vector<uint8_t> dir(n_coarse_dofs, 0);
  for (uint32_t i = 0; i < n_coarse_dirichlet; ++i) {
    if (coarse_dirichlet[i] >= n_coarse_dofs) {
      set_error(std::string(who) + ": Dirichlet dof out of range");
      return MFGPU_EINVAL;
    }
    dir[coarse_dirichlet[i]] = 1;
  }
  std::vector<uint32_t> cd((size_t)n_coarse_cells * N), fd((size_t)n_fine_cells * N), words(n_fine_cells);
  for (size_t i = 0; i < cd.size(); ++i) {
    const uint32_t g = coarse_cell_dofs[i];
    if (g >= n_coarse_dofs) {
      set_error(std::string(who) + ": coarse dof out of range");
      return MFGPU_EINVAL;
    }
    cd[i] = g | (dir[g] ? 0x80000000u : 0u);
  }
  for (uint32_t c = 0; c < n_coarse_cells; ++c)
    if (coarse_mask && !valid_mask(dim, coarse_mask[c])) {
      set_error(std::string(who) + ": a coarse constraint mask has bits outside the defined ones (9 in 3D; TYPE x, y and "
                "FACE x, y in 2D)");
      return MFGPU_EINVAL;
    }
  for (uint32_t f = 0; f < n_fine_cells; ++f) {
    if (parent[f] >= n_coarse_cells || child[f] > (1u << dim)) {
      set_error(std::string(who) + ": parent out of range or child > 2^dim");
      return MFGPU_EINVAL;
    }
    words[f] = (coarse_mask ? coarse_mask[parent[f]] : 0u) | (child[f] << 16);
  }
  size_t covered = 0;
  int rc;
  if ((rc = p_owner_list(who, dim, degree, n_fine_cells, fine_cell_dofs, fine_mask, n_fine_dofs, fd.data(), covered)))
    return rc;
  std::vector<double> P1, W;
  if (prolongation_1d)
    P1.assign(prolongation_1d, prolongation_1d + (size_t)(2 * degree + 1) * n);
  else
    default_prolongation_1d(degree, P1);
  if (constraint_weights)
    W.assign(constraint_weights, constraint_weights + (size_t)n * n);
  else
    fe_q_constraint_weights(degree, W);
  std::unique_ptr<mfgpu_transfer> t(new mfgpu_transfer());
  t->kind = TRANSFER_KIND_H_HN;
  t->dim = dim;
  t->degree = degree;
  t->number_type = number_type;
  t->n_coarse_cells = n_coarse_cells;
  t->n_fine_cells = n_fine_cells;
  t->n_coarse_dofs = n_coarse_dofs;
  t->n_fine_dofs = n_fine_dofs;
  t->covers_all = covered == n_fine_dofs;
  t->hanging_nodes = true;
  std::vector<float> P1f(P1.begin(), P1.end()), Wf(W.begin(), W.end());
  const bool f64 = number_type == MFGPU_F64;
  if ((rc = t->d_coarse.upload(cd.data(), cd.size())) || (rc = t->d_fine.upload(fd.data(), fd.size())) ||
      (rc = t->d_parent.upload(parent, n_fine_cells)) || (rc = t->d_mask.upload(words.data(), words.size())) ||
      (rc = t->d_p1.upload(f64 ? (const void *)P1.data() : (const void *)P1f.data(), P1.size() * esize(number_type))) ||
      (rc = t->d_weights.upload(f64 ? (const void *)W.data() : (const void *)Wf.data(), W.size() * esize(number_type))))
    return rc;
  t->device_bytes = t->d_coarse.bytes() + t->d_fine.bytes() + t->d_parent.bytes() + t->d_mask.bytes() + t->d_p1.bytes() +
                    t->d_weights.bytes();
  *out = t.release();
  return 0;
}

int mfgpu_transfer_create_h_hn_from_meshes(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, mfgpu_transfer **out) {
  using namespace mfgpu;
  if (!coarse || !fine || !out) {
    set_error("mfgpu_transfer_create_h_hn_from_meshes: null argument");
    return MFGPU_EINVAL;
  }
  const Mesh &C = coarse->mesh, &F = fine->mesh;
  if (C.cells_kind != -1 || F.cells_kind != -1 || C.cell_levels.empty() || F.cell_levels.empty() || C.dim != F.dim ||
      C.degree != F.degree) {
    set_error("mfgpu_transfer_create_h_hn_from_meshes: needs two leaf meshes (adaptive, from leaves) of one dimension and "
              "one degree");
    return MFGPU_EINVAL;
  }
  std::vector<uint32_t> parent(F.n_cells), child(F.n_cells);
  int rc = mfgpu_mesh_coarsening_map(coarse, fine, parent.data(), child.data());
  if (rc) return rc;
  return mfgpu_transfer_create_h_hn(C.dim, C.degree, F.number_type, C.n_cells, F.n_cells, C.loc2glob.data(), F.loc2glob.data(),
                                    parent.data(), child.data(), C.n_dofs, F.n_dofs, C.constrained.data(),
                                    (uint32_t)C.constrained.size(), nullptr,
                                    C.constraint_mask.empty() ? nullptr : C.constraint_mask.data(),
                                    F.constraint_mask.empty() ? nullptr : F.constraint_mask.data(), C.weights.data(), out);
}

}  // extern "C"
