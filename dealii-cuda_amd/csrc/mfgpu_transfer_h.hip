// Global-coarsening h-transfer: prolongate / prolongate_add / restrict_and_add between two LEAF
// meshes with hanging nodes at ONE degree p, the fine mesh's leaves each either a leaf of the coarse mesh (child = 0) or
// child k of one (child = 1 + k, bit d of k: the upper half in direction d).  What deal.II's MGTransferGlobalCoarsening
// does between two members of create_geometric_coarsening_sequence.  The object is an mfgpu_transfer (mfgpu_transfer.h,
// kind H_HN); the semantics are section 19's with two masks:
//   owner of a fine dof   the first fine cell that lists it at a position its FINE mask does not constrain (the owner rule)
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
// The creator is in mfgpu_transfer.hip; what the kernel shares with the p kernel in mfgpu_transfer_wave.h.
// The second kernel of this file, h_hn_interpolate_kernel, is the interpolation of the same object from the fine to the
// coarse mesh (one wave per COARSE cell); its mapping and byte model stand in front of it.
#include <hip/hip_runtime.h>

#include "mfgpu_transfer.h"
#include "mfgpu_transfer_wave.h"

namespace mfgpu {

namespace {

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
  const uint64_t stride = (uint64_t)gridDim.x * kWaves;
  uint64_t cell = (uint64_t)blockIdx.x * kWaves + wave;
  uint32_t word = cell < n_cells ? words[cell] : 0u;
  uint32_t gc[KF], gf[KF];
  {
    const uint64_t par = cell < n_cells ? parent[cell] : 0u;
#pragma unroll
    for (int j = 0; j < KF; ++j) {
      const int t = lane + 64 * j;
      gc[j] = (cell < n_cells && t < N) ? coarse[par * N + t] : kTransferSkip;
      gf[j] = (cell < n_cells && t < N) ? fine[cell * N + t] : kTransferSkip;
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
      next_gc[j] = (next < n_cells && t < N) ? coarse[(uint64_t)next_par * N + t] : kTransferSkip;
      next_gf[j] = (next < n_cells && t < N) ? fine[next * N + t] : kTransferSkip;
    }
    // one wave owns one cell: the word is the same in all lanes, say so (scalar branches and a scalar matrix offset)
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)word);
    const uint32_t m = transfer_word_mask(w), child = transfer_word_child(w);
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
    }
    wave_hand_over(gc, gf, next_gc, next_gf);
    word = next_word;
    next_par = after_par;
    next_word = after_word;
  }
}

// mfgpu_transfer_interpolate: the fine function's nodal interpolant on the coarse mesh, per
// include/mfgpu.h.  One wave per COARSE cell on the skeleton above.  An unchanged cell gathers its one fine cell, resolves
// the FINE mask and stores.  A refined cell loops over its 2^dim children (the trip count is wave-uniform): each child is
// gathered, resolved where it has a mask, and contracted per direction with the rows of J1 that lie in its half only
// (rows 0..p/2 the lower, the others the upper half), at the positions that lie in its sub-block in the directions done
// so far; the sub-blocks of the children partition the N positions, so every lane keeps the results of its entries
// (lane + 64 j) in registers over the loop and the cell is stored once, by the owner, with plain stores.
// Requested ahead: the coarse owner list and the first fine cell's index one coarse cell ahead, the fine list and the
// fine mask one FINE cell ahead (the next child, or the next coarse cell's first fine cell).
// Byte model per coarse cell (N = n^dim, T = 8 or 4 bytes, c = 1 for an unchanged and 2^dim for a refined cell):
//   4 N coarse indices (owner marking), 4 * 2^dim fine cell indices, c * (4 N fine indices + 4 (mask) + N T source
//   entries), and the owned part of N T entries stored.
// At p = 4 in 3D for a refined cell: 500 + 32 + 8 * (504 + 1000) B read, at most 1000 B written; the fine side dominates
// as it does for restrict_and_add of the same pair, which reads the same fine lists and entries.
template <int dim, int n>
__device__ __forceinline__ bool in_child_block(int t, int k, int upto) {
  constexpr int H = (n - 1) / 2 + 1;  // rows of the lower half
  bool ok = true;
#pragma unroll
  for (int d = 0; d < dim; ++d) {
    const int c = (t / (d == 0 ? 1 : d == 1 ? n : n * n)) % n;
    if (d <= upto) ok = ok && (((k >> d) & 1) ? c >= H : c < H);
  }
  return ok;
}

template <int dim, int p, typename T>
__global__ void __launch_bounds__(64 * kWaves)
h_hn_interpolate_kernel(T *__restrict__ dst, const T *__restrict__ src, const uint32_t *__restrict__ coarse_owned,
                        const uint32_t *__restrict__ fine, const uint32_t *__restrict__ kids,
                        const uint32_t *__restrict__ fine_mask, const T *__restrict__ j1, const T *__restrict__ hn_weights,
                        uint32_t n_cells) {
  constexpr int n = p + 1, N = ipow_c(n, dim), NK = 1 << dim;
  __shared__ T buf[kWaves][2][N], J[2 * n * n];  // J1[n * n], then W[n * n]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = threadIdx.x; t < n * n; t += 64 * kWaves) {
    J[t] = j1[t];
    J[n * n + t] = hn_weights[t];
  }
  const T *W = J + n * n;
  __syncthreads();
  constexpr int KF = (N + 63) / 64;
  constexpr uint32_t kIndex = ~kTransferSkip;
  const uint64_t stride = (uint64_t)gridDim.x * kWaves;
  uint64_t cell = (uint64_t)blockIdx.x * kWaves + wave;
  uint32_t first = cell < n_cells ? kids[cell * NK] : 0u;  // fine cell 0 of the cell; bit 31: it is the cell itself
  uint32_t fm = cell < n_cells ? fine_mask[first & kIndex] : 0u;
  uint32_t gc[KF], gf[KF];
#pragma unroll
  for (int j = 0; j < KF; ++j) {
    const int t = lane + 64 * j;
    gc[j] = (cell < n_cells && t < N) ? coarse_owned[cell * N + t] : kTransferSkip;
    gf[j] = (cell < n_cells && t < N) ? fine[(uint64_t)(first & kIndex) * N + t] & kIndex : 0u;
  }
  for (; cell < n_cells; cell += stride) {
    const uint64_t next = cell + stride;
    const uint32_t next_first = next < n_cells ? kids[next * NK] : 0u;
    uint32_t next_gc[KF];
#pragma unroll
    for (int j = 0; j < KF; ++j) {
      const int t = lane + 64 * j;
      next_gc[j] = (next < n_cells && t < N) ? coarse_owned[next * N + t] : kTransferSkip;
    }
    // one wave owns one cell: say so (a scalar trip count, scalar branches)
    const bool same = (uint32_t)__builtin_amdgcn_readfirstlane((int)first) >> 31;
    const int n_kids = same ? 1 : NK;
    T r[KF];
#pragma unroll
    for (int j = 0; j < KF; ++j) r[j] = T(0);
    for (int k = 0; k < n_kids; ++k) {
      T *in = buf[wave][0], *out = buf[wave][1];
      wave_sync();  // the previous fine cell's last reads of its arrays come first
#pragma unroll
      for (int j = 0; j < KF; ++j) {
        const int t = lane + 64 * j;
        if (t < N) in[t] = src[gf[j]];  // every entry as it stands, whoever owns it
      }
      const bool more = k + 1 < n_kids, valid = more || next < n_cells;
      const uint32_t nf = (more ? kids[cell * NK + k + 1] : next_first) & kIndex;
      const uint32_t next_fm = valid ? fine_mask[nf] : 0u;
      uint32_t next_gf[KF];
#pragma unroll
      for (int j = 0; j < KF; ++j) {
        const int t = lane + 64 * j;
        next_gf[j] = (valid && t < N) ? fine[(uint64_t)nf * N + t] & kIndex : 0u;
      }
      const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)fm);
      wave_sync();
      if (m) hn_resolve_wave<dim, false, KF>(in, W, n, m, lane);  // C_p of the FINE mask on the gathered values
      if (!same) {
#pragma unroll
        for (int d = 0; d < dim; ++d) {
          const int lo = d == 0 ? 1 : d == 1 ? n : n * n;
#pragma unroll
          for (int j = 0; j < KF; ++j) {
            const int t = lane + 64 * j;
            if (t < N && in_child_block<dim, n>(t, k, d)) {
              const int o = (t / lo) % n;
              const T *v = in + (t - o * lo), *row = J + o * n;
              T s = T(0);
#pragma unroll
              for (int i = 0; i < n; ++i) s += row[i] * v[i * lo];
              out[t] = s;
            }
          }
          wave_sync();
          T *tmp = in;
          in = out;
          out = tmp;
        }
      }
#pragma unroll
      for (int j = 0; j < KF; ++j) {
        const int t = lane + 64 * j;
        if (t < N && (same || in_child_block<dim, n>(t, k, dim - 1))) r[j] = in[t];
      }
#pragma unroll
      for (int j = 0; j < KF; ++j) gf[j] = next_gf[j];
      fm = next_fm;
    }
#pragma unroll
    for (int j = 0; j < KF; ++j) {
      const int t = lane + 64 * j;
      const uint32_t g = gc[j];
      if (t < N && !(g >> 31)) dst[g] = r[j];  // one owner per coarse dof: no atomics
      gc[j] = next_gc[j];
    }
    first = next_first;
  }
}

}  // namespace

template <typename T>
hipError_t launch_h_hn_interpolate(const mfgpu_transfer *t, void *dst, const void *src, hipStream_t st) {
  const uint32_t n = t->n_coarse_cells;
  if (n == 0) return hipSuccess;
  return dispatch_dim_degree<1>(t->dim, t->degree, [&](auto D, auto P) {
    hipLaunchKernelGGL((h_hn_interpolate_kernel<D(), P(), T>), dim3(wave_grid(n)), dim3(64 * kWaves), 0, st, (T *)dst,
                       (const T *)src, t->d_interp_coarse.get(), t->d_fine.get(), t->d_interp_kids.get(),
                       t->d_interp_fine_mask.get(), t->d_j1.as<const T>(), t->d_weights.as<const T>(), n);
    return hipGetLastError();
  });
}
template hipError_t launch_h_hn_interpolate<double>(const mfgpu_transfer *, void *, const void *, hipStream_t);
template hipError_t launch_h_hn_interpolate<float>(const mfgpu_transfer *, void *, const void *, hipStream_t);

template <typename T>
hipError_t launch_h_hn_transfer(const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, hipStream_t st) {
  const uint32_t n = t->n_fine_cells;
  if (n == 0) return hipSuccess;
  return dispatch_kernel<1>(t, mode, [&](auto D, auto P, auto R, auto A) {
    hipLaunchKernelGGL((h_hn_transfer_kernel<D(), P(), T, R(), A()>), dim3(wave_grid(n)), dim3(64 * kWaves), 0, st, (T *)dst,
                       (const T *)src, t->d_coarse.get(), t->d_fine.get(), t->d_parent.get(), t->d_mask.get(),
                       t->d_p1.as<const T>(), t->d_weights.as<const T>(), n);
    return hipGetLastError();
  });
}
template hipError_t launch_h_hn_transfer<double>(const mfgpu_transfer *, void *, const void *, TransferMode, hipStream_t);
template hipError_t launch_h_hn_transfer<float>(const mfgpu_transfer *, void *, const void *, TransferMode, hipStream_t);

}  // namespace mfgpu
