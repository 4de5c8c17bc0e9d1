// p-multigrid transfer: prolongate / prolongate_add / restrict_and_add between FE_Q(pc) and
// FE_Q(pf), pc < pf, on the SAME cells.  The object is an mfgpu_transfer (mfgpu_transfer.h) and the semantics are those
// of the h-transfer in mfgpu_transfer.hip, with "coarse cell and the patch of its children" read as "the cell at degree
// pc and the same cell at degree pf":
//   prolongate        dst_fine    = P (src_coarse with the coarse Dirichlet dofs read as 0)   plain store by the owner cell
//   prolongate_add    dst_fine   += P (...)                                                     plain read-modify-write by the owner
//   restrict_and_add  dst_coarse += Z P^T src_fine                                             fine dofs enter through their owner,
//                                                                                              floating-point atomics on the coarse dofs
// P per cell is the tensor product of P1[(pf+1) x (pc+1)], the coarse 1D basis at the fine 1D nodes.
//
// Mapping: ONE WAVE owns one cell, four cells share a 256-thread workgroup, grid-stride over groups of four cells.  A cell
// has at most 7^3 = 343 entries (125 at degree 4), so the h-kernel's 256 threads and block-wide barriers per cell would
// leave most lanes idle and serialise the cells of a workgroup on s_barrier.  Each wave keeps its two ping-pong arrays
// in its own slice of LDS; the stages of one cell are ordered by program order within the wave (wave_sync below, the
// idiom of WaveSync in mfgpu_cell.h), so the only workgroup barrier is the one after P1 has been staged in LDS.
// Instantiated on (dim, pf, T, mode); pc is a run-time argument: 5 fine degrees instead of 15 pairs.  The loops over the
// fine extent have compile-time bounds, those over the coarse extent (at most pf) run-time ones.
//
// Byte model per cell (T = 8 or 4 bytes, NC = (pc+1)^dim, NF = (pf+1)^dim): 4 (NC + NF) index bytes; prolongate reads NC T
// and writes the owned part of NF T (prolongate_add reads it too); restrict_and_add reads the owned part of NF T and
// issues up to NC atomic adds.  Index and vector traffic: the contractions are (pc+1 + pf+1) NF-sized passes through LDS.
//
// Cells with hanging nodes (mfgpu_transfer_create_p_hn): the kernel's HN = true instantiations.  The
// cell's constraint mask (4 more bytes per cell) is requested one cell ahead like the index lists, the weight matrix of
// the COARSE degree sits in LDS behind P1, and a masked cell runs resolve_hanging_nodes on its coarse values in its wave's
// LDS slice: after the gather (prolongate), before the atomics (restrict, transposed).  Cells without a mask skip it on a
// scalar branch.  The fine side needs nothing: a constrained fine position is a bit-31 entry made on the host (the owner
// rule, mfgpu_transfer_build.h).
// The creators are in mfgpu_transfer.hip; what the kernel shares with the h_hn kernel in mfgpu_transfer_wave.h.
#include <hip/hip_runtime.h>

#include "mfgpu_transfer.h"
#include "mfgpu_transfer_wave.h"

namespace mfgpu {

namespace {

template <int dim, int pf, typename T, bool RESTRICT, bool ADD, bool HN>
__global__ void __launch_bounds__(64 * kWaves)
p_transfer_kernel(T *__restrict__ dst, const T *__restrict__ src, const uint32_t *__restrict__ coarse,
                  const uint32_t *__restrict__ fine, const T *__restrict__ p1, uint32_t n_cells, int pc,
                  const uint32_t *__restrict__ cmask, const T *__restrict__ hn_weights) {
  constexpr int nf = pf + 1, NF = ipow_c(nf, dim);
  const int nc = pc + 1;                         // 2 .. pf
  const int NC = dim == 3 ? nc * nc * nc : nc * nc;  // <= NF; every intermediate array has at most NF entries too
  __shared__ T buf[kWaves][2][NF], P[nf * pf + (HN ? pf * pf : 0)];  // HN: W[nc * nc] of the coarse degree behind P1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int t = threadIdx.x; t < nf * nc; t += 64 * kWaves) P[t] = p1[t];
  const T *W = P + nf * pf;
  if (HN)
    for (int t = threadIdx.x; t < nc * nc; t += 64 * kWaves) P[nf * pf + t] = hn_weights[t];
  __syncthreads();
  // A cell's two index lists sit in registers (entry lane + 64 j in slot j; past the end: bit 31, "skip") and are
  // requested ONE CELL AHEAD: index -> value is a dependent pair of global loads at both ends of a cell, and a wave
  // works through its cells one after the other, so without the prefetch a cell costs four memory latencies in a row.
  constexpr int KF = (NF + 63) / 64;
  const uint64_t stride = (uint64_t)gridDim.x * kWaves;
  uint64_t cell = (uint64_t)blockIdx.x * kWaves + wave;
  uint32_t gc[KF], gf[KF];
#pragma unroll
  for (int j = 0; j < KF; ++j) {
    const int t = lane + 64 * j;
    gc[j] = (cell < n_cells && t < NC) ? coarse[cell * NC + t] : kTransferSkip;
    gf[j] = (cell < n_cells && t < NF) ? fine[cell * NF + t] : kTransferSkip;
  }
  uint32_t mask = (HN && cell < n_cells) ? cmask[cell] : 0u;  // requested one cell ahead like the index lists
  constexpr int KC = (ipow_c(pf, dim) + 63) / 64;
  for (; cell < n_cells; cell += stride) {
    T *in = buf[wave][0], *out = buf[wave][1];
    wave_sync();  // the previous cell's last reads of its arrays come first
#pragma unroll
    for (int j = 0; j < KF; ++j) {
      const int t = lane + 64 * j;
      if (!RESTRICT) {
        if (t < NC) in[t] = (gc[j] >> 31) ? T(0) : src[gc[j]];  // coarse Dirichlet dofs read as 0
      } else {
        if (t < NF) in[t] = (gf[j] >> 31) ? T(0) : src[gf[j]];  // a fine dof enters through its owner cell only
      }
    }
    const uint64_t next = cell + stride;
    uint32_t next_gc[KF], next_gf[KF];
#pragma unroll
    for (int j = 0; j < KF; ++j) {
      const int t = lane + 64 * j;
      next_gc[j] = (next < n_cells && t < NC) ? coarse[next * NC + t] : kTransferSkip;
      next_gf[j] = (next < n_cells && t < NF) ? fine[next * NF + t] : kTransferSkip;
    }
    const uint32_t next_mask = (HN && next < n_cells) ? cmask[next] : 0u;
    // one wave owns one cell: the mask is the same in all lanes, say so (a scalar branch; cells without a mask skip)
    const uint32_t m = HN ? (uint32_t)__builtin_amdgcn_readfirstlane((int)mask) : 0u;
    wave_sync();
    if (HN && !RESTRICT && m) hn_resolve_wave<dim, false, KC>(in, W, nc, m, lane);  // C_pc on the gathered coarse values
#pragma unroll
    for (int k = 0; k < dim; ++k) {
      if (!RESTRICT) {
        // direction k goes nc -> nf; directions < k are nf long already, directions > k still nc
        const int lo = ipow_c(nf, k);  // (compile-time once the loop over k is unrolled)
        const int hi = (dim - 1 - k) == 2 ? nc * nc : (dim - 1 - k) == 1 ? nc : 1;
        const int total = lo * nf * hi;
        for (int t = lane; t < total; t += 64) {
          const int a = t % lo, o = (t / lo) % nf, b = t / (lo * nf);
          const T *v = in + a + b * lo * nc, *row = P + o * nc;
          T s = T(0);
          for (int i = 0; i < nc; ++i) s += row[i] * v[i * lo];
          out[t] = s;
        }
      } else {
        // direction k goes nf -> nc; directions < k are nc long already, directions > k still nf
        const int lo = k == 2 ? nc * nc : k == 1 ? nc : 1;
        const int hi = ipow_c(nf, dim - 1 - k);
        const int total = lo * nc * hi;
        for (int t = lane; t < total; t += 64) {
          const int a = t % lo, o = (t / lo) % nc, b = t / (lo * nc);
          const T *v = in + a + b * lo * nf;
          T s = T(0);
#pragma unroll
          for (int i = 0; i < nf; ++i) s += P[i * nc + o] * v[i * lo];
          out[t] = s;
        }
      }
      wave_sync();
      T *tmp = in;
      in = out;
      out = tmp;
    }
    if (HN && RESTRICT && m) hn_resolve_wave<dim, true, KC>(in, W, nc, m, lane);  // C_pc^T before the atomics
#pragma unroll
    for (int j = 0; j < KF; ++j) {
      const int t = lane + 64 * j;
      if (!RESTRICT) {
        const uint32_t g = gf[j];
        if (t < NF && !(g >> 31)) dst[g] = ADD ? dst[g] + in[t] : in[t];  // one owner per fine dof: no atomics
      } else {
        const uint32_t g = gc[j];
        if (t < NC && !(g >> 31)) atomicAdd(dst + g, in[t]);  // several cells share the coarse dof; Dirichlet dofs are skipped
      }
    }
    wave_hand_over(gc, gf, next_gc, next_gf);
    mask = next_mask;
  }
}

}  // namespace

template <typename T, bool HN>
hipError_t launch_p_transfer(const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, hipStream_t st) {
  const uint32_t n = t->n_coarse_cells;
  if (n == 0) return hipSuccess;
  return dispatch_kernel<2>(t, mode, [&](auto D, auto PF, auto R, auto A) {
    hipLaunchKernelGGL((p_transfer_kernel<D(), PF(), T, R(), A(), HN>), dim3(wave_grid(n)), dim3(64 * kWaves), 0, st, (T *)dst,
                       (const T *)src, t->d_coarse.get(), t->d_fine.get(), t->d_p1.as<const T>(), n, t->degree_coarse,
                       HN ? t->d_mask.get() : nullptr, HN ? t->d_weights.as<const T>() : nullptr);
    return hipGetLastError();
  });
}
template hipError_t launch_p_transfer<double, false>(const mfgpu_transfer *, void *, const void *, TransferMode, hipStream_t);
template hipError_t launch_p_transfer<double, true>(const mfgpu_transfer *, void *, const void *, TransferMode, hipStream_t);
template hipError_t launch_p_transfer<float, false>(const mfgpu_transfer *, void *, const void *, TransferMode, hipStream_t);
template hipError_t launch_p_transfer<float, true>(const mfgpu_transfer *, void *, const void *, TransferMode, hipStream_t);

}  // namespace mfgpu
