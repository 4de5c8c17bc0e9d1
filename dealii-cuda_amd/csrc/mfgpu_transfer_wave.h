// What the one-wave-per-cell transfer kernels share (mfgpu_transfer_p.hip: between two degrees on one mesh;
// mfgpu_transfer_h.hip: between two leaf meshes at one degree): the grid, the stage fence of a wave that keeps its arrays
// in its own slice of LDS, the hand-over of the prefetched index lists, and resolve_hanging_nodes on one wave's cell.  How a cell's coarse list is addressed, the
// contractions and the place of resolve_hanging_nodes differ between the two kernels and stay with them.
#ifndef MFGPU_TRANSFER_WAVE_H
#define MFGPU_TRANSFER_WAVE_H

#include <hip/hip_runtime.h>

#include "mfgpu_hn_flags.h"
#include "mfgpu_transfer.h"

namespace mfgpu {

constexpr int kWaves = 4;            // cells per workgroup pass
constexpr unsigned kMaxGrid = 2048;  // workgroups: 8 per CU on 256 CUs; more cells than 4 * kMaxGrid take further passes
inline unsigned wave_grid(uint32_t n_cells) {
  const unsigned groups = (n_cells + kWaves - 1) / kWaves;
  return groups < kMaxGrid ? groups : kMaxGrid;
}

// A cell's two index lists sit in registers: entry lane + 64 j in slot j, past the end (or no cell): bit 31, "skip".
// The kernels request them one cell ahead, gather and scatter through them in their own text: behind a function each of
// these phases compiles to a different instruction stream in one kernel or both (profiles/r19_notes.md).
// the prefetched lists become the current ones
template <int K>
__device__ __forceinline__ void wave_hand_over(uint32_t (&gc)[K], uint32_t (&gf)[K], const uint32_t (&next_gc)[K],
                                               const uint32_t (&next_gf)[K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    gc[j] = next_gc[j];
    gf[j] = next_gf[j];
  }
}

// LDS accesses of one wave execute in order; this keeps the compiler from moving them across a stage boundary
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// resolve_hanging_nodes (TR: its transpose) at run-time n = pc + 1 on the n^dim values v of ONE wave's cell, with the
// weight matrix W[n * n] in LDS: the passes x, y, z of oracle hn_resolve (transpose: z, y, x, so that it is the exact
// transpose).  The pencils of one pass are disjoint, but an output reads its whole pencil: every lane computes the new
// values of its entries (lane + 64 j) into registers, then the wave writes them.  KC slots cover pf^dim >= n^dim entries.
template <int dim, bool TR, int KC, typename T>
__device__ __forceinline__ void hn_resolve_wave(T *v, const T *W, int n, unsigned mask, int lane) {
  const int NC = dim == 3 ? n * n * n : n * n;
#pragma unroll
  for (int s = 0; s < dim; ++s) {
    const int dir = TR ? dim - 1 - s : s;
    if (!(mask & hn_dir_bits(dim, dir))) continue;  // (uniform)
    const int stride = dir == 0 ? 1 : dir == 1 ? n : n * n;
    T r[KC];
    unsigned hit = 0;
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      const int t = lane + 64 * j;
      bool type;
      int q;
      r[j] = T(0);
      if (t < NC && hn_flag_at(dim, n, mask, dir, t, type, q)) {
        hit |= 1u << j;
        // type: w = TR ? W[i][q] : W[q][i]; otherwise the mirrored entry W[p-i][p-q] / W[p-q][p-i] (hn_pencil), which
        // sits at n * n - 1 - (the index of the unmirrored one)
        const T *w = type ? W + (TR ? q : q * n) : W + (TR ? n * n - 1 - q : n * n - 1 - q * n);
        const int ws = (TR ? n : 1) * (type ? 1 : -1);
        const T *x = v + (t - q * stride);
        T sum = T(0);
        for (int i = 0; i < n; ++i) sum += w[i * ws] * x[i * stride];
        r[j] = sum;
      }
    }
    wave_sync();
#pragma unroll
    for (int j = 0; j < KC; ++j)
      if ((hit >> j) & 1u) v[lane + 64 * j] = r[j];
    wave_sync();
  }
}

}  // namespace mfgpu

#endif
