// What the one-wave-per-cell transfer kernels share (mfgpu_transfer_p.hip: between two degrees on one mesh;
// mfgpu_transfer_h.hip: between two leaf meshes at one degree): the stage fence of a wave that keeps its arrays in its
// own slice of LDS, the run-time-n forms of the hanging-node pencil flags, and resolve_hanging_nodes on one wave's cell.
// The flag functions are __host__ __device__: the host's owner rule (p_owner_list) and the kernels read the same code.
#ifndef MFGPU_TRANSFER_HN_H
#define MFGPU_TRANSFER_HN_H

#include <hip/hip_runtime.h>

namespace mfgpu {

// LDS accesses of one wave execute in order; this keeps the compiler from moving them across a stage boundary
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Run-time-n form of hn_flag3 / hn_flag2 (mfgpu_cell.h), for the host's owner rule and the kernel alike: does
// resolve_hanging_nodes interpolate the pencil along `dir` whose other coordinates are f1 (direction (dir+1)%3; in 2D
// the other direction) and f2 (direction (dir+2)%3), and from which half of the parent's line (type)?
__host__ __device__ inline bool hn_flag_rt(int dim, int p, unsigned m, int dir, int f1, int f2, bool &type) {
  type = (m >> dir) & 1u;  // TYPE x, y, z: bits 0..2; FACE x, y, z: bits 3..5; EDGE xy, yz, zx: bits 6..8
  if (dim == 2) {
    const int o = 1 - dir;
    const bool on = ((m >> o) & 1u) ? f1 == 0 : f1 == p;
    return ((m >> (3 + o)) & 1u) && on;
  }
  const int d1 = (dir + 1) % 3, d2 = (dir + 2) % 3;
  const bool on1 = ((m >> d1) & 1u) ? f1 == 0 : f1 == p;
  const bool on2 = ((m >> d2) & 1u) ? f2 == 0 : f2 == p;
  const int edge = dir == 0 ? 7 : dir == 1 ? 8 : 6;  // the edge along dir: yz, zx, xy
  return (((m >> (3 + d1)) & 1u) && on1) || (((m >> (3 + d2)) & 1u) && on2) || (((m >> edge) & 1u) && on1 && on2);
}
// the same for the pencil along `dir` through local position t of n^dim (x fastest); q = t's coordinate along dir
__host__ __device__ inline bool hn_flag_at(int dim, int n, unsigned m, int dir, int t, bool &type, int &q) {
  const int c[3] = {t % n, (t / n) % n, dim == 3 ? t / (n * n) : 0};
  q = c[dir];
  return dim == 2 ? hn_flag_rt(2, n - 1, m, dir, c[1 - dir], 0, type)
                  : hn_flag_rt(3, n - 1, m, dir, c[(dir + 1) % 3], c[(dir + 2) % 3], type);
}
// the bits of a mask that make resolve_hanging_nodes touch pencils along dir (none set: the pass is the identity)
__host__ __device__ inline unsigned hn_dir_bits(int dim, int dir) {
  if (dim == 2) return 1u << (3 + 1 - dir);
  return (1u << (3 + (dir + 1) % 3)) | (1u << (3 + (dir + 2) % 3)) | (1u << (dir == 0 ? 7 : dir == 1 ? 8 : 6));
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
