// Run-time-n forms of the hanging-node pencil flags hn_flag3 / hn_flag2 (mfgpu_cell.h).  The host's owner rule and
// constrained_position (mfgpu_transfer_build.cpp) and the wave-per-cell transfer kernels (mfgpu_transfer_wave.h) read
// this one text: it compiles with and without HIP.
#ifndef MFGPU_HN_FLAGS_H
#define MFGPU_HN_FLAGS_H

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MFGPU_HD __host__ __device__
#else
#define MFGPU_HD
#endif

namespace mfgpu {

// does resolve_hanging_nodes interpolate the pencil along `dir` whose other coordinates are f1 (direction (dir+1)%3; in
// 2D the other direction) and f2 (direction (dir+2)%3), and from which half of the parent's line (type)?
MFGPU_HD inline bool hn_flag_rt(int dim, int p, unsigned m, int dir, int f1, int f2, bool &type) {
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
MFGPU_HD inline bool hn_flag_at(int dim, int n, unsigned m, int dir, int t, bool &type, int &q) {
  const int c[3] = {t % n, (t / n) % n, dim == 3 ? t / (n * n) : 0};
  q = c[dir];
  return dim == 2 ? hn_flag_rt(2, n - 1, m, dir, c[1 - dir], 0, type)
                  : hn_flag_rt(3, n - 1, m, dir, c[(dir + 1) % 3], c[(dir + 2) % 3], type);
}
// the bits of a mask that make resolve_hanging_nodes touch pencils along dir (none set: the pass is the identity)
MFGPU_HD inline unsigned hn_dir_bits(int dim, int dir) {
  if (dim == 2) return 1u << (3 + 1 - dir);
  return (1u << (3 + (dir + 1) % 3)) | (1u << (3 + (dir + 2) % 3)) | (1u << (dir == 0 ? 7 : dir == 1 ? 8 : 6));
}

}  // namespace mfgpu

#endif
