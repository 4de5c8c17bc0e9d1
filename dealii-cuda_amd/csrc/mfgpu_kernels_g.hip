// general (non-Cartesian) geometry, the reference's default code path when
// MATRIX_FREE_UNIFORM_MESH is not defined: a full inverse Jacobian J^-1[dim][dim] per quadrature point
// (fee_gpu.cuh:235-241 get_gradient: grad_d1 = sum_d2 J[d2][d1] ghat_d2;  :275-281 submit_gradient:
// out_d1 = (sum_d2 J[d1][d2] grad_d2) * JxW;  coefficient in between, laplace_operator_gpu.h:257-260).
// Per quadrature point that is  t = M ghat  with the SYMMETRIC  M = a JxW J J^T  (6 entries in 3D), which
// mfgpu_create folds once (fold_general_kernel): 48 B per point are streamed instead of the reference's
// 72 (J^-1) + 8 (JxW) + 8 (coefficient).
//
// 3D, two-pass scatter mode; hanging nodes through the same constraint passes as apply_batches_x (template HN).  The batch machinery is apply_batches_x's (persistent
// workgroups, XCD-aware batch ranges, aliased source/accumulator array, x-pencil index runs from global
// memory, next batch's loads in flight).  The cell pipeline needs all three reference-gradient components
// at the same point, so they go through LDS: 11 barrier-separated stages per chunk,
//   S_x | S_y | S_z, D_z -> Gz | D_x -> Gx | D_y -> Gy | t = M g (pointwise, linear layout)
//       | D_z^T tz | + D_x^T tx | + D_y^T ty, S_y^T | S_z^T | S_x^T -> accumulator
// with 4 scratch arrays per cell (W/R aliased, Gx, Gy, Gz) -> 2 workgroups per CU at p=4.
// Bound: HBM -- 48 B per quadrature point = 945 MB per vmult on the C2 mesh, against 157 MB of folded
// coefficient on the Cartesian path.
//
// Width NV (mfgpu_vmult_multi): the same kernel applies the operator to a GROUP of NV = 2 or 3 vectors in one sweep;
// NV = 1 is the single apply.  One apply streams the folded metric, 48 B per quadrature point in double (+ 8 B with a
// mass term): 6 000 B per cell at p = 4 against about 1.0-1.4 KB of vector traffic.  Nothing of it depends on the
// vector, and neither do the dof list, the x-pencil index runs and the cell masks.  All of that is read ONCE per batch
// (the metric once per chunk, into the registers M[PF][6] / MM[PF]); the pointwise stage P5 and the ten contraction
// stages run once per vector on the SAME four scratch arrays.  What is per vector:
//   * the batch array (gathered source values, then the accumulator): NV arrays of nb_max doubles, each aliased
//     source/accumulator;
//   * the source pencils of every chunk in registers, U[NV][3][n] (read before the arrays become accumulators);
//   * the gathered values of the NEXT batch, SVn[NV][kGU] (in flight during the last chunk);
//   * interior dofs go to dst + v * stride, partial sums to halo buffer v (reduce_classes<T, NV> sums them).
// Transition from vector v to v + 1 inside a chunk = the transition from chunk k to k + 1: every thread ends on its
// own x-pencil of the W/R array and starts on it again, program order, no extra barrier.
//
// Budget at p = 4 in double (CH = 10 cells per chunk, nb_max <= 2304): scratch 4 x 1250 x 8 = 40 000 B, batch arrays
// NV x 18 432 B -> 76 864 B at NV = 2 (two workgroups per CU by LDS), 95 296 B at NV = 3 (one).  Registers are the tighter
// side: U, SVn and the metric of a group do not fit 256 registers per lane at p = 4 in double, so those instantiations
// are built for one wave per SIMD (g_waves_per_simd below).  DESIGN.md section 14 has the table.
#include <hip/hip_runtime.h>

#include "mfgpu_cell.h"
#include "mfgpu_kernels.h"

namespace mfgpu {

// The kernel's by-value arguments, and what vector v of a group adds to a single apply's: vec_at(A, p, v) is vector v's
// dst or src for p = A.dst, A.src, and vec_halo(A, v) its halo buffer.  A single apply (ApplyArgs<T>) has neither a
// stride nor a halo table and reads none.  (Called where the pointer is used, not once per vector: the single apply
// then loads A.dst and A.src where it always did, and compiles to the code it had before it had a width.)
template <typename T, int NV>
using GArgs = std::conditional_t<NV == 1, ApplyArgs<T>, MultiArgs<T>>;
template <typename T, typename P>
__device__ __forceinline__ P *vec_at(const ApplyArgs<T> &, P *p, int) { return p; }
template <typename T, typename P>
__device__ __forceinline__ P *vec_at(const MultiArgs<T> &A, P *p, int v) { return p + (size_t)v * A.stride; }
template <typename T>
__device__ __forceinline__ T *vec_halo(const ApplyArgs<T> &A, int) { return A.halo; }
template <typename T>
__device__ __forceinline__ T *vec_halo(const MultiArgs<T> &A, int v) { return A.halos[v]; }

// Waves per SIMD the register allocation aims at: 2 (two workgroups per CU, 256 registers per lane) for the single
// apply and where U[NV][3][n], SVn[NV][9] and the metric of a group fit that without spilling, else 1 (512 registers).
// From the resource-usage remarks of the gfx950 build: NV = 3 never fits 256 from n = 3 on; NV = 2 fits in double up to
// n = 3 (with HN: n = 2), in float up to n = 6 (with HN: n = 4).
template <int n, typename T, bool HN, int NV>
constexpr int g_waves_per_simd() {
  if (NV == 1) return 2;
  if (NV != 2) return 1;
  if (sizeof(T) == 8) return n <= (HN ? 2 : 3) ? 2 : 1;
  return n <= (HN ? 4 : 6) ? 2 : 1;
}

// MASS: the mass term int c u v.  The pointwise stage P5 is where everything per quadrature point meets in linear order:
// the values at the quadrature points w are still in their array (last read as w in P4), so P5 also replaces w by
// m .* w (m = c JxW, A.mass, loaded with the metric), and P6 starts the result from it: r = m .* w + D_z^T tz.
// MASS instantiations add into the batch accumulator one wave after the other (fixed summation order: two calls on the
// same inputs give the same bits; see cell_pipeline in mfgpu_cell.h).
template <int n, typename T, bool HN, bool MASS = false, int NV = 1>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(g_waves_per_simd<n, T, HN, NV>())))
apply_batches_g(const GArgs<T, NV> A, const Tables<T, n> tab) {
  constexpr int kBlock = 256;
  constexpr int kGU = (max_batch_dofs(kBlock) + kBlock - 1) / kBlock;
  constexpr int n2 = n * n, nd = n2 * n;
  constexpr int P = n2;
  constexpr int CH = kBlock / P;
  constexpr int CHND = CH * nd;
  constexpr int NW = (n + 1) / 2;
  constexpr int PF = (CHND + kBlock - 1) / kBlock;  // quadrature points per thread in the pointwise stage
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  // vector v's gathered source values, then its accumulator: ua + v * nb_max, always double (ds_add_f32 is far slower
  // than ds_add_f64 on gfx950, see apply_batches_x)
  double *ua = reinterpret_cast<double *>(smem_raw);
  T *Wb = reinterpret_cast<T *>(ua + (size_t)NV * A.nb_max);  // w, later the result r (aliased: w is dead after the D_y stage)
  T *Gxb = Wb + CHND;
  T *Gyb = Gxb + CHND;
  T *Gzb = Gyb + CHND;
  T *Wl = Gzb + CHND;  // hanging-node weights (HN only)

  const int tid = threadIdx.x;
  uint32_t b, bstride, bend;
  xcd_batch_range(A.batch0, A.batch_end, b, bend, bstride);
  if (b >= bend) return;

  const int lc = tid / P;
  const int pen = tid - lc * P;
  const int pa = pen % n;
  const int pb = pen / n;
  const bool lane_on = tid < CH * P;
  const int bx = n * pa + n2 * pb;  // x-pencil (y = pa, z = pb), stride 1
  const int by = pa + n2 * pb;      // y-pencil (x = pa, z = pb), stride n
  const int bz = pa + n * pb;       // z-pencil (x = pa, y = pb), stride n2
  T *Wc = Wb + lc * nd, *Gxc = Gxb + lc * nd, *Gyc = Gyb + lc * nd, *Gzc = Gzb + lc * nd;

  auto lane = [&]() {  // opaque copy of the thread index: keeps hipcc from hoisting tid + j*256 constants
    int l = tid;
    asm volatile("" : "+v"(l));
    return l;
  };
  uint32_t c0, d0, hoff;
  int nb, ncell, nint;
  auto load_meta = [&](uint32_t bb, uint32_t &c0_, int &ncell_, uint32_t &d0_, int &nb_, int &nint_, uint32_t &hoff_) {
    c0_ = A.batch_cell_off[bb];
    ncell_ = (int)(A.batch_cell_off[bb + 1] - c0_);
    d0_ = A.batch_dof_off[bb];
    nb_ = (int)(A.batch_dof_off[bb + 1] - d0_);
    nint_ = (int)A.batch_nint[bb];
    hoff_ = A.halo_off[bb];
  };
  auto load_dofs = [&](uint32_t d0_, int nb_, uint32_t (&g_)[kGU]) {
    const int l = lane();
    const uint32_t *bd = A.bdofs + d0_;
#pragma unroll
    for (int j = 0; j < kGU; ++j) {
      const int t = l + j * kBlock;
      g_[j] = stream_load(bd + (t < nb_ ? t : nb_ - 1));
    }
  };
  // The per-vector loops, here and below: `const int v = NV == 1 ? 0 : iv` and the closing `if (NV == 1) break` are
  // folded by the compiler's front end, so the single apply is straight-line code on the constant v = 0 before the
  // optimiser sees it (it compiles to what it was as a kernel of its own); at NV > 1 they are plain unrolled loops.  A
  // plain loop of one trip goes away too late: the hanging-node instantiations then need up to 70 more registers.
  auto load_src = [&](const uint32_t (&g_)[kGU], T (&sv_)[NV][kGU]) {
#pragma unroll
    for (int iv = 0; iv < NV; ++iv) {
      const int v = NV == 1 ? 0 : iv;
#pragma unroll
      for (int j = 0; j < kGU; ++j) sv_[v][j] = vec_at(A, A.src, v)[g_[j] & 0x7fffffffu];
      if (NV == 1) break;
    }
  };
  auto load_ix = [&](uint32_t c0_, int ncell_, uint32_t (&ix_)[kMaxChunks][NW]) {
    const uint32_t *lx = reinterpret_cast<const uint32_t *>(A.lmapx);
#pragma unroll
    for (int k = 0; k < kMaxChunks; ++k) {
      int cell = k * CH + lc;
      cell = cell < ncell_ ? cell : ncell_ - 1;
      const uint32_t *p = lx + ((size_t)(c0_ + cell) * P + (lane_on ? pen : 0)) * NW;
#pragma unroll
      for (int q = 0; q < NW; ++q) ix_[k][q] = stream_load(p + q);
    }
  };
  // folded metric M = a JxW J J^T of this thread's points of a chunk, stored [cell][e][q] with
  // e = {00, 01, 02, 11, 12, 22}: for one entry the lanes of a wave read consecutive doubles; read once for the NV vectors
  T M[PF][6];
  T MM[MASS ? PF : 1];
  auto load_metric = [&](uint32_t cell0, int cnt) {
    const T *mg = A.coef + (size_t)cell0 * nd * 6;
    const int l = lane();
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      int i = l + j * kBlock;
      i = i < cnt ? i : cnt - 1;
      const int cl = i / nd, q = i - cl * nd;
      const T *p = mg + (size_t)cl * (6 * nd) + q;
#pragma unroll
      for (int e = 0; e < 6; ++e) M[j][e] = stream_load(p + e * nd);
      if (MASS) MM[j] = stream_load(A.mass + (size_t)cell0 * nd + i);
    }
  };
  auto chunk_count = [&](int ncell_, int base_) { return (ncell_ - base_ < CH ? ncell_ - base_ : CH) * nd; };

  if (HN)
    for (int t = tid; t < n2; t += kBlock) Wl[t] = A.hn_weights[t];
  uint32_t G[kGU];
  T SV[NV][kGU];
  uint32_t IX[kMaxChunks][NW];
  load_meta(b, c0, ncell, d0, nb, nint, hoff);
  load_dofs(d0, nb, G);
  load_ix(c0, ncell, IX);
  load_src(G, SV);
  while (true) {
    // ---- 1. gather -> LDS, one array per vector; bit 31 of a dof entry = constrained row: reads as 0, and the owning
    // batch writes dst_v = src_v (constraint_handler_gpu.cu:258-259,286)
    {
      const int l = lane();
#pragma unroll
      for (int iv = 0; iv < NV; ++iv) {
        const int v = NV == 1 ? 0 : iv;
        double *ul = ua + (size_t)v * A.nb_max + l;
#pragma unroll
        for (int j = 0; j < kGU; ++j) {
          const bool con = (G[j] >> 31) != 0;
          if (l < nb - j * kBlock) {
            ul[j * kBlock] = con ? 0.0 : (double)SV[v][j];
            if (con && l < nint - j * kBlock) {
              T *d = vec_at(A, A.dst, v) + (G[j] & 0x7fffffffu);
              *d = A.add ? *d + SV[v][j] : SV[v][j];
            }
          }
        }
        if (NV == 1) break;
      }
    }
    const uint32_t bn = b + bstride;
    const bool has_nb = bn < bend;
    uint32_t c0n = c0, d0n = d0, hoffn = hoff;
    int nbn = nb, ncelln = ncell, nintn = nint;
    uint32_t Gn[kGU];
    T SVn[NV][kGU];
    uint32_t IXn[kMaxChunks][NW];
    if (has_nb) {
      load_meta(bn, c0n, ncelln, d0n, nbn, nintn, hoffn);
      load_dofs(d0n, nbn, Gn);
    }
    __syncthreads();
    // ---- 2. source pencils of every chunk and vector -> registers; afterwards the arrays are the accumulators
    T U[NV][kMaxChunks][n];
#pragma unroll
    for (int iv = 0; iv < NV; ++iv) {
      const int v = NV == 1 ? 0 : iv;
      const double *uv = ua + (size_t)v * A.nb_max;
#pragma unroll
      for (int k = 0; k < kMaxChunks; ++k)
        if (k * CH < ncell) {
#pragma unroll
          for (int i = 0; i < n; ++i) U[v][k][i] = (T)uv[ix_at<n>(IX[k], i)];
        }
      if (NV == 1) break;
    }
    __syncthreads();
    {
      const int l = lane();
#pragma unroll
      for (int iv = 0; iv < NV; ++iv) {
        const int v = NV == 1 ? 0 : iv;
        double *ul = ua + (size_t)v * A.nb_max + l;
#pragma unroll
        for (int j = 0; j < kGU; ++j)
          if (l < nb - j * kBlock) ul[j * kBlock] = 0.0;
        if (NV == 1) break;
      }
    }

    // ---- 3. cells: metric and mask once per chunk, the stages once per vector
#pragma unroll
    for (int k = 0; k < kMaxChunks; ++k) {
      const int base = k * CH;
      if (base >= ncell) continue;  // uniform
      const bool act = lane_on && (base + lc < ncell);
      const int cnt = chunk_count(ncell, base);
      load_metric(c0 + base, cnt);  // consumed six stages later, then again by every further vector
      if (k == kMaxChunks - 1 && has_nb) load_src(Gn, SVn);
      if (k == 1 && has_nb) load_ix(c0n, ncelln, IXn);
      unsigned mask = 0;
      bool any_mask = false;
      if (HN) {
        if (act) mask = A.cmask[(size_t)c0 + base + lc];
        any_mask = __syncthreads_or(mask != 0) != 0;
      }
#pragma unroll
      for (int iv = 0; iv < NV; ++iv) {
        const int v = NV == 1 ? 0 : iv;
        double *acc = ua + (size_t)v * A.nb_max;
        T u[n], vv[n], w[n], g[n];
        if (HN && any_mask) {
          // resolve_hanging_nodes_shmem<NOTRANSPOSE>: x, then y, then z (hanging_nodes.cuh:767-777); only the
          // pencils on a constrained face or edge take the y / z round trips
          bool type;
          if (act) {
            if (mask && hn_flag3<n, 0>(mask, pa, pb, type)) hn_pencil<n, T, false, true>(Wl, type, U[v][k]);
            lds_put<n>(Wc + bx, 1, U[v][k]);
          }
          __syncthreads();
          if (act && mask && hn_flag3<n, 1>(mask, pb, pa, type)) {
            lds_load<n>(Wc + by, n, u);
            hn_pencil<n, T, false, true>(Wl, type, u);
            lds_put<n>(Wc + by, n, u);
          }
          __syncthreads();
          if (act && mask && hn_flag3<n, 2>(mask, pa, pb, type)) {
            lds_load<n>(Wc + bz, n2, u);
            hn_pencil<n, T, false, true>(Wl, type, u);
            lds_put<n>(Wc + bz, n2, u);
          }
          __syncthreads();
          if (act) lds_load<n>(Wc + bx, 1, U[v][k]);
        }
        // P0: interpolate along x
        if (act) {
          mvt<n, 1>(tab.S, U[v][k], vv);
          lds_put<n>(Wc + bx, 1, vv);
        }
        __syncthreads();
        // P1: interpolate along y
        if (act) {
          lds_load<n>(Wc + by, n, u);
          mvt<n, 1>(tab.S, u, vv);
          lds_put<n>(Wc + by, n, vv);
        }
        __syncthreads();
        // P2: interpolate along z -> values at the quadrature points; z-derivative
        if (act) {
          lds_load<n>(Wc + bz, n2, u);
          mvt<n, 1>(tab.S, u, w);
          mv<n, -1>(tab.Dt, w, g);
          lds_put<n>(Wc + bz, n2, w);
          lds_put<n>(Gzc + bz, n2, g);
        }
        __syncthreads();
        // P3: x-derivative
        if (act) {
          lds_load<n>(Wc + bx, 1, w);
          mv<n, -1>(tab.Dt, w, g);
          lds_put<n>(Gxc + bx, 1, g);
        }
        __syncthreads();
        // P4: y-derivative (last read of w: the array becomes the result r)
        if (act) {
          lds_load<n>(Wc + by, n, w);
          mv<n, -1>(tab.Dt, w, g);
          lds_put<n>(Gyc + by, n, g);
        }
        __syncthreads();
        // P5: quadrature-point operation t = M ghat with the chunk's metric registers, points in linear order (the
        // chunk's cells are contiguous)
        {
          const int l = lane();
#pragma unroll
          for (int j = 0; j < PF; ++j) {
            if (l < cnt - j * kBlock) {
              const int i = l + j * kBlock;
              const T gx = Gxb[i], gy = Gyb[i], gz = Gzb[i];
              Gxb[i] = fma(M[j][0], gx, fma(M[j][1], gy, M[j][2] * gz));
              Gyb[i] = fma(M[j][1], gx, fma(M[j][3], gy, M[j][4] * gz));
              Gzb[i] = fma(M[j][2], gx, fma(M[j][4], gy, M[j][5] * gz));
              if (MASS) Wb[i] = MM[j] * Wb[i];
            }
          }
        }
        __syncthreads();
        // P6: r = D_z^T tz
        if (act) {
          lds_load<n>(Gzc + bz, n2, g);
          mvt<n, -1>(tab.Dt, g, vv);
          if (MASS) {
            lds_load<n>(Wc + bz, n2, u);
#pragma unroll
            for (int s = 0; s < n; ++s) vv[s] += u[s];
          }
          lds_put<n>(Wc + bz, n2, vv);
        }
        __syncthreads();
        // P7: r += D_x^T tx
        if (act) {
          lds_load<n>(Gxc + bx, 1, g);
          lds_load<n>(Wc + bx, 1, u);
          mvt<n, -1>(tab.Dt, g, vv);
#pragma unroll
          for (int s = 0; s < n; ++s) vv[s] += u[s];
          lds_put<n>(Wc + bx, 1, vv);
        }
        __syncthreads();
        // P8: r += D_y^T ty, then S^T along y
        if (act) {
          lds_load<n>(Gyc + by, n, g);
          lds_load<n>(Wc + by, n, u);
          mvt<n, -1>(tab.Dt, g, w);
#pragma unroll
          for (int s = 0; s < n; ++s) w[s] += u[s];
          mv<n, 1>(tab.S, w, vv);
          lds_put<n>(Wc + by, n, vv);
        }
        __syncthreads();
        // P9: S^T along z
        if (act) {
          lds_load<n>(Wc + bz, n2, u);
          mv<n, 1>(tab.S, u, vv);
          lds_put<n>(Wc + bz, n2, vv);
        }
        __syncthreads();
        // P10: S^T along x, add into vector v's accumulator (the thread re-uses its own pencil of the array in the
        // next vector's / chunk's first stage: program order, no barrier needed)
        if (act) {
          lds_load<n>(Wc + bx, 1, u);
          mv<n, 1>(tab.S, u, vv);
        }
        if (HN && any_mask) {
          // resolve_hanging_nodes_shmem<TRANSPOSE>: the passes commute; y, z, then x (the index set's pencil)
          bool type;
          if (act) lds_put<n>(Wc + bx, 1, vv);
          __syncthreads();
          if (act && mask && hn_flag3<n, 1>(mask, pb, pa, type)) {
            lds_load<n>(Wc + by, n, vv);
            hn_pencil<n, T, true, true>(Wl, type, vv);
            lds_put<n>(Wc + by, n, vv);
          }
          __syncthreads();
          if (act && mask && hn_flag3<n, 2>(mask, pa, pb, type)) {
            lds_load<n>(Wc + bz, n2, vv);
            hn_pencil<n, T, true, true>(Wl, type, vv);
            lds_put<n>(Wc + bz, n2, vv);
          }
          __syncthreads();
          if (act) {
            lds_load<n>(Wc + bx, 1, vv);
            if (mask && hn_flag3<n, 0>(mask, pa, pb, type)) hn_pencil<n, T, true, true>(Wl, type, vv);
          }
        }
        if (MASS) {
          for (int wv = 0; wv < 4; ++wv) {  // (256 threads; uniform: every thread passes every barrier)
            if (act && (tid >> 6) == wv) {
#pragma unroll
              for (int i = 0; i < n; ++i) lds_add(&acc[ix_at<n>(IX[k], i)], (double)vv[i]);
            }
            __syncthreads();
          }
        } else if (act) {
#pragma unroll
          for (int i = 0; i < n; ++i) lds_add(&acc[ix_at<n>(IX[k], i)], (double)vv[i]);
        }
        if (NV == 1) break;
      }
    }
    if (has_nb && ncell <= (kMaxChunks - 1) * CH) {  // short batch (ragged meshes): no overlap
      load_src(Gn, SVn);
      if (ncell <= CH) load_ix(c0n, ncelln, IXn);
    }
    __syncthreads();

    // ---- 4. scatter per vector: interior dofs -> dst_v, partial sums of shared dofs -> halo buffer v (the reduce pass
    // sums them)
    {
      const int l = lane();
#pragma unroll
      for (int iv = 0; iv < NV; ++iv) {
        const int v = NV == 1 ? 0 : iv;
        const double *ul = ua + (size_t)v * A.nb_max + l;
        T *hl = vec_halo(A, v) + hoff + l - nint;
        T old[kGU];
        if (A.add) {
#pragma unroll
          for (int j = 0; j < kGU; ++j) old[j] = vec_at(A, A.dst, v)[G[j] & 0x7fffffffu];
        }
#pragma unroll
        for (int j = 0; j < kGU; ++j) {
          if (l < nint - j * kBlock) {
            if (!(G[j] >> 31)) vec_at(A, A.dst, v)[G[j]] = A.add ? old[j] + (T)ul[j * kBlock] : (T)ul[j * kBlock];
          } else if (l < nb - j * kBlock) {
            hl[j * kBlock] = (T)ul[j * kBlock];
          }
        }
        if (NV == 1) break;
      }
    }
    if (!has_nb) break;
    b = bn;
    c0 = c0n;
    ncell = ncelln;
    d0 = d0n;
    nb = nbn;
    nint = nintn;
    hoff = hoffn;
#pragma unroll
    for (int j = 0; j < kGU; ++j) {
      G[j] = Gn[j];
#pragma unroll
      for (int iv = 0; iv < NV; ++iv) {
        const int v = NV == 1 ? 0 : iv;
        SV[v][j] = SVn[v][j];
        if (NV == 1) break;
      }
    }
#pragma unroll
    for (int k = 0; k < kMaxChunks; ++k)
#pragma unroll
      for (int q = 0; q < NW; ++q) IX[k][q] = IXn[k][q];
  }
}

// M = a JxW J J^T per quadrature point, plan cell order, [cell][entry][q]; J = inv_jac[cell][q] row-major J[d1][d2]
template <typename T>
__global__ void fold_general_kernel(T *M, const T *coef, const T *jxw, const T *jinv, const uint32_t *order,
                                    uint32_t n_cells, uint32_t nd) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)n_cells * nd) return;
  const uint32_t cell = (uint32_t)(i / nd), q = (uint32_t)(i - (size_t)cell * nd);
  const size_t s = (size_t)order[cell] * nd + q;
  const T *J = jinv + s * 9;
  const T a = coef[s] * jxw[s];
  T *m = M + (size_t)cell * (6 * nd) + q;  // [cell][e][q]
  int e = 0;
  for (int d1 = 0; d1 < 3; ++d1)
    for (int d2 = d1; d2 < 3; ++d2)
      m[(e++) * nd] = a * (J[3 * d1] * J[3 * d2] + J[3 * d1 + 1] * J[3 * d2 + 1] + J[3 * d1 + 2] * J[3 * d2 + 2]);
}

template <int n, typename T>
static size_t g_lds_bytes(uint32_t nb_max, int nv) {
  constexpr int nd = n * n * n;
  constexpr int CH = 256 / (n * n);
  return (size_t)nv * nb_max * sizeof(double) + (size_t)(4 * CH * nd + n * n) * sizeof(T);
}

// The only place that names the family's instantiations: with Args = ApplyArgs<T> the single apply that kernel_exists
// admits (nv is 1), with MultiArgs<T> the fused one of width nv that fused_kernel_exists admits
template <typename T, typename Args>
hipError_t g_bind_width(int n, bool hn, bool sh, bool mass, int nv, uint32_t nb_max, CellKernel<T, Args> *k) {
  return dispatch_instantiation(n, [&](auto N, auto W3, auto HN, auto SH, auto MASS) {
    constexpr int n_ = N;
    constexpr int NV = std::is_same_v<Args, ApplyArgs<T>> ? 1 : W3 ? 3 : 2;
    if constexpr (NV == 1 ? kernel_exists(BatchKernel::g, n_, number_type_of<T>, HN, SH, MASS)
                          : !SH && fused_kernel_exists(BatchKernel::g, n_, number_type_of<T>, HN, MASS, NV)) {
      constexpr auto K = apply_batches_g<n_, T, HN, MASS, NV>;
      const size_t lds = g_lds_bytes<n_, T>(nb_max, NV);
      k->lds = lds;
      if (NV > 1 && lds > kMaxLdsBytes) return hipErrorInvalidValue;  // (the plan's batches are too large for the width)
      return bind_cell_kernel<T, 256, K, K, make_tables<T, n_>>(lds, k);
    } else
      return hipErrorInvalidValue;
  }, nv == 3, hn, sh, mass);
}

template <typename T>
hipError_t g_bind(int, int n, bool hn, bool, bool sh, bool mass, uint32_t nb_max, CellKernel<T> *k) {
  return g_bind_width(n, hn, sh, mass, 1, nb_max, k);
}

template <typename T>
hipError_t fold_general_launch(T *M, const T *coef, const T *jxw, const T *jinv, const uint32_t *order,
                               uint32_t n_cells, uint32_t nd, hipStream_t st) {
  const size_t tot = (size_t)n_cells * nd;
  hipLaunchKernelGGL(fold_general_kernel<T>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, M, coef, jxw, jinv,
                     order, n_cells, nd);
  return hipGetLastError();
}

#define INST(T)                                                                                                  \
  template hipError_t g_bind<T>(int, int, bool, bool, bool, bool, uint32_t, CellKernel<T> *);                    \
  template hipError_t g_bind_width<T>(int, bool, bool, bool, int, uint32_t, MultiKernel<T> *);                   \
  template hipError_t fold_general_launch<T>(T *, const T *, const T *, const T *, const uint32_t *, uint32_t, \
                                             uint32_t, hipStream_t);
INST(double)
INST(float)

}  // namespace mfgpu
