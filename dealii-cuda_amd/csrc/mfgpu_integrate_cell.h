// Device-side building blocks of the integrator's one-wave-per-cell kernels, shared by mfgpu_integrate.hip and
// mfgpu_points.hip: the layout of the 1D tables, the sum-factorised tensor passes in LDS and the hanging-node
// resolution on the LDS values of one cell.  Included by .hip files only.
#ifndef MFGPU_INTEGRATE_CELL_H
#define MFGPU_INTEGRATE_CELL_H

#include <hip/hip_runtime.h>

#include "mfgpu_cell.h"

namespace mfgpu {

constexpr int cpow(int a, int e) { return e == 0 ? 1 : a * cpow(a, e - 1); }

// 1D tables (row-major [out][in]), one device array, copied to LDS by every workgroup
template <int N>
struct Tab {
  static constexpr int M = N + 1;
  static constexpr int SE = 0;              // [q][i] = phi_i(x_q)      nodal -> QGauss(N) values
  static constexpr int GE = SE + N * N;     // [q][i] = phi_i'(x_q)     nodal -> QGauss(N) derivatives
  static constexpr int SI = GE + N * N;     // [i][q] = phi_i(x_q)      integration of values
  static constexpr int GI = SI + N * N;     // [i][q] = phi_i'(x_q)     integration against derivatives
  static constexpr int E = GI + N * N;      // [k][i] = phi_i(y_k)      nodal -> QGauss(M) values
  static constexpr int LV = E + M * N;      // [k][q] = L_q(y_k)        Lagrange basis on QGauss(N) points
  static constexpr int LD = LV + M * N;     // [k][q] = L_q'(y_k)
  static constexpr int WM = LD + M * N;     // [k]    QGauss(M) weights on [0,1]
  static constexpr int W = WM + M;          // [i][j] hanging-node weights
  static constexpr int size = W + N * N;
};

// ---- sum factorisation in LDS
// out = M (NB x NA) applied along direction `dir` of `in` (extents E0, E1, E2, x fastest; E_dir == NA)
template <int dir, int NA, int NB, int E0, int E1, int E2>
__device__ __forceinline__ void tpass(const double *__restrict__ in, double *__restrict__ out,
                                      const double *__restrict__ M) {
  constexpr int O0 = dir == 0 ? NB : E0, O1 = dir == 1 ? NB : E1, O2 = dir == 2 ? NB : E2;
  constexpr int stride = dir == 0 ? 1 : dir == 1 ? E0 : E0 * E1;
  for (int t = threadIdx.x; t < O0 * O1 * O2; t += 64) {
    const int x = t % O0, y = (t / O0) % O1, z = t / (O0 * O1);
    const int k = dir == 0 ? x : dir == 1 ? y : z;
    const double *src = in + (dir == 0 ? 0 : x) + E0 * ((dir == 1 ? 0 : y) + E1 * (dir == 2 ? 0 : z));
    double s = 0;
#pragma unroll
    for (int i = 0; i < NA; ++i) s = fma(M[k * NA + i], src[i * stride], s);
    out[t] = s;
  }
  __syncthreads();
}

// out = (Mz x My x Mx) in, NA^dim -> NB^dim, through the temporaries t1, t2 (NB^dim each)
template <int dim, int NA, int NB>
__device__ __forceinline__ void tensor(const double *in, double *out, const double *Mx, const double *My,
                                       const double *Mz, double *t1, double *t2) {
  __syncthreads();
  if constexpr (dim == 2) {
    tpass<0, NA, NB, NA, NA, 1>(in, t1, Mx);
    tpass<1, NA, NB, NB, NA, 1>(t1, out, My);
  } else {
    tpass<0, NA, NB, NA, NA, NA>(in, t1, Mx);
    tpass<1, NA, NB, NB, NA, NA>(t1, t2, My);
    tpass<2, NA, NB, NB, NB, NA>(t2, out, Mz);
  }
}

// resolve_hanging_nodes on the LDS values of one cell, directions x, y(, z) in that order (hn_resolve)
template <int dim, int N, bool TR, int dir>
__device__ __forceinline__ void hn_dir(double *v, unsigned mask, const double *W) {
  constexpr int d1 = (dir + 1) % 3, d2 = (dir + 2) % 3;
  for (int t = threadIdx.x; t < cpow(N, dim - 1); t += 64) {
    bool type = false, flag;
    int base;
    if constexpr (dim == 3) {
      const int a = t % N, b = t / N;
      flag = hn_flag3<N, dir>(mask, a, b, type);
      base = a * cpow(N, d1) + b * cpow(N, d2);
    } else {
      flag = hn_flag2<N, dir>(mask, t, type);
      base = t * cpow(N, 1 - dir);
    }
    if (flag) {
      double p[N];
#pragma unroll
      for (int i = 0; i < N; ++i) p[i] = v[base + i * cpow(N, dir)];
      hn_pencil<N, double, TR>(W, type, p);
#pragma unroll
      for (int i = 0; i < N; ++i) v[base + i * cpow(N, dir)] = p[i];
    }
  }
  __syncthreads();
}

template <int dim, int N, bool TR>
__device__ __forceinline__ void hn_resolve(double *v, unsigned mask, const double *W) {
  __syncthreads();
  hn_dir<dim, N, TR, 0>(v, mask, W);
  hn_dir<dim, N, TR, 1>(v, mask, W);
  if constexpr (dim == 3) hn_dir<dim, N, TR, 2>(v, mask, W);
}

template <int N>
__device__ __forceinline__ void load_tab(double *tab, const double *g) {
  for (int i = threadIdx.x; i < Tab<N>::size; i += 64) tab[i] = g[i];
}

template <int dim, int N>
__device__ __forceinline__ void load_qpts(double *Q, const double *qpts, uint32_t c) {
  constexpr int ND = cpow(N, dim);
  for (int t = threadIdx.x; t < ND * dim; t += 64) {
    const int q = t / dim, d = t - q * dim;
    Q[d * ND + q] = qpts[(size_t)c * ND * dim + t];
  }
}

}  // namespace mfgpu
#endif
