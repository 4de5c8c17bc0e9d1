// Kernel argument structs + launcher declarations (implemented in the mfgpu_kernels*.hip files).
#ifndef MFGPU_KERNELS_H
#define MFGPU_KERNELS_H

#include <hip/hip_runtime.h>

#include <type_traits>

#include "mfgpu_device.h"
#include "mfgpu_internal.h"

namespace mfgpu {

template <typename T>
struct ApplyArgs {
  const uint32_t *batch_cell_off;
  const uint32_t *batch_dof_off;
  const uint32_t *bdofs;
  const uint8_t *bflags;
  const uint16_t *lmap;
  const uint16_t *lmapx;  // apply_batches_x: x-pencil index runs padded to 32-bit words, or nullptr
  const uint16_t *perm;   // apply_batches_x: [2][256] lane -> pencil id of the y- and the z-stage (nullptr: hanging nodes)
  // apply_planes3: fixed-size per-batch records (nullptr otherwise)
  const uint32_t *bdofsp;  // [p_kgu(n) * 64] dof list: p_ji(n) slots of interior dofs, p_hs(n) slots of pass-2 dofs
  const uint32_t *idxp;    // [(n*n+1)/2 words][NT tasks] packed 16-bit byte offsets into the batch array
  const T *coefp;          // [n*n rows][NT tasks] folded coefficient
  // apply_planes3<HN> (batches hn_batch0 ..): fixed-size records of p_hn_rows(n) x 64 words (mfgpu_internal.h)
  const uint32_t *hnrec;
  const uint32_t *hn_slot;  // per plane batch: index of its record in hnrec, or 0xffffffff (cells without a mask)
  const T *coef;          // folded a*J0^2*JxW (apply_batches_g: the 6 entries of a*JxW*J*J^T), plan cell order
  const uint32_t *cmask;  // plan cell order, or nullptr
  const T *hn_weights;    // [n*n] W[i*n+j] (device), or nullptr
  const T *tabS, *tabDt;  // apply_batches_g2: full 1D tables S[i*n+q], Dt[q*n+t] on the device (nullptr otherwise)
  const uint32_t *batch_nint;  // two-pass mode: interior dofs per batch
  const uint32_t *halo_off;    // two-pass mode: first halo slot per batch
  T *halo;                     // two-pass mode: partial sums of shared dofs
  T *dst;
  const T *src;
  uint32_t batch0;     // first batch of this launch (colour)
  uint32_t batch_end;  // one past the last batch of this launch
  uint32_t hole0 = 0xffffffffu, hole_len = 0;  // plane kernels: batches [hole0, hole0 + hole_len) are skipped
  uint32_t nb_max;  // LDS layout: max dofs per batch
  int add;          // vmult_add semantics
  unsigned long long *stamps;  // diagnostic build only (MFGPU_STAMPS), else nullptr
  int dbg;                     // diagnostic build only: ablation bits (1 cells, 2 gather, 4 scatter, 8 prefetch)
  // plane kernels, SHARED form of the index records (Plan::sh_*; nullptr: the expanded form): per plane batch
  // kShBatchWords words {dof base, dof-list record, index-run record, 0}; bdofsp / idxp then hold every DISTINCT
  // record once, the dof lists relative to the batch's dof base
  const uint32_t *shtab = nullptr;
  // mass term (mfgpu_desc.mass_coefficient; nullptr: none -- the launchers then run the MASS = false instantiations):
  // the folded weight m = c * JxW per quadrature point, in plan cell order (pencil families) and in the per-batch
  // [n*n rows][NT tasks] layout of coefp (plane families)
  const T *mass = nullptr;
  const T *massp = nullptr;
};

// mfgpu_vmult_multi, fused groups (apply_batches_g at width NV = 2, 3): the arguments of a single apply -- dst, src
// and halo are those of vector 0 -- plus what a group adds.  A struct of its own: ApplyArgs<T> is passed by value to
// every single-vector kernel (apply_batches_g at width 1 among them) and stays byte for byte what it is.
constexpr int kMaxFusedWidth = 3;
template <typename T>
struct MultiArgs : ApplyArgs<T> {
  size_t stride = 0;         // vector v starts at element v * stride of dst and of src
  T *halos[kMaxFusedWidth];  // halo buffer of vector v (halos[0] == halo)
};
constexpr size_t kMaxLdsBytes = 160 * 1024;  // LDS of a gfx950 CU

// 1D tables, passed by value as kernel arguments (=> scalar registers).
template <typename T, int n>
struct Tables {
  T S[((n + 1) / 2) * n];   // S[i*n+q]  = phi_i(x_q), rows i < (n+1)/2 (rest by symmetry)
  T Dt[((n + 1) / 2) * n];  // Dt[q*n+t] = l_t'(x_q), rows q < (n+1)/2 (rest by antisymmetry)
};

// the kernel-argument tables of the pencil kernels from the host tables S, Dt
template <typename T, int n>
inline Tables<T, n> make_tables(const double *S, const double *Dt) {
  Tables<T, n> tab;
  for (int i = 0; i < ((n + 1) / 2) * n; ++i) {
    tab.S[i] = (T)S[i];
    tab.Dt[i] = (T)Dt[i];
  }
  return tab;
}

// One cell-loop kernel instantiation, bound for a handle (mfgpu_api.hip create_arrays; at most three per handle: the
// plane family, its <HN> instantiation, the batch family).  The six families -- apply: apply_batches, x:
// apply_batches_x, g / g2: apply_batches_g / _g2 (g2 reads a.tabS, a.tabDt instead of S, Dt), p: apply_planes3,
// q: apply_planes4 / apply_planes4w -- each have ONE function F_bind, the only place that names the family's
// instantiations: it maps (dim, n, hn, twopass, sh, mass) to the instantiation that kernel_exists (mfgpu_internal.h)
// admits (else hipErrorInvalidValue) and hands it to bind_cell_kernel, which sets the dynamic-LDS attribute of
// precisely the kernels whose launch entries it stores.  So what can be launched has been configured.
// launch[add](a, S, Dt, lds, grid, st) runs batches [a.batch0, a.batch_end) with the 1D tables made from S, Dt.
// (Args: the kernel's by-value argument struct -- ApplyArgs<T> for every single-vector kernel, MultiArgs<T> for the
// g family at the fused widths of mfgpu_vmult_multi)
template <typename T, typename Args = ApplyArgs<T>>
struct CellKernel {
  size_t lds = 0;  // dynamic LDS bytes per workgroup (set first, also when binding fails)
  int per_cu = 0;  // resident workgroups per CU (of launch[0])
  hipError_t (*launch[2])(const Args &a, const double *S, const double *Dt, size_t lds, uint32_t grid,
                          hipStream_t st) = {nullptr, nullptr};
};

// MakeTab: the kernel's by-value table argument from the host tables (make_tables, make_tables_eo), or nullptr
template <typename T, int Block, auto K, auto MakeTab, typename Args = ApplyArgs<T>>
hipError_t launch_cell_kernel(const Args &a, const double *S, const double *Dt, size_t lds, uint32_t grid,
                              hipStream_t st) {
  if constexpr (std::is_null_pointer_v<decltype(MakeTab)>)
    hipLaunchKernelGGL(K, dim3(grid), dim3(Block), lds, st, a);
  else
    hipLaunchKernelGGL(K, dim3(grid), dim3(Block), lds, st, a, MakeTab(S, Dt));
  return hipGetLastError();
}

// K0 / K1: the add = 0 / add = 1 instantiations (the same kernel where ADD is the run-time field a.add)
template <typename T, int Block, auto K0, auto K1, auto MakeTab, typename Args = ApplyArgs<T>>
hipError_t bind_cell_kernel(size_t lds, CellKernel<T, Args> *k) {
  k->lds = lds;
  for (const void *f : {(const void *)K1, (const void *)K0})
    if (const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  k->launch[0] = launch_cell_kernel<T, Block, K0, MakeTab, Args>;
  k->launch[1] = launch_cell_kernel<T, Block, K1, MakeTab, Args>;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&k->per_cu, (const void *)K0, Block, lds);
}

// run-time n = 2 .. 7 and switches -> f(std::integral_constant<int, n>, std::bool_constant<flag>...)
template <typename F>
hipError_t dispatch_flags(F &&f) { return f(); }
template <typename F, typename... B>
hipError_t dispatch_flags(F &&f, bool flag, B... rest) {
  return dispatch_flags(
      [&](auto... c) { return flag ? f(std::true_type{}, c...) : f(std::false_type{}, c...); }, rest...);
}
template <typename F, typename... B>
hipError_t dispatch_instantiation(int n, F &&f, B... flags) {
  auto at = [&](auto N) { return dispatch_flags([&](auto... c) { return f(N, c...); }, flags...); };
  switch (n) {
    case 2: return at(std::integral_constant<int, 2>{});
    case 3: return at(std::integral_constant<int, 3>{});
    case 4: return at(std::integral_constant<int, 4>{});
    case 5: return at(std::integral_constant<int, 5>{});
    case 6: return at(std::integral_constant<int, 6>{});
    case 7: return at(std::integral_constant<int, 7>{});
    default: return hipErrorInvalidValue;
  }
}
template <typename T>
constexpr int number_type_of = sizeof(T) == 8 ? MFGPU_F64 : MFGPU_F32;

#define MFGPU_CELL_LOOP_FAMILY(F)                                                                              \
  template <typename T>                                                                                        \
  hipError_t F##_bind(int dim, int n, bool hn, bool twopass, bool sh, bool mass, uint32_t nb_max, CellKernel<T> *k);
MFGPU_CELL_LOOP_FAMILY(apply)
MFGPU_CELL_LOOP_FAMILY(x)
MFGPU_CELL_LOOP_FAMILY(g)
MFGPU_CELL_LOOP_FAMILY(g2)
MFGPU_CELL_LOOP_FAMILY(p)
MFGPU_CELL_LOOP_FAMILY(q)
#undef MFGPU_CELL_LOOP_FAMILY
// the g family by width (mfgpu_kernels_g.hip): g_bind is width 1; with a MultiKernel<T> the fused instantiation
// (n, hn, mass) of width nv = 2, 3 that fused_kernel_exists admits, else hipErrorInvalidValue (also where the plan's
// batches need more LDS than a CU has)
template <typename T>
using MultiKernel = CellKernel<T, MultiArgs<T>>;
template <typename T, typename Args>
hipError_t g_bind_width(int n, bool hn, bool sh, bool mass, int nv, uint32_t nb_max, CellKernel<T, Args> *k);

// pass 2, class-sorted structure-of-arrays form (mfgpu_pass2.hip)
void build_pass2_classes(const std::vector<uint32_t> &sdofs, const std::vector<uint32_t> &s_off,
                         const std::vector<uint32_t> &s_idx, std::vector<uint32_t> &arr, std::vector<uint32_t> &tiles);
template <typename T>
hipError_t reduce_classes_launch(T *dst, const T *src, const T *halo, const uint32_t *arr, const uint32_t *tiles,
                                 uint32_t n_tiles, int add, hipStream_t st);
// ... the same kernel at width nv = 2, 3 for a fused group: the class arrays are read once per tile; vector v's sums
// come from halos[v] and go to dst + v * stride (identity rows: src + v * stride), each in the single apply's order
template <typename T>
hipError_t reduce_classes_multi_launch(int nv, T *dst, const T *src, size_t stride, T *const *halos, const uint32_t *arr,
                                       const uint32_t *tiles, uint32_t n_tiles, int add, hipStream_t st);
// pass 2, shared form: one workgroup per owner batch (Plan::sh_p2rec / sh_p2tab); reverse: last batch first
template <typename T>
hipError_t reduce_owner_batches_launch(T *dst, const T *src, const T *halo, const uint32_t *rec, const uint32_t *tab,
                                       uint32_t n_batches, uint32_t hstride, int reverse, int add, hipStream_t st);
// setup relayout of the folded coefficient for the plane kernels (mfgpu_kernels_p.hip)
template <typename T>
hipError_t relayout_coef_launch(T *out, const T *in, const uint32_t *cell_batch, const uint32_t *cell_pos,
                                size_t total, int n, hipStream_t st);
// setup folds of the general-Jacobian kernels: 6 (3D, mfgpu_kernels_g.hip) or 3 (2D, mfgpu_kernels_g2.hip) metric
// entries per point
template <typename T>
hipError_t fold_general_launch(T *M, const T *coef, const T *jxw, const T *jinv, const uint32_t *order,
                               uint32_t n_cells, uint32_t nd, hipStream_t st);
template <typename T>
hipError_t fold_general2_launch(T *M, const T *coef, const T *jxw, const T *jinv, const uint32_t *order,
                                uint32_t n_cells, uint32_t nd, hipStream_t st);
template <typename T>
hipError_t orphan_launch(T *dst, const T *src, const uint32_t *orph, uint32_t n, int add, hipStream_t st);
template <typename T>
hipError_t coefficient_launch(T *coef, const T *qpts, size_t nq, int dim, hipStream_t st);
template <typename T>
hipError_t fold_launch(T *c, const T *coef, const T *jxw, const T *j0, const uint32_t *order,
                       uint32_t n_cells, uint32_t nd, hipStream_t st);
template <typename T>
hipError_t fill_launch(T *v, size_t n, T a, hipStream_t st);
// What a fold of the coefficient or of the mass weight reads besides the coefficient itself, on the device: JxW
// [n_cells * nd], inv_jac (one scalar per cell, or with `general` the full J^-1 per point), and the plan's cell order
// (plan position -> caller cell).  Temporaries of the set-up, or resident in a handle created with
// MFGPU_UPDATABLE_COEFFICIENTS (FoldGeometry).
template <typename T>
struct FoldInputs {
  const T *jxw = nullptr, *jinv = nullptr;
  const uint32_t *order = nullptr;
  int dim = 0;
  uint32_t n_cells = 0, nd = 0;
  bool general = false;
  size_t metric_entries() const { return (size_t)n_cells * nd * (general ? (dim == 3 ? 6 : 3) : 1); }
};
// The folds themselves, asynchronous on st, no allocation: the one code path of the set-up and of
// mfgpu_*_update_coefficients.  coef, c: device arrays [n_cells * nd] in the caller's cell order.
//   metric: per point the scalar a J0^2 JxW, or with `general` the symmetric a JxW J^-1 J^-T (6 entries in 3D, 3 in 2D)
//   mass:   out[pos * nd + q] = c[cell][q] * JxW[cell][q] for the cell at plan position pos
template <typename T>
hipError_t fold_coefficient_launch(T *out, const T *coef, const FoldInputs<T> &in, hipStream_t st);
template <typename T>
hipError_t fold_mass_launch(T *out, const T *c, const FoldInputs<T> &in, hipStream_t st);
// Owner of the device copies behind a FoldInputs (the operator's number type; JxW may stay empty where the owner has
// it resident already)
struct FoldGeometry {
  DeviceArray<void> jxw, jinv;
  DeviceArray<uint32_t> order;
  int dim = 0;
  uint32_t n_cells = 0, nd = 0;
  bool general = false;
  int upload(const void *JxW, const void *inv_jac, const uint32_t *cell_order, int dim_, uint32_t n_cells_, uint32_t nd_,
             bool general_, int number_type);
  size_t bytes() const { return jxw.bytes() + jinv.bytes() + order.bytes(); }
  template <typename T>
  FoldInputs<T> inputs(const T *jxw_resident = nullptr) const {
    FoldInputs<T> in;
    in.jxw = jxw_resident ? jxw_resident : jxw.as<const T>();
    in.jinv = jinv.as<const T>();
    in.order = order.get();
    in.dim = dim, in.n_cells = n_cells, in.nd = nd, in.general = general;
    return in;
  }
};
// Set-up of the mass weight, synchronised on return: the description's mass_coefficient goes to the device as a
// temporary and is folded into `out` (allocated here)
template <typename T>
int fold_mass(DeviceArray<T> &out, const void *mass_coefficient, const FoldInputs<T> &in);
// Set-up of the folded metric, synchronised on return: the description's coefficient (or, if NULL, the coefficient
// evaluated from its quadrature_points) goes to the device as a temporary and is folded into `out` (allocated here)
template <typename T>
int fold_coefficient(DeviceArray<T> &out, const void *coefficient, const void *quadrature_points,
                     const FoldInputs<T> &in);

// ---- SURVEY.md 8(f) N1 / N2 (mfgpu_aux.hip)
template <typename T>
hipError_t diag_launch(int dim, int n, T *diag, uint32_t n_batches, const uint32_t *batch_cell_off,
                       const uint32_t *batch_dof_off, const uint32_t *bdofs, const uint16_t *lmap, const T *coef,
                       const uint32_t *cmask, const T *hn_weights, const T *tab2, hipStream_t st);
template <typename T>
hipError_t diag_general_launch(int n, T *diag, uint32_t n_batches, const uint32_t *batch_cell_off,
                               const uint32_t *batch_dof_off, const uint32_t *bdofs, const uint16_t *lmap,
                               const T *metric, const uint32_t *cmask, const T *hn_weights, const T *tab,
                               hipStream_t st);
template <typename T>
hipError_t diag_general2_launch(int n, T *diag, uint32_t n_batches, const uint32_t *batch_cell_off,
                                const uint32_t *batch_dof_off, const uint32_t *bdofs, const uint16_t *lmap,
                                const T *metric, const uint32_t *cmask, const T *hn_weights, const T *tab,
                                hipStream_t st);
// adds the mass term's local diagonal M_ii = sum_q m_q prod_d S[i_d][q_d]^2 (all geometry variants; tab = the 1D table
// [n*n] index dof*n + q, squared already or not)
template <typename T>
hipError_t diag_mass_launch(int dim, int n, T *diag, uint32_t n_batches, const uint32_t *batch_cell_off,
                            const uint32_t *batch_dof_off, const uint32_t *bdofs, const uint16_t *lmap, const T *mass,
                            const uint32_t *cmask, const T *hn_weights, const T *tab, bool squared, hipStream_t st);
template <typename T>
hipError_t set_values_launch(T *v, const uint32_t *idx, uint32_t n, T value, hipStream_t st);
// op: 0 sadd (v = s v + a w), 1 equ (v = a w), 2 scale (v *= w), 3 divide (v /= w), 4 invert, 5 mul (v *= a)
template <typename T>
hipError_t vec_map_launch(int op, T *v, const T *w, T s, T a, size_t n, hipStream_t st);
// op: 0 dot (v . w), 1 add_and_dot (v += a x; v . w), 2 count of non-zeros; blocking, result on the host
template <typename T>
hipError_t vec_reduce_launch(int op, T *v, const T *x, const T *w, T a, size_t n, hipStream_t st, double *out);

}  // namespace mfgpu
#endif
