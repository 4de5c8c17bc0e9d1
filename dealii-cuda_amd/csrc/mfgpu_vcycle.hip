// The multigrid V-cycle as one object: deal.II's Multigrid::level_v_step + PreconditionMG with
// PreconditionChebyshev smoothers, as host/mfgpu_shim_mg.h composes it (MultigridPreconditioner::level_v_step,
// SURVEY's poisson_mg.cu:365-380), on the level operators, transfers and copy pairs of the C-ABI, which it borrows.
//   mfgpu_vcycle_create   set-up: level vectors, inverse diagonals, eigenvalue estimates, the coarse solver's data
//   mfgpu_vcycle_apply    z = M^-1 r: only enqueues kernels and device-to-device copies on the caller's stream
//   mfgpu_vcycle_refresh  the set-up's values again after a coefficient update, enqueue-only (the pieces
//                         are in mfgpu_refresh.hip); from the first one on the smoother reads its scalars from the device
// New kernel here: dense_solve_kernel, x = A0^-1 b on the coarsest level from the inverse formed at creation, which
// replaces a CG loop with two blocking reductions per iteration.  The other new launches of the schedule are
// mfgpu_transfer_prolongate_add (mfgpu_transfer.hip) and mfgpu_vec_residual (mfgpu_mixed.hip).
// Schedule per level l > 0 (launch counts in DESIGN.md §16), the smoother always in its fused form:
//   x = Chebyshev(defect) from zero;  t = A x;  [edge = down x;]  t = defect - (t [+ edge]);  defect_{l-1} += R t;
//   level l - 1;  x += P x_{l-1};  [edge = up x;  edge = defect - edge;]  x = Chebyshev(defect or edge) from x
// Zero fills the schedule makes redundant are not launched: the pre-smoother and the coarse solve write every entry of
// `solution`, and without copy pairs the finest defect is a full copy of r.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <vector>

#include "mfgpu_device.h"
#include "mfgpu_refresh.h"
#include "mfgpu_stream.h"

using namespace mfgpu;

namespace {

// x = inv b.  inv: n rows of ld doubles, ld = n rounded up to even with a zero in the padding column, so every row
// starts on 16 bytes and is read as double2.  One wave per row, the lanes stride the row by 128 columns; each lane
// accumulates in double in column order, the 64 lane sums are added in the fixed order of wave_sum, lane 0 rounds to
// T.  No atomics, no LDS: two calls give equal bits.  Bound: one read of the inverse (n * ld * 8 bytes) from L2 / HBM;
// b (n numbers) is re-read by every wave and stays in cache.
template <typename T>
__global__ void __launch_bounds__(256)
dense_solve_kernel(T *__restrict__ x, const double *__restrict__ inv, const T *__restrict__ b, uint32_t n, uint32_t ld) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= n) return;  // uniform per wave
  const double *a = inv + (size_t)row * ld;
  double acc = 0.0;
  for (uint32_t c = 2u * lane; c < ld; c += 128u) {
    const double2 v = *reinterpret_cast<const double2 *>(a + c);
    // c is even and below ld = n rounded up to even, so c < n; c + 1 == n is the zero padding column of an odd n
    const double b0 = (double)b[c], b1 = c + 1u < n ? (double)b[c + 1u] : 0.0;
    acc += v.x * b0;
    acc += v.y * b1;
  }
  acc = wave_sum(acc);
  if (lane == 0) x[row] = (T)acc;
}

// the unit vectors e_0 .. e_{n-1}, one after the other: what the level-0 operator is applied to (refresh)
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) identity_kernel(T *__restrict__ e, uint32_t n, size_t nn) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  stream_chunks<lanes16<T>(), VEC>(tid, stride, nn, [&](size_t o, auto width) {
    constexpr int W = width;
    T v[W];
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = (o + k) / n == (o + k) % n ? T(1) : T(0);
    stw<W>(e + o, v);
  });
}

// y[j n + i] = (A0 e_j)[i] = A0[i][j] in the level type -> a[i][j] = a[j][i] = (double) A0[max(i, j)][min(i, j)]: the
// conversion and the lower triangle that create_dense hands to mfgpu_spd_inverse.  Every entry written by one lane.
template <typename T>
__global__ void __launch_bounds__(256) lower_to_double_kernel(double *__restrict__ a, const T *__restrict__ y, uint32_t n) {
  const size_t nn = (size_t)n * n, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nn; e += stride) {
    const uint32_t i = (uint32_t)(e / n), j = (uint32_t)(e % n), lo = i < j ? i : j, hi = i < j ? j : i;
    a[e] = (double)y[(size_t)lo * n + hi];
  }
}

struct VLevel {
  mfgpu_handle *op = nullptr;
  mfgpu_level *edges = nullptr;
  mfgpu_transfer *from_coarser = nullptr;
  const mfgpu_index_pairs *to_mg = nullptr, *from_mg = nullptr;
  uint32_t n = 0;
  double lambda_max = 0.0;
  uint32_t eig_steps = 0;    // the steps the estimate at creation took
  std::vector<double> cheb;  // mfgpu_cg_chebyshev_scalars
  // refresh (inside mfgpu_vcycle::refresh): the state block of the device estimate and the scalar table
  EigState *state = nullptr;
  double *table = nullptr;
  DeviceArray<void> defect, solution, t, r, upd, dinv, edge;
};

}  // namespace

struct mfgpu_vcycle {
  std::vector<VLevel> levels;
  int level_type = MFGPU_F64, active_type = MFGPU_F64;
  uint32_t n_active = 0, degree = 5;
  bool pairs = false;
  uint32_t coarse = MFGPU_VCYCLE_COARSE_DENSE, coarse_max_iterations = 0, ld = 0;
  double coarse_tolerance = 0.0;
  DeviceArray<double> inverse;  // DENSE
  mfgpu_cg *cg = nullptr;       // CG
  size_t device_bytes = 0;
  // refresh: what creation was told, and the one allocation of the first mfgpu_vcycle_refresh with the pieces in it
  bool estimated = false;
  uint32_t eig_iterations = 15;
  double range = 15.0;
  DeviceArray<void> refresh;       // coarse status | state blocks | scalar tables | partial sums | dense coarse pieces
  uint32_t *coarse_status = nullptr;
  double *partials = nullptr, *a_double = nullptr, *spd_workspace = nullptr;
  void *identity = nullptr, *a_level = nullptr;
  std::vector<char> mirror;        // host copy of coarse status + state blocks (mfgpu_vcycle_refresh_status)
  ~mfgpu_vcycle() { mfgpu_cg_destroy(cg); }
};

namespace mfgpu {
void vcycle_active(const mfgpu_vcycle *v, int *active_type, uint32_t *n_active) {
  *active_type = v->active_type;
  *n_active = v->n_active;
}
}  // namespace mfgpu

namespace {

// A0 on the host in double: column j = A0 e_j, one apply per unit vector (set-up)
int level_matrix_to_host(mfgpu_handle *op, uint32_t n, int nt, std::vector<double> &a) {
  DeviceArray<void> e, y;
  const size_t es = esize(nt);
  if (const int rc = e.alloc(n * es, true)) return rc;
  if (const int rc = y.alloc(n * es, true)) return rc;
  const double one_d = 1.0, zero_d = 0.0;
  const float one_f = 1.0f, zero_f = 0.0f;
  const void *one = nt == MFGPU_F64 ? (const void *)&one_d : (const void *)&one_f;
  const void *zero = nt == MFGPU_F64 ? (const void *)&zero_d : (const void *)&zero_f;
  std::vector<double> col_d(nt == MFGPU_F64 ? n : 0);
  std::vector<float> col_f(nt == MFGPU_F32 ? n : 0);
  a.assign((size_t)n * n, 0.0);
  for (uint32_t j = 0; j < n; ++j) {
    char *ej = static_cast<char *>(e.get()) + (size_t)j * es;
    if (j) HIP_TRY(hipMemcpy(ej - es, zero, es, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ej, one, es, hipMemcpyHostToDevice));
    if (const int rc = mfgpu_vmult(op, y.get(), e.get(), nullptr)) return rc;
    if (nt == MFGPU_F64) {
      HIP_TRY(hipMemcpy(col_d.data(), y.get(), n * es, hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < n; ++i) a[(size_t)i * n + j] = col_d[i];
    } else {
      HIP_TRY(hipMemcpy(col_f.data(), y.get(), n * es, hipMemcpyDeviceToHost));
      for (uint32_t i = 0; i < n; ++i) a[(size_t)i * n + j] = (double)col_f[i];
    }
  }
  return 0;
}

int create_dense(mfgpu_vcycle *v) {
  VLevel &L0 = v->levels[0];
  const uint32_t n = L0.n;
  std::vector<double> a, inv((size_t)n * n);
  if (const int rc = level_matrix_to_host(L0.op, n, v->level_type, a)) return rc;
  if (mfgpu_spd_inverse(n, a.data(), inv.data()))  // reads the lower triangle: the symmetrised matrix
    return einval("mfgpu_vcycle_create: the level-0 matrix is not positive definite");
  const uint32_t ld = n + (n & 1u);
  std::vector<double> padded((size_t)n * ld, 0.0);
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j < n; ++j) padded[(size_t)i * ld + j] = inv[(size_t)i * n + j];
  v->ld = ld;
  return v->inverse.upload(padded.data(), padded.size());
}

template <typename T>
int dense_solve(mfgpu_vcycle *v, hipStream_t st) {
  VLevel &L0 = v->levels[0];
  hipLaunchKernelGGL(dense_solve_kernel<T>, dim3((L0.n + 3u) / 4u), dim3(256), 0, st, L0.solution.as<T>(),
                     (const double *)v->inverse.get(), (const T *)L0.defect.as<T>(), L0.n, v->ld);
  return hip_check(hipGetLastError(), "mfgpu_vcycle_apply: dense coarse solve");
}

int coarse_solve(mfgpu_vcycle *v, void *stream) {
  VLevel &L0 = v->levels[0];
  if (v->coarse == MFGPU_VCYCLE_COARSE_DENSE)
    return v->level_type == MFGPU_F64 ? dense_solve<double>(v, (hipStream_t)stream) : dense_solve<float>(v, (hipStream_t)stream);
  // MGCoarseIterative (host/poisson_mg.cc) without its host loop: every iteration is enqueued, the freeze rule of
  // mfgpu_cg ends the solve on the device
  if (const int rc = mfgpu_cg_begin_relative(v->cg, L0.solution.get(), L0.defect.get(), v->coarse_tolerance,
                                             v->coarse_max_iterations, stream))
    return rc;
  return mfgpu_cg_iterate(v->cg, v->coarse_max_iterations, stream);
}

// PreconditionChebyshev::run_fused (host/mfgpu_shim_mg.h): x = p(A) b from zero, or one more sweep on x
int smooth(mfgpu_vcycle *v, VLevel &L, const void *b, bool zero_start, void *stream) {
  const int nt = v->level_type;
  void *x = L.solution.get(), *upd = L.upd.get(), *r = L.r.get(), *t = L.t.get();
  if (!zero_start)
    if (const int rc = mfgpu_vmult(L.op, t, x, stream)) return rc;
  if (L.table) {  // after the first refresh: the same sweep on the device table
    if (const int rc = mfgpu_vec_chebyshev_start_dev(x, upd, r, b, zero_start ? nullptr : t, L.dinv.get(), L.table,
                                                     zero_start ? 1 : 0, L.n, nt, stream))
      return rc;
    for (uint32_t k = 1; k < v->degree; ++k) {
      if (const int rc = mfgpu_vmult(L.op, t, upd, stream)) return rc;
      if (const int rc = mfgpu_vec_chebyshev_update_dev(x, upd, r, t, L.dinv.get(), L.table + (2 * k - 1), L.n, nt, stream))
        return rc;
    }
    return 0;
  }
  if (const int rc = mfgpu_vec_chebyshev_start(x, upd, r, b, zero_start ? nullptr : t, L.dinv.get(), L.cheb[0],
                                               zero_start ? 1 : 0, L.n, nt, stream))
    return rc;
  for (uint32_t k = 1; k < v->degree; ++k) {
    if (const int rc = mfgpu_vmult(L.op, t, upd, stream)) return rc;
    if (const int rc = mfgpu_vec_chebyshev_update(x, upd, r, t, L.dinv.get(), L.cheb[2 * k - 1], L.cheb[2 * k], L.n, nt, stream))
      return rc;
  }
  return 0;
}

int v_step(mfgpu_vcycle *v, uint32_t l, void *stream) {
  if (l == 0) return coarse_solve(v, stream);
  VLevel &L = v->levels[l], &C = v->levels[l - 1];
  const int nt = v->level_type;
  int rc;
  if ((rc = smooth(v, L, L.defect.get(), true, stream))) return rc;          // pre-smoothing from zero
  if ((rc = mfgpu_vmult(L.op, L.t.get(), L.solution.get(), stream))) return rc;  // t = A x
  if (L.edges) {
    if ((rc = mfgpu_level_vmult_interface_down(L.edges, L.edge.get(), L.solution.get(), stream))) return rc;
    if ((rc = mfgpu_vec_residual(L.t.get(), L.defect.get(), L.edge.get(), L.n, nt, stream))) return rc;
  } else {
    if ((rc = mfgpu_vec_residual(L.t.get(), L.defect.get(), nullptr, L.n, nt, stream))) return rc;
  }
  if ((rc = mfgpu_transfer_restrict_and_add(L.from_coarser, C.defect.get(), L.t.get(), stream))) return rc;
  if ((rc = v_step(v, l - 1, stream))) return rc;
  if ((rc = mfgpu_transfer_prolongate_add(L.from_coarser, L.solution.get(), C.solution.get(), stream))) return rc;
  if (L.edges) {  // post-smoothing on defect - up x
    if ((rc = mfgpu_level_vmult_interface_up(L.edges, L.edge.get(), L.solution.get(), stream))) return rc;
    if ((rc = mfgpu_vec_residual(L.edge.get(), L.defect.get(), nullptr, L.n, nt, stream))) return rc;
    return smooth(v, L, L.edge.get(), false, stream);
  }
  return smooth(v, L, L.defect.get(), false, stream);
}

// everything that needs no device; fills v->levels with the borrowed pieces
int validate(const mfgpu_vcycle_desc *d, mfgpu_vcycle *v) {
  if (d->n_levels == 0) return einval("mfgpu_vcycle_create: n_levels == 0");
  if (!d->levels) return einval("mfgpu_vcycle_create: null levels");
  if (!valid_number_type(d->active_type)) return einval("mfgpu_vcycle_create: active_type must be MFGPU_F64 or MFGPU_F32");
  if (d->coarse > MFGPU_VCYCLE_COARSE_CG) return einval("mfgpu_vcycle_create: unknown coarse mode");
  if (d->smoothing_range != 0.0 && !(d->smoothing_range > 1.0 && std::isfinite(d->smoothing_range)))
    return einval("mfgpu_vcycle_create: the smoothing range must be > 1");
  if (!(d->coarse_tolerance >= 0.0) || !std::isfinite(d->coarse_tolerance))
    return einval("mfgpu_vcycle_create: the coarse tolerance must be a finite number >= 0");
  const uint32_t nl = d->n_levels;
  for (uint32_t l = 0; l < nl; ++l) {
    const mfgpu_vcycle_level_desc &ld = d->levels[l];
    if (!ld.op) return einval("mfgpu_vcycle_create: a level without an operator");
    if (l > 0 && !ld.from_coarser) return einval("mfgpu_vcycle_create: a level above 0 without a transfer");
    if ((ld.to_mg == nullptr) != (ld.from_mg == nullptr) ||
        (ld.to_mg == nullptr) != (d->levels[0].to_mg == nullptr))
      return einval("mfgpu_vcycle_create: copy pairs on every level (to_mg and from_mg) or on none");
  }
  v->levels.resize(nl);
  v->level_type = handle_number_type(d->levels[0].op);
  v->active_type = d->active_type;
  v->n_active = d->n_active;
  v->pairs = d->levels[0].to_mg != nullptr;
  v->degree = d->smoother_degree ? d->smoother_degree : 5;
  const double range = d->smoothing_range != 0.0 ? d->smoothing_range : 15.0;
  v->range = range;
  v->estimated = d->lambda_max == nullptr;
  v->eig_iterations = d->eig_iterations ? d->eig_iterations : 15u;
  for (uint32_t l = 0; l < nl; ++l) {
    const mfgpu_vcycle_level_desc &ld = d->levels[l];
    VLevel &L = v->levels[l];
    L.op = ld.op;
    L.edges = ld.edges;
    L.from_coarser = l ? ld.from_coarser : nullptr;
    L.to_mg = ld.to_mg;
    L.from_mg = ld.from_mg;
    L.n = mfgpu_n_dofs(ld.op);
    if (handle_number_type(ld.op) != v->level_type) return einval("mfgpu_vcycle_create: the levels are of different number types");
    if (ld.edges && mfgpu_level_operator(ld.edges) != ld.op)
      return einval("mfgpu_vcycle_create: op is not the operator of the level's edges");
    if (l > 0) {
      uint32_t nc = 0, nf = 0;
      int nt = 0;
      transfer_sizes(ld.from_coarser, &nc, &nf, &nt);
      if (nc != v->levels[l - 1].n || nf != L.n || nt != v->level_type)
        return einval("mfgpu_vcycle_create: a transfer does not fit its two levels (sizes or number type)");
      if (d->lambda_max) {
        if (!(d->lambda_max[l] > 0.0) || !std::isfinite(d->lambda_max[l]))
          return einval("mfgpu_vcycle_create: lambda_max must be > 0 on every level above 0");
        L.lambda_max = d->lambda_max[l];
        L.cheb.resize(2 * v->degree - 1);
        if (const int rc = mfgpu_cg_chebyshev_scalars(v->degree, L.lambda_max, range, L.cheb.data())) return rc;
      }
    } else if (d->lambda_max) {
      L.lambda_max = d->lambda_max[0];
    }
  }
  if (!v->pairs && d->n_active != v->levels[nl - 1].n)
    return einval("mfgpu_vcycle_create: without copy pairs the active vector is the finest level's (n_active != n_dofs(top))");
  const uint32_t n0 = v->levels[0].n;
  v->coarse = d->coarse != MFGPU_VCYCLE_COARSE_AUTO ? d->coarse
              : n0 <= MFGPU_VCYCLE_DENSE_MAX        ? MFGPU_VCYCLE_COARSE_DENSE
                                                    : MFGPU_VCYCLE_COARSE_CG;
  if (v->coarse == MFGPU_VCYCLE_COARSE_DENSE && n0 > MFGPU_VCYCLE_DENSE_MAX)
    return einval("mfgpu_vcycle_create: MFGPU_VCYCLE_COARSE_DENSE above MFGPU_VCYCLE_DENSE_MAX level-0 dofs");
  const double eps = v->level_type == MFGPU_F64 ? std::numeric_limits<double>::epsilon()
                                                : (double)std::numeric_limits<float>::epsilon();
  v->coarse_tolerance = d->coarse_tolerance != 0.0 ? d->coarse_tolerance : std::max(1e-10, 100.0 * eps);
  v->coarse_max_iterations = d->coarse_max_iterations ? d->coarse_max_iterations : n0;
  return 0;
}

size_t round16(size_t b) { return (b + 15u) & ~(size_t)15u; }

// the one allocation of the first refresh (sizes: include/mfgpu.h) and what has to be in it before the first kernel
int refresh_allocate(mfgpu_vcycle *v, hipStream_t st) {
  const uint32_t nl = (uint32_t)v->levels.size(), n0 = v->levels[0].n;
  const size_t es = esize(v->level_type), nn = (size_t)n0 * n0;
  const size_t table = round16(sizeof(double) * (2 * v->degree - 1));
  const bool dense = v->coarse == MFGPU_VCYCLE_COARSE_DENSE;
  size_t bytes = 16 + (nl - 1) * (kEigStateBytes + table);
  if (v->estimated) bytes += 2 * kStreamBlocks * sizeof(double);
  if (dense) bytes += 2 * round16(nn * es) + round16(nn * sizeof(double)) + round16(2 * nn * sizeof(double));
  DeviceArray<void> block;
  if (const int rc = block.alloc(bytes, true)) return rc;
  char *p = block.as<char>();
  uint32_t *coarse_status = reinterpret_cast<uint32_t *>(p);
  p += 16;
  std::vector<EigState> states(nl - 1);
  for (uint32_t l = 1; l < nl; ++l) {
    states[l - 1] = EigState();
    states[l - 1].result.lambda_max = v->levels[l].lambda_max;  // an estimate that fails keeps it
  }
  if (nl > 1) HIP_TRY(hipMemcpy(p, states.data(), (nl - 1) * kEigStateBytes, hipMemcpyHostToDevice));
  EigState *state0 = reinterpret_cast<EigState *>(p);
  p += (nl - 1) * kEigStateBytes;
  char *table0 = p;
  for (uint32_t l = 1; l < nl; ++l, p += table)  // the scalars in use: those of a given lambda_max stay for good
    HIP_TRY(hipMemcpy(p, v->levels[l].cheb.data(), v->levels[l].cheb.size() * sizeof(double), hipMemcpyHostToDevice));
  if (v->estimated) {
    v->partials = reinterpret_cast<double *>(p);
    p += 2 * kStreamBlocks * sizeof(double);
  }
  if (dense) {
    v->identity = p;
    v->a_level = p + round16(nn * es);
    v->a_double = reinterpret_cast<double *>(p + 2 * round16(nn * es));
    v->spd_workspace = reinterpret_cast<double *>(p + 2 * round16(nn * es) + round16(nn * sizeof(double)));
    const unsigned grid = stream_grid(nn, 16 / es, true);
    if (v->level_type == MFGPU_F64)
      hipLaunchKernelGGL((identity_kernel<double, true>), dim3(grid), dim3(256), 0, st, (double *)v->identity, n0, nn);
    else
      hipLaunchKernelGGL((identity_kernel<float, true>), dim3(grid), dim3(256), 0, st, (float *)v->identity, n0, nn);
    if (const int rc = hip_check(hipGetLastError(), "mfgpu_vcycle_refresh: unit vectors")) return rc;
  }
  for (uint32_t l = 1; l < nl; ++l) {  // from here on smooth() runs the _dev forms
    v->levels[l].state = state0 + (l - 1);
    v->levels[l].table = reinterpret_cast<double *>(table0 + (l - 1) * table);
  }
  v->coarse_status = coarse_status;
  v->mirror.assign(16 + (nl - 1) * kEigStateBytes, 0);
  v->refresh = std::move(block);
  v->device_bytes += bytes;
  return 0;
}

}  // namespace

extern "C" {

int mfgpu_spd_inverse(uint32_t n, const double *a, double *inv) {
  if (!a || !inv || a == inv) return einval("mfgpu_spd_inverse: null or aliasing argument");
  // a = L L^T (L in the lower triangle of inv), then L <- L^-1 in place, then inv = L^-T L^-1
  double *L = inv;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j < n; ++j) L[(size_t)i * n + j] = j <= i ? a[(size_t)i * n + j] : 0.0;
  for (uint32_t j = 0; j < n; ++j) {
    double *Lj = L + (size_t)j * n;
    double d = Lj[j];
    for (uint32_t k = 0; k < j; ++k) d -= Lj[k] * Lj[k];
    if (!(d > 0.0) || !std::isfinite(d)) return einval("mfgpu_spd_inverse: the matrix is not positive definite");
    const double ljj = std::sqrt(d);
    Lj[j] = ljj;
    for (uint32_t i = j + 1; i < n; ++i) {
      double *Li = L + (size_t)i * n;
      double s = Li[j];
      for (uint32_t k = 0; k < j; ++k) s -= Li[k] * Lj[k];
      Li[j] = s / ljj;
    }
  }
  // M = L^-1, row by row from the top: M[i][j] = -(sum_{k=j}^{i-1} L[i][k] M[k][j]) / L[i][i]; row i of L is used up by
  // row i of M only, rows k < i already hold M
  std::vector<double> row(n);
  for (uint32_t i = 0; i < n; ++i) {
    double *Li = L + (size_t)i * n;
    const double inv_d = 1.0 / Li[i];
    for (uint32_t j = 0; j < i; ++j) row[j] = 0.0;
    for (uint32_t k = 0; k < i; ++k) {
      const double lik = Li[k];
      const double *Mk = L + (size_t)k * n;
      for (uint32_t j = 0; j <= k; ++j) row[j] += lik * Mk[j];
    }
    for (uint32_t j = 0; j < i; ++j) Li[j] = -row[j] * inv_d;
    Li[i] = inv_d;
  }
  // inv = M^T M: inv[i][j] = sum_{k >= max(i, j)} M[k][i] M[k][j]; accumulate row k of M into a separate upper part is
  // not possible in place, so go through a copy of M
  std::vector<double> M(L, L + (size_t)n * n);
  for (size_t e = 0; e < (size_t)n * n; ++e) inv[e] = 0.0;
  for (uint32_t k = 0; k < n; ++k) {
    const double *Mk = M.data() + (size_t)k * n;
    for (uint32_t i = 0; i <= k; ++i) {
      const double mki = Mk[i];
      double *Ii = inv + (size_t)i * n;
      for (uint32_t j = 0; j <= i; ++j) Ii[j] += mki * Mk[j];
    }
  }
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = i + 1; j < n; ++j) inv[(size_t)i * n + j] = inv[(size_t)j * n + i];
  return MFGPU_OK;
}

int mfgpu_estimate_lambda_max(mfgpu_handle *op, const void *inv_diag_dev, uint32_t min_iterations, double *lambda_max) {
  uint32_t steps = 0;
  return mfgpu_estimate_lambda_max_steps(op, inv_diag_dev, min_iterations, lambda_max, &steps);
}

int mfgpu_estimate_lambda_max_steps(mfgpu_handle *op, const void *inv_diag_dev, uint32_t min_iterations, double *lambda_max,
                                    uint32_t *steps) {
  if (!op || !inv_diag_dev || !lambda_max || !steps) return einval("mfgpu_estimate_lambda_max: null argument");
  const uint32_t n = mfgpu_n_dofs(op);
  const int nt = handle_number_type(op);
  if (n == 0) return einval("mfgpu_estimate_lambda_max: an operator without dofs");
  // PreconditionChebyshev::initialize (host/mfgpu_shim_mg.h), unchanged
  DeviceArray<void> v, w;
  if (const int rc = v.alloc(n * esize(nt))) return rc;
  if (const int rc = w.alloc(n * esize(nt), true)) return rc;
  if (nt == MFGPU_F64) {
    std::vector<double> init(n);
    for (uint32_t i = 0; i < n; ++i) init[i] = std::sin(0.7 * i) + 0.3;
    HIP_TRY(hipMemcpy(v.get(), init.data(), n * sizeof(double), hipMemcpyHostToDevice));
  } else {
    std::vector<float> init(n);
    for (uint32_t i = 0; i < n; ++i) init[i] = (float)(std::sin(0.7 * i) + 0.3);
    HIP_TRY(hipMemcpy(v.get(), init.data(), n * sizeof(float), hipMemcpyHostToDevice));
  }
  const uint32_t min_steps = min_iterations > 5u ? min_iterations : 5u;
  double lam = 1.0, prev = 0.0;
  for (uint32_t k = 0; k < 200; ++k) {
    int rc;
    double nw = 0.0, nv = 0.0;
    if ((rc = mfgpu_vmult(op, w.get(), v.get(), nullptr))) return rc;
    if ((rc = mfgpu_vec_scale(w.get(), inv_diag_dev, n, nt, nullptr))) return rc;
    if ((rc = mfgpu_vec_l2_norm(w.get(), n, nt, nullptr, &nw))) return rc;
    if ((rc = mfgpu_vec_l2_norm(v.get(), n, nt, nullptr, &nv))) return rc;
    if (!(nw > 0.0) || !(nv > 0.0) || !std::isfinite(nw)) return einval("mfgpu_estimate_lambda_max: the power iteration broke down");
    lam = nw / nv;
    const double scale = nt == MFGPU_F64 ? 1.0 / nw : (double)(float)(1.0 / nw);
    if ((rc = mfgpu_vec_equ(v.get(), scale, w.get(), n, nt, nullptr))) return rc;
    *steps = k + 1;
    if (k + 1 >= min_steps && std::fabs(lam - prev) <= 0.01 * lam) break;
    prev = lam;
  }
  HIP_TRY(hipStreamSynchronize(nullptr));  // the work vectors are freed on return
  *lambda_max = 1.2 * lam;
  return MFGPU_OK;
}

int mfgpu_vcycle_create(const mfgpu_vcycle_desc *d, mfgpu_vcycle **out) {
  if (!d || !out) return einval("mfgpu_vcycle_create: null argument");
  std::unique_ptr<mfgpu_vcycle> v(new (std::nothrow) mfgpu_vcycle);
  if (!v) return MFGPU_ENOMEM;
  if (const int rc = validate(d, v.get())) return rc;
  const size_t es = esize(v->level_type);
  const uint32_t nl = (uint32_t)v->levels.size();
  const double range = d->smoothing_range != 0.0 ? d->smoothing_range : 15.0;
  size_t bytes = 0;
  for (uint32_t l = 0; l < nl; ++l) {
    VLevel &L = v->levels[l];
    const size_t vb = (size_t)L.n * es;
    int rc = 0;
    // level 0 has no smoother: neither coarse solver reads an inverse diagonal, so it keeps none.  Its lambda_max is
    // still estimated when none is given (mfgpu_vcycle_lambda_max reports every level), through a diagonal that is freed
    // before create returns
    DeviceArray<void> *vectors[7] = {&L.defect, &L.solution, &L.dinv, &L.t, &L.r, &L.upd, &L.edge};
    const int n_vectors = l == 0 ? 2 : L.edges ? 7 : 6;
    for (int k = 0; k < n_vectors && !rc; ++k) rc = vectors[k]->alloc(vb, true);
    if (rc) return rc;
    bytes += n_vectors * vb;
    if (l == 0 && d->lambda_max) continue;
    DeviceArray<void> dinv0;  // level 0 only
    if (l == 0 && (rc = dinv0.alloc(vb, true))) return rc;
    void *dinv = l == 0 ? dinv0.get() : L.dinv.get();
    if ((rc = mfgpu_compute_inverse_diagonal(L.op, dinv, nullptr))) return rc;
    if (!d->lambda_max) {
      if ((rc = mfgpu_estimate_lambda_max_steps(L.op, dinv, v->eig_iterations, &L.lambda_max, &L.eig_steps))) return rc;
      if (l > 0) {
        L.cheb.resize(2 * v->degree - 1);
        if ((rc = mfgpu_cg_chebyshev_scalars(v->degree, L.lambda_max, range, L.cheb.data()))) return rc;
      }
    }
  }
  if (v->coarse == MFGPU_VCYCLE_COARSE_DENSE) {
    if (const int rc = create_dense(v.get())) return rc;
    bytes += v->inverse.bytes();
  } else {
    if (const int rc = mfgpu_cg_create(v->levels[0].op, MFGPU_CG_NONE, nullptr, 0, 0, 0, &v->cg)) return rc;
    bytes += mfgpu_cg_memory_consumption(v->cg);
  }
  HIP_TRY(hipDeviceSynchronize());  // set-up is complete before the first apply on any stream
  v->device_bytes = bytes;
  *out = v.release();
  return MFGPU_OK;
}

int mfgpu_vcycle_apply(mfgpu_vcycle *v, void *z_dev, const void *r_dev, void *stream) {
  if (!v || !z_dev || !r_dev || z_dev == r_dev) return einval("mfgpu_vcycle_apply: null or aliasing argument");
  const int lt = v->level_type, at = v->active_type;
  const uint32_t top = (uint32_t)v->levels.size() - 1;
  int rc;
  // copy_to_mg: the restriction adds into the coarser defects, so they start from zero
  for (uint32_t l = 0; l <= top; ++l) {
    VLevel &L = v->levels[l];
    if (v->pairs) {
      if ((rc = mfgpu_vec_fill(L.defect.get(), L.n, lt, 0.0, stream))) return rc;
      if ((rc = mfgpu_vec_copy_pairs_convert(L.to_mg, L.defect.get(), lt, r_dev, at, stream))) return rc;
    } else if (l < top) {
      if ((rc = mfgpu_vec_fill(L.defect.get(), L.n, lt, 0.0, stream))) return rc;
    } else {
      if ((rc = mfgpu_vec_convert(L.defect.get(), lt, r_dev, at, L.n, stream))) return rc;
    }
  }
  if ((rc = v_step(v, top, stream))) return rc;
  // copy_from_mg
  if (!v->pairs) return mfgpu_vec_convert(z_dev, at, v->levels[top].solution.get(), lt, v->levels[top].n, stream);
  if ((rc = mfgpu_vec_fill(z_dev, v->n_active, at, 0.0, stream))) return rc;
  for (uint32_t l = 0; l <= top; ++l)
    if ((rc = mfgpu_vec_copy_pairs_convert(v->levels[l].from_mg, z_dev, at, v->levels[l].solution.get(), lt, stream))) return rc;
  return MFGPU_OK;
}

int mfgpu_vcycle_refresh(mfgpu_vcycle *v, uint32_t eig_steps, void *stream) {
  if (!v) return einval("mfgpu_vcycle_refresh: null argument");
  VLevel &L0 = v->levels[0];
  const bool dense = v->coarse == MFGPU_VCYCLE_COARSE_DENSE;
  if (dense && L0.n > MFGPU_SPD_INVERSE_DEVICE_MAX) {
    set_error("mfgpu_vcycle_refresh: MFGPU_VCYCLE_COARSE_DENSE above MFGPU_SPD_INVERSE_DEVICE_MAX level-0 dofs: re-create "
              "the object or use MFGPU_VCYCLE_COARSE_CG");
    return MFGPU_EUNSUPPORTED;
  }
  const hipStream_t st = (hipStream_t)stream;
  int rc;
  if (!v->refresh.get() && (rc = refresh_allocate(v, st))) return rc;
  const uint32_t nl = (uint32_t)v->levels.size();
  for (uint32_t l = 1; l < nl; ++l)
    if ((rc = mfgpu_compute_inverse_diagonal(v->levels[l].op, v->levels[l].dinv.get(), stream))) return rc;
  if (v->estimated)
    for (uint32_t l = 1; l < nl; ++l) {
      VLevel &L = v->levels[l];  // t and r are scratch between applies
      if ((rc = eig_enqueue(L.op, L.dinv.get(), v->eig_iterations, eig_steps ? eig_steps : L.eig_steps, L.state, v->partials,
                            L.t.get(), L.r.get(), stream)))
        return rc;
      if ((rc = mfgpu_cg_chebyshev_scalars_dev(v->degree, &L.state->result.lambda_max, v->range, L.table, stream))) return rc;
    }
  if (!dense) return MFGPU_OK;
  const uint32_t n0 = L0.n;
  if ((rc = mfgpu_vmult_multi(L0.op, v->a_level, v->identity, n0, n0, MFGPU_MULTI_LOOP, stream))) return rc;
  const unsigned grid = stream_grid((size_t)n0 * n0, 1, false);
  if (v->level_type == MFGPU_F64)
    hipLaunchKernelGGL(lower_to_double_kernel<double>, dim3(grid), dim3(256), 0, st, v->a_double, (const double *)v->a_level, n0);
  else
    hipLaunchKernelGGL(lower_to_double_kernel<float>, dim3(grid), dim3(256), 0, st, v->a_double, (const float *)v->a_level, n0);
  if ((rc = hip_check(hipGetLastError(), "mfgpu_vcycle_refresh: level-0 matrix"))) return rc;
  return mfgpu_spd_inverse_enqueue(n0, v->a_double, n0, v->inverse.get(), v->ld, v->spd_workspace, v->coarse_status, stream);
}

int mfgpu_vcycle_refresh_status(mfgpu_vcycle *v, void *stream, mfgpu_vcycle_refresh_info *info) {
  if (!v || !info) return einval("mfgpu_vcycle_refresh_status: null argument");
  if (!v->refresh.get()) return einval("mfgpu_vcycle_refresh_status: call mfgpu_vcycle_refresh first");
  HIP_TRY(hipMemcpyAsync(v->mirror.data(), v->refresh.get(), v->mirror.size(), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  *info = mfgpu_vcycle_refresh_info();
  std::memcpy(&info->coarse_status, v->mirror.data(), sizeof(uint32_t));
  if (!v->estimated) return MFGPU_OK;
  for (size_t l = 1; l < v->levels.size(); ++l) {
    EigState s;
    std::memcpy(&s, v->mirror.data() + 16 + (l - 1) * kEigStateBytes, sizeof s);
    info->eig_status_max = std::max(info->eig_status_max, s.result.status);
    info->eig_steps_max = std::max(info->eig_steps_max, s.result.steps);
    if (s.result.status == 1u || s.result.status == 2u) v->levels[l].lambda_max = s.result.lambda_max;
  }
  return MFGPU_OK;
}

int mfgpu_vcycle_lambda_max(const mfgpu_vcycle *v, double *lambda) {
  if (!v || !lambda) return einval("mfgpu_vcycle_lambda_max: null argument");
  for (size_t l = 0; l < v->levels.size(); ++l) lambda[l] = v->levels[l].lambda_max;
  return MFGPU_OK;
}

size_t mfgpu_vcycle_memory_consumption(const mfgpu_vcycle *v) { return v ? v->device_bytes : 0; }

void mfgpu_vcycle_destroy(mfgpu_vcycle *v) { delete v; }

}  // extern "C"
