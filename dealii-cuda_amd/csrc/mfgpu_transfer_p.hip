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
// scalar branch.  The fine side needs nothing: a constrained fine position is a bit-31 entry made on the host
// (p_owner_list).  HN = false is the code as it was.
#include <hip/hip_runtime.h>

#include <cmath>
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
constexpr int kWaves = 4;            // cells per workgroup pass
constexpr unsigned kMaxGrid = 2048;  // workgroups: 8 per CU on 256 CUs; more cells than 4 * kMaxGrid take further passes

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
  constexpr uint32_t kSkip = 0x80000000u;
  const uint64_t stride = (uint64_t)gridDim.x * kWaves;
  uint64_t cell = (uint64_t)blockIdx.x * kWaves + wave;
  uint32_t gc[KF], gf[KF];
#pragma unroll
  for (int j = 0; j < KF; ++j) {
    const int t = lane + 64 * j;
    gc[j] = (cell < n_cells && t < NC) ? coarse[cell * NC + t] : kSkip;
    gf[j] = (cell < n_cells && t < NF) ? fine[cell * NF + t] : kSkip;
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
      next_gc[j] = (next < n_cells && t < NC) ? coarse[next * NC + t] : kSkip;
      next_gf[j] = (next < n_cells && t < NF) ? fine[next * NF + t] : kSkip;
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
      gc[j] = next_gc[j];
      gf[j] = next_gf[j];
    }
    mask = next_mask;
  }
}

template <typename T, bool RESTRICT, bool ADD, bool HN>
hipError_t launch_p(const mfgpu_transfer *t, T *dst, const T *src, hipStream_t st) {
  const uint32_t n = t->n_coarse_cells;
  if (n == 0) return hipSuccess;
  const unsigned groups = (n + kWaves - 1) / kWaves;
  const unsigned grid = groups < kMaxGrid ? groups : kMaxGrid;
#define TRP_CASE(D, PF)                                                                                          \
  case D * 10 + PF:                                                                                              \
    hipLaunchKernelGGL((p_transfer_kernel<D, PF, T, RESTRICT, ADD, HN>), dim3(grid), dim3(64 * kWaves), 0, st, dst, src, \
                       t->d_coarse.get(), t->d_fine.get(), t->d_p1.as<const T>(), n, t->degree_coarse,           \
                       HN ? t->d_mask.get() : nullptr, HN ? t->d_weights.as<const T>() : nullptr);               \
    break;
  switch (t->dim * 10 + t->degree) {
    TRP_CASE(2, 2) TRP_CASE(2, 3) TRP_CASE(2, 4) TRP_CASE(2, 5) TRP_CASE(2, 6)
    TRP_CASE(3, 2) TRP_CASE(3, 3) TRP_CASE(3, 4) TRP_CASE(3, 5) TRP_CASE(3, 6)
    default: return hipErrorInvalidValue;
  }
#undef TRP_CASE
  return hipGetLastError();
}

template <typename T, bool HN>
hipError_t launch_mode(const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, hipStream_t st) {
  switch (mode) {
    case TRANSFER_PROLONGATE: return launch_p<T, false, false, HN>(t, (T *)dst, (const T *)src, st);
    case TRANSFER_PROLONGATE_ADD: return launch_p<T, false, true, HN>(t, (T *)dst, (const T *)src, st);
    case TRANSFER_RESTRICT_ADD: return launch_p<T, true, false, HN>(t, (T *)dst, (const T *)src, st);
  }
  return hipErrorInvalidValue;
}

bool valid_degree_pair(int pc, int pf) { return pc >= 1 && pf <= 6 && pc < pf; }

// P1[X * (pc+1) + x] = phi_x(xi_X): the FE_Q(pc) Lagrange basis on its Gauss-Lobatto nodes at the FE_Q(pf) nodes
void p_prolongation_1d(int pc, int pf, std::vector<double> &P1) {
  std::vector<double> cn, fn, val, der;
  gll_01(pc, cn);
  gll_01(pf, fn);
  const int nc = pc + 1, nf = pf + 1;
  P1.assign((size_t)nf * nc, 0.0);
  for (int X = 0; X < nf; ++X) {
    int same = -1;  // a fine node that is a coarse node (the end points; 1/2 when both degrees are even): exact 0 / 1
    for (int x = 0; x < nc; ++x)
      if (std::fabs(fn[X] - cn[x]) < 1e-14) same = x;
    if (same >= 0) {
      P1[(size_t)X * nc + same] = 1.0;
      continue;
    }
    lagrange_eval(cn, fn[X], val, der);
    for (int x = 0; x < nc; ++x) P1[(size_t)X * nc + x] = val[x];
  }
}

}  // namespace

// the 9 bits of a constraint mask (hanging_nodes.cuh:38-50); in 2D only TYPE x, y and FACE x, y
bool valid_mask(int dim, uint32_t m) { return !(m & ~(dim == 3 ? 0x1ffu : 0x1bu)); }

// can resolve_hanging_nodes with mask m write local position t of a cell of n^dim entries?
bool constrained_position(int dim, int n, uint32_t m, int t) {
  bool type;
  int q;
  for (int dir = 0; dir < dim; ++dir)
    if (hn_flag_at(dim, n, m, dir, t, type, q)) return true;
  return false;
}

// The fine index list as it is uploaded: bit 31 on every entry but the owner's.  The owner of a fine dof is the first
// cell, in cell order, that lists it at a position that is not constrained (without a mask: the first that lists it).
// `covered` = the number of fine dofs with an owner.  A dof that is listed but has no owner is an error: the kernels would
// drop it without a word.
int p_owner_list(const char *who, int dim, int degree_fine, uint32_t n_cells, const uint32_t *fine_cell_dofs,
                 const uint32_t *mask, uint32_t n_fine_dofs, uint32_t *out, size_t &covered) {
  const int nf = degree_fine + 1;
  const size_t NF = (size_t)ipow(nf, dim);
  std::vector<uint8_t> seen(n_fine_dofs, 0);  // 1: listed, 2: owned
  std::vector<uint8_t> con;                   // the constrained positions of the current cell's mask
  uint32_t con_mask = 0;
  covered = 0;
  size_t listed = 0;
  for (uint32_t c = 0; c < n_cells; ++c) {
    const uint32_t m = mask ? mask[c] : 0u;
    if (!valid_mask(dim, m)) {
      set_error(std::string(who) + ": a constraint mask has bits outside the defined ones (9 in 3D; TYPE x, y and FACE x, y "
                "in 2D)");
      return MFGPU_EINVAL;
    }
    if (m && (con.empty() || m != con_mask)) {
      con.resize(NF);
      for (size_t i = 0; i < NF; ++i) con[i] = constrained_position(dim, nf, m, (int)i);
      con_mask = m;
    }
    for (size_t i = 0; i < NF; ++i) {
      const uint32_t g = fine_cell_dofs[c * NF + i];
      if (g >= n_fine_dofs) {
        set_error(std::string(who) + ": fine dof out of range");
        return MFGPU_EINVAL;
      }
      const bool owns = seen[g] < 2 && !(m && con[i]);
      out[c * NF + i] = g | (owns ? 0u : 0x80000000u);
      if (!seen[g]) ++listed;
      if (owns) ++covered;
      seen[g] = owns ? 2 : (seen[g] ? seen[g] : 1);
    }
  }
  if (covered != listed) {
    set_error(std::string(who) + ": a fine dof is listed only at constrained positions, so no cell owns it (the masks and "
              "fine_cell_dofs do not belong together)");
    return MFGPU_EINVAL;
  }
  return 0;
}

hipError_t launch_p_transfer(const mfgpu_transfer *t, void *dst, const void *src, TransferMode mode, hipStream_t st) {
  if (t->hanging_nodes)
    return t->number_type == MFGPU_F64 ? launch_mode<double, true>(t, dst, src, mode, st)
                                       : launch_mode<float, true>(t, dst, src, mode, st);
  return t->number_type == MFGPU_F64 ? launch_mode<double, false>(t, dst, src, mode, st)
                                     : launch_mode<float, false>(t, dst, src, mode, st);
}

}  // namespace mfgpu

extern "C" {

int mfgpu_transfer_p_prolongation_1d(int degree_coarse, int degree_fine, double *p1) {
  using namespace mfgpu;
  if (!p1 || !valid_degree_pair(degree_coarse, degree_fine)) {
    set_error("mfgpu_transfer_p_prolongation_1d: needs 1 <= degree_coarse < degree_fine <= 6 and an output array");
    return MFGPU_EINVAL;
  }
  std::vector<double> P1;
  p_prolongation_1d(degree_coarse, degree_fine, P1);
  std::memcpy(p1, P1.data(), P1.size() * sizeof(double));
  return 0;
}

int mfgpu_transfer_p_owner_list(int dim, int degree_fine, uint32_t n_cells, const uint32_t *fine_cell_dofs,
                                const uint32_t *constraint_mask, uint32_t n_fine_dofs, uint32_t *out) {
  using namespace mfgpu;
  if ((dim != 2 && dim != 3) || degree_fine < 1 || degree_fine > 6 || (n_cells && (!fine_cell_dofs || !out)) ||
      n_fine_dofs >= (1u << 31)) {
    set_error("mfgpu_transfer_p_owner_list: bad argument (1 <= degree_fine <= 6, dim 2 or 3, dof count < 2^31, arrays)");
    return MFGPU_EINVAL;
  }
  size_t covered;
  return p_owner_list("mfgpu_transfer_p_owner_list", dim, degree_fine, n_cells, fine_cell_dofs, constraint_mask, n_fine_dofs,
                      out, covered);
}

int mfgpu_transfer_create_p(int dim, int degree_coarse, int degree_fine, int number_type, uint32_t n_cells,
                            const uint32_t *coarse_cell_dofs, const uint32_t *fine_cell_dofs, uint32_t n_coarse_dofs,
                            uint32_t n_fine_dofs, const uint32_t *coarse_dirichlet, uint32_t n_coarse_dirichlet,
                            const double *prolongation_1d, mfgpu_transfer **out) {
  return mfgpu_transfer_create_p_hn(dim, degree_coarse, degree_fine, number_type, n_cells, coarse_cell_dofs, fine_cell_dofs,
                                    n_coarse_dofs, n_fine_dofs, coarse_dirichlet, n_coarse_dirichlet, prolongation_1d, nullptr,
                                    nullptr, out);
}

int mfgpu_transfer_create_p_hn(int dim, int degree_coarse, int degree_fine, int number_type, uint32_t n_cells,
                               const uint32_t *coarse_cell_dofs, const uint32_t *fine_cell_dofs, uint32_t n_coarse_dofs,
                               uint32_t n_fine_dofs, const uint32_t *coarse_dirichlet, uint32_t n_coarse_dirichlet,
                               const double *prolongation_1d, const uint32_t *constraint_mask,
                               const double *coarse_constraint_weights, mfgpu_transfer **out) {
  using namespace mfgpu;
  if (!out || (dim != 2 && dim != 3) || !valid_degree_pair(degree_coarse, degree_fine) ||
      (n_cells && (!coarse_cell_dofs || !fine_cell_dofs)) || (n_coarse_dirichlet && !coarse_dirichlet) ||
      !valid_number_type(number_type) || n_coarse_dofs >= (1u << 31) || n_fine_dofs >= (1u << 31)) {
    set_error("mfgpu_transfer_create_p: bad argument (1 <= degree_coarse < degree_fine <= 6, dim 2 or 3, dof counts < 2^31)");
    return MFGPU_EINVAL;
  }
  const int nc = degree_coarse + 1, nf = degree_fine + 1;
  const size_t NC = (size_t)ipow(nc, dim), NF = (size_t)ipow(nf, dim);
  std::vector<uint8_t> dir(n_coarse_dofs, 0);
  for (uint32_t i = 0; i < n_coarse_dirichlet; ++i) {
    if (coarse_dirichlet[i] >= n_coarse_dofs) {
      set_error("mfgpu_transfer_create_p: Dirichlet dof out of range");
      return MFGPU_EINVAL;
    }
    dir[coarse_dirichlet[i]] = 1;
  }
  std::vector<uint32_t> cd((size_t)n_cells * NC), fd((size_t)n_cells * NF);
  for (size_t i = 0; i < cd.size(); ++i) {
    const uint32_t g = coarse_cell_dofs[i];
    if (g >= n_coarse_dofs) {
      set_error("mfgpu_transfer_create_p: coarse dof out of range");
      return MFGPU_EINVAL;
    }
    cd[i] = g | (dir[g] ? 0x80000000u : 0u);
  }
  size_t covered = 0;
  int rc;
  if ((rc = p_owner_list("mfgpu_transfer_create_p", dim, degree_fine, n_cells, fine_cell_dofs, constraint_mask, n_fine_dofs,
                         fd.data(), covered)))
    return rc;
  std::vector<double> P1;
  if (prolongation_1d)
    P1.assign(prolongation_1d, prolongation_1d + (size_t)nf * nc);
  else
    p_prolongation_1d(degree_coarse, degree_fine, P1);
  std::unique_ptr<mfgpu_transfer> t(new mfgpu_transfer());
  t->kind = TRANSFER_KIND_P;
  t->dim = dim;
  t->degree = degree_fine;
  t->degree_coarse = degree_coarse;
  t->number_type = number_type;
  t->n_coarse_cells = n_cells;
  t->n_coarse_dofs = n_coarse_dofs;
  t->n_fine_dofs = n_fine_dofs;
  t->covers_all = covered == n_fine_dofs;
  std::vector<float> P1f(P1.begin(), P1.end());
  const void *p1src = number_type == MFGPU_F64 ? (const void *)P1.data() : (const void *)P1f.data();
  if ((rc = t->d_coarse.upload(cd.data(), cd.size())) || (rc = t->d_fine.upload(fd.data(), fd.size())) ||
      (rc = t->d_p1.upload(p1src, P1.size() * esize(number_type))))
    return rc;
  t->device_bytes = t->d_coarse.bytes() + t->d_fine.bytes() + t->d_p1.bytes();
  if (constraint_mask) {  // (NULL: the conforming object, the HN = false kernels)
    std::vector<double> W;
    if (coarse_constraint_weights)
      W.assign(coarse_constraint_weights, coarse_constraint_weights + (size_t)nc * nc);
    else
      fe_q_constraint_weights(degree_coarse, W);
    std::vector<float> Wf(W.begin(), W.end());
    const void *wsrc = number_type == MFGPU_F64 ? (const void *)W.data() : (const void *)Wf.data();
    if ((rc = t->d_mask.upload(constraint_mask, n_cells)) || (rc = t->d_weights.upload(wsrc, W.size() * esize(number_type))))
      return rc;
    t->hanging_nodes = true;
    t->device_bytes += t->d_mask.bytes() + t->d_weights.bytes();
  }
  *out = t.release();
  return 0;
}

int mfgpu_transfer_create_p_from_meshes(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, mfgpu_transfer **out) {
  using namespace mfgpu;
  if (!coarse || !fine || !out) {
    set_error("mfgpu_transfer_create_p_from_meshes: null argument");
    return MFGPU_EINVAL;
  }
  const Mesh &C = coarse->mesh, &F = fine->mesh;
  if (C.cells_kind < 0 || F.cells_kind < 0 || !C.constraint_mask.empty() || !F.constraint_mask.empty()) {
    set_error("mfgpu_transfer_create_p_from_meshes: meshes with hanging nodes (adaptive, from leaves) are not supported");
    return MFGPU_EUNSUPPORTED;
  }
  bool same = C.dim == F.dim && C.cells_kind == F.cells_kind && C.n_cells == F.n_cells;
  if (same && C.cells_kind == 0)
    for (int d = 0; d < 3; ++d) same = same && C.nper[d] == F.nper[d];
  same = same && C.slab[0] == F.slab[0] && C.slab[1] == F.slab[1] && C.n_ref == F.n_ref;
  if (!same) {
    set_error("mfgpu_transfer_create_p_from_meshes: the two meshes are not the same cells (dimension, kind, cells per "
              "direction and slab or n_ref, cell count)");
    return MFGPU_EINVAL;
  }
  return mfgpu_transfer_create_p(C.dim, C.degree, F.degree, F.number_type, C.n_cells, C.loc2glob.data(), F.loc2glob.data(),
                                 C.n_dofs, F.n_dofs, C.constrained.data(), (uint32_t)C.constrained.size(), nullptr, out);
}

int mfgpu_transfer_create_p_hn_from_meshes(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, mfgpu_transfer **out) {
  using namespace mfgpu;
  if (!coarse || !fine || !out) {
    set_error("mfgpu_transfer_create_p_hn_from_meshes: null argument");
    return MFGPU_EINVAL;
  }
  const Mesh &C = coarse->mesh, &F = fine->mesh;
  if (C.cells_kind >= 0 && F.cells_kind >= 0 && C.constraint_mask.empty() && F.constraint_mask.empty())
    return mfgpu_transfer_create_p_from_meshes(coarse, fine, out);
  // adaptive meshes and meshes from leaves: the same leaves in the same order; the masks are geometric, so equal too
  if (C.cells_kind != -1 || F.cells_kind != -1 || C.dim != F.dim || C.n_cells != F.n_cells || C.cell_levels.empty() ||
      C.cell_levels != F.cell_levels || C.constraint_mask != F.constraint_mask) {
    set_error("mfgpu_transfer_create_p_hn_from_meshes: the two meshes are not the same cells (dimension, cell count, the "
              "leaves and their order, constraint masks)");
    return MFGPU_EINVAL;
  }
  return mfgpu_transfer_create_p_hn(C.dim, C.degree, F.degree, F.number_type, C.n_cells, C.loc2glob.data(), F.loc2glob.data(),
                                    C.n_dofs, F.n_dofs, C.constrained.data(), (uint32_t)C.constrained.size(), nullptr,
                                    C.constraint_mask.empty() ? nullptr : C.constraint_mask.data(), C.weights.data(), out);
}

}  // extern "C"
