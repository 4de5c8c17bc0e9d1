// C-ABI entry points (include/mfgpu.h): handle life cycle, vmult / vmult_add, GpuVector pieces.
#include <hip/hip_runtime.h>

#include <type_traits>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mfgpu_kernels.h"

using namespace mfgpu;

// start / stop pairs of timing events around a stretch of a stream's work (profiling)
struct EventTimer {
  std::vector<Event> ev;
  size_t used = 0;
  double ms = 0.0;
  int begin(hipStream_t st) {
    if (used + 2 > ev.size()) {
      Event e0, e1;
      int rc;
      if ((rc = e0.create(hipEventDefault)) || (rc = e1.create(hipEventDefault))) return rc;
      ev.push_back(std::move(e0));
      ev.push_back(std::move(e1));
    }
    HIP_TRY(hipEventRecord(ev[used].get(), st));
    return 0;
  }
  int end(hipStream_t st) {
    HIP_TRY(hipEventRecord(ev[used + 1].get(), st));
    used += 2;
    return 0;
  }
  // adds the pairs recorded since the last call (the caller has synchronised) and returns the total
  int drain(double *total) {
    for (size_t i = 0; i + 1 < used; i += 2) {
      float t = 0.f;
      HIP_TRY(hipEventElapsedTime(&t, ev[i].get(), ev[i + 1].get()));
      ms += t;
    }
    used = 0;
    *total = ms;
    return 0;
  }
  void reset() {
    used = 0;
    ms = 0.0;
  }
};

struct mfgpu_handle {
  Plan plan;
  int dim = 0, n = 0, nd = 0, number_type = MFGPU_F64;
  bool hn = false;
  std::vector<double> S, Dt;
  std::vector<double> sv, sg;  // the caller's 1D tables (diagonal)
  // device arrays
  DeviceArray<uint32_t> d_batch_cell_off, d_batch_dof_off, d_bdofs;
  DeviceArray<uint8_t> d_bflags;
  DeviceArray<uint16_t> d_lmap;
  DeviceArray<uint16_t> d_lmapx;
  DeviceArray<uint16_t> d_perm;  // apply_batches_x: bank-conflict-free lane -> pencil maps of the y- and z-stage
  // apply_planes3: fixed-size per-batch records (see ApplyArgs)
  DeviceArray<uint32_t> d_bdofsp, d_idxp;
  // ... or their shared form (Plan::sh_*): d_bdofsp / d_idxp then hold the distinct records, d_shtab the per-batch table
  DeviceArray<uint32_t> d_shtab;
  bool shared_records = false;
  size_t record_bytes = 0;  // bytes of d_bdofsp + d_idxp + d_shtab
  DeviceArray<uint32_t> d_hnrec;  // apply_planes3<HN>: per-batch records of the hanging-node line operations
  DeviceArray<uint32_t> d_hn_slot;  // ... and per plane batch the index of its record (0xffffffff: none)
  DeviceArray<void> d_coefp;
  DeviceArray<void> d_coef;
  // mass term (mfgpu_desc.mass_coefficient; empty without): c * JxW in plan cell order, and for the plane batches
  // again in d_coefp's layout
  DeviceArray<void> d_mass, d_massp;
  // MFGPU_UPDATABLE_COEFFICIENTS: what a re-fold reads stays on the device (empty without the flag) -- JxW, inv_jac and
  // the cell order, and for plane plans the cell -> (batch, position in the batch) tables of the relayout
  bool updatable = false;
  FoldGeometry geo;
  DeviceArray<uint32_t> d_cell_batch, d_cell_pos;
  size_t n_plane_cells = 0;  // the plane batches' cells (they come first in plan order)
  DeviceArray<uint32_t> d_cmask, d_orphans;
  DeviceArray<void> d_hnw;
  DeviceArray<uint32_t> d_constrained;  // constrained dof list (set_constrained_values)
  uint32_t n_constrained = 0;
  DeviceArray<void> d_tabsd;  // apply_batches_g2: [S | Dt] full 1D tables in the operator's number type
  DeviceArray<void> d_tab2;  // [2][n*n] squared 1D tables of the diagonal kernel, built on first use
  // two-pass mode
  bool twopass = true;
  DeviceArray<uint32_t> d_batch_nint, d_halo_off;
  // The cell loop runs in SEGMENTS of consecutive batches, one launch each (seg_end[s] = one past the segment's last
  // batch).  Pass 2, class-sorted form (mfgpu_pass2.hip), in 1 + n_segments groups: [0] the priority dofs (mfgpu_dist:
  // the slab's interface planes, reduced first after the whole cell loop so that their exchange overlaps the rest),
  // [1 + s] the other dofs whose LAST toucher batch lies in segment s.  Group 1 + s needs segments 0..s only, so for
  // s < last it runs on the handle's side stream while the next segment's cells are computed (a latency-bound kernel
  // next to an issue-bound one); the last group and the priority group run on the caller's stream.
  std::vector<uint32_t> seg_end;
  std::vector<DeviceArray<uint32_t>> d_p2arr, d_p2tiles;
  std::vector<uint32_t> n_p2tiles;
  // ... or, for the last group of a one-segment plan without priority dofs, the shared form (Plan::sh_p2rec / sh_p2tab):
  // one workgroup per owner batch (reduce_owner_batches); the group's class arrays then hold only the dofs without a
  // partial sum and the orphans
  DeviceArray<uint32_t> d_p2rec, d_p2tab;
  bool p2_shared = false, p2_reverse = false, no_shared_records = false;
  Stream side;
  std::vector<Event> ev_seg;  // [s]: segment s done (recorded on the caller's stream)
  Event ev_side;              // the side stream's pass-2 launches of this vmult done
  bool side_pending = false;  // the caller's stream has not joined the side stream yet
  DeviceArray<void> d_halo;
  DeviceArray<unsigned long long> d_stamps;  // diagnostic build only
  size_t lds = 0, device_bytes = 0;
  // the cell-loop kernel families (choose_kernel_and_plan): `planes` takes the first plan.n_plane_batches batches,
  // `batches` the rest
  PlaneKernel planes = PlaneKernel::none;
  BatchKernel batches = BatchKernel::none;
  // ... and their kernels, bound once by create_arrays (those of the handle's number type; a family the handle does
  // not use stays unbound): the plane family's plain instantiation, its <HN> one (the plane batches of cells with a
  // hanging-node mask), the batch family
  enum { kPlain, kMasked, kBatch };
  CellKernel<double> kernels_f64[3];
  CellKernel<float> kernels_f32[3];
  template <typename T>
  CellKernel<T> &kernel(int which) {
    if constexpr (std::is_same<T, double>::value) return kernels_f64[which];
    else return kernels_f32[which];
  }
  // mfgpu_vmult_multi: the fused instantiations this handle has (index = width - 2; unbound: launch[0] == nullptr),
  // bound by create_arrays next to the batch family, and the halo buffers 2 .. multi_width of a fused group (one
  // allocation of halo_bytes each, made by the first fused call)
  MultiKernel<double> multi_f64[kMaxFusedWidth - 1];
  MultiKernel<float> multi_f32[kMaxFusedWidth - 1];
  template <typename T>
  MultiKernel<T> &multi(int width) {
    if constexpr (std::is_same<T, double>::value) return multi_f64[width - 2];
    else return multi_f32[width - 2];
  }
  int multi_width = 1;
  DeviceArray<void> d_halo_multi;
  size_t halo_bytes = 0;
  uint32_t n_cus = 0, max_workgroups = 0;  // persistent grids: the chip's CUs, mfgpu_desc.max_workgroups (0: no cap)
  // profiling
  bool prof = false;
  EventTimer t_cells;  // around the cell loop
  EventTimer t_pass2;  // around pass 2 (mfgpu_vmult / mfgpu_vmult_add only)
  uint64_t prof_vmults = 0;
};

namespace {

// The only mapping from a kernel family to its F_bind (mfgpu_kernels.h): binds the instantiation (hn, sh) of the plane
// family pk or, with PlaneKernel::none, of the batch family bk
template <typename T>
hipError_t bind_kernel(const mfgpu_handle *h, PlaneKernel pk, BatchKernel bk, bool hn, bool sh, CellKernel<T> *k) {
  const Plan &P = h->plan;
  const auto bind = pk == PlaneKernel::planes3 ? p_bind<T> : pk == PlaneKernel::planes4 ? q_bind<T>
                    : bk == BatchKernel::batches ? apply_bind<T> : bk == BatchKernel::x ? x_bind<T>
                    : bk == BatchKernel::g ? g_bind<T> : bk == BatchKernel::g2 ? g2_bind<T> : nullptr;
  if (!bind) return hipErrorInvalidValue;
  return bind(P.dim, P.n, hn, h->twopass, sh, h->d_mass.get() != nullptr, P.max_batch_dofs, k);
}

// batches [a.batch0, a.batch_end) less the hole, nbat of them, in a bound kernel: a persistent grid of as many
// workgroups as fit on the chip (each loops over its batches)
template <typename T, typename Args>
int launch_bound(mfgpu_handle *h, const CellKernel<T, Args> &k, const Args &a, uint32_t nbat, hipStream_t st) {
  if (!k.launch[0]) {
    set_error("cell-loop kernel not bound");
    return MFGPU_EINVAL;
  }
  uint32_t grid = (uint32_t)(k.per_cu < 1 ? 1 : k.per_cu) * h->n_cus;
  if (h->max_workgroups && h->max_workgroups < grid) grid = h->max_workgroups;
  HIP_TRY(k.launch[a.add != 0](a, h->S.data(), h->Dt.data(), k.lds, nbat < grid ? nbat : grid, st));
  return 0;
}

// symmetry of the 1D tables (see mfgpu_kernels.hip tab_at); also makes mirrored entries bit-equal
int check_symmetrize(int n, std::vector<double> &S, std::vector<double> &Dt) {
  const int p = n - 1;
  double err = 0, mag = 0;
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) {
      const double s1 = S[r * n + c], s2 = S[(p - r) * n + (p - c)];
      const double d1 = Dt[r * n + c], d2 = -Dt[(p - r) * n + (p - c)];
      err = std::fmax(err, std::fmax(std::fabs(s1 - s2), std::fabs(d1 - d2)));
      mag = std::fmax(mag, std::fmax(std::fabs(s1), std::fabs(d1)));
    }
  if (err > 1e-10 * mag) {
    set_error("shape tables are not symmetric about the cell midpoint (unsupported)");
    return MFGPU_EUNSUPPORTED;
  }
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) {
      const int r2 = p - r, c2 = p - c;
      if (r * n + c < r2 * n + c2) {
        const double s = 0.5 * (S[r * n + c] + S[r2 * n + c2]);
        S[r * n + c] = S[r2 * n + c2] = s;
        const double d = 0.5 * (Dt[r * n + c] - Dt[r2 * n + c2]);
        Dt[r * n + c] = d;
        Dt[r2 * n + c2] = -d;
      } else if (r == r2 && c == c2) {
        Dt[r * n + c] = 0.0;
      }
    }
  return 0;
}

// pass-2 arrays from the plan (pass2_groups): group 0 = the dofs listed in `priority` (may be empty), the others by the
// cell-loop segment of their last toucher
int upload_pass2(mfgpu_handle *h, const uint32_t *priority, uint32_t n_priority) {
  const Plan &P = h->plan;
  const size_t ng = 1 + h->seg_end.size();
  // the shared form serves the one group that matters: everything, on a one-segment plan without priority dofs
  const bool shared = P.sh_p2_use && !h->no_shared_records && n_priority == 0 && ng == 2;
  std::vector<Pass2Group> groups;
  int rc;
  if ((rc = pass2_groups(P, h->seg_end, priority, n_priority, shared, groups))) return rc;
  // built aside and moved into the handle when every group is on the device: a failure leaves the handle's arrays
  // as they were.  (These arrays are not counted in device_bytes.)
  std::vector<DeviceArray<uint32_t>> d_arr(ng), d_tiles(ng);
  std::vector<uint32_t> n_tiles(ng, 0u);
  const bool reverse = (size_t)P.halo_off.back() * esize(h->number_type) <= ((size_t)256 << 20);  // (see below)
  DeviceArray<uint32_t> d_rec, d_tab;
  if (shared) {
    if ((rc = d_rec.upload(P.sh_p2rec.data(), P.sh_p2rec.size()))) return rc;
    if ((rc = d_tab.upload(P.sh_p2tab.data(), P.sh_p2tab.size()))) return rc;
  }
  for (size_t g = 0; g < ng; ++g) {
    std::vector<uint32_t> arr, tiles;
    build_pass2_classes(groups[g].dofs, groups[g].offsets, groups[g].slots, arr, tiles);
    n_tiles[g] = (uint32_t)(tiles.size() / 4);
    // Tile order = the order the workgroups of pass 2 are dispatched in.  The builder's order is ascending in the
    // position of a dof's first toucher; while the halo buffer fits the 256 MB Infinity Cache the REVERSE is faster --
    // the partial sums the cell loop wrote last are read first, from cache: pass 2 42.4 -> 41.3 us on C2, 38.9 -> 35.3
    // on C5, -1 .. -3 % per vmult up to 38 M dofs; beyond (n = 96: 57 M dofs, 340 MB of partial sums) it is slower, at
    // 81 M dofs by 10 % (profiles/r03_notes.md section 13)
    if (reverse) {
      const size_t nt = tiles.size() / 4;
      for (size_t a = 0, b = nt ? nt - 1 : 0; a < b; ++a, --b)
        for (int w = 0; w < 4; ++w) std::swap(tiles[4 * a + w], tiles[4 * b + w]);
    }
    if ((rc = d_arr[g].upload(arr.data(), arr.size()))) return rc;
    if ((rc = d_tiles[g].upload(tiles.data(), tiles.size()))) return rc;
  }
  h->d_p2arr = std::move(d_arr);
  h->d_p2tiles = std::move(d_tiles);
  h->n_p2tiles = std::move(n_tiles);
  h->d_p2rec = std::move(d_rec);
  h->d_p2tab = std::move(d_tab);
  h->p2_shared = shared;
  h->p2_reverse = reverse;
  return 0;
}

// d_coef -> d_coefp and / or d_mass -> d_massp for the plane batches (set-up and mfgpu_update_coefficients)
template <typename T>
int relayout_planes(mfgpu_handle *h, const uint32_t *cell_batch, const uint32_t *cell_pos, bool coef, bool mass,
                    hipStream_t st) {
  const size_t total = h->n_plane_cells * (size_t)h->nd;
  if (coef)
    HIP_TRY(relayout_coef_launch<T>(h->d_coefp.as<T>(), h->d_coef.as<const T>(), cell_batch, cell_pos, total, h->n, st));
  if (mass)
    HIP_TRY(relayout_coef_launch<T>(h->d_massp.as<T>(), h->d_mass.as<const T>(), cell_batch, cell_pos, total, h->n, st));
  return 0;
}

// mfgpu_update_coefficients: the set-up's folds again, from device arrays, into the handle's existing arrays
template <typename T>
int update_typed(mfgpu_handle *h, const void *coef, const void *mass, hipStream_t st) {
  const FoldInputs<T> in = h->geo.inputs<T>();
  if (coef) HIP_TRY(fold_coefficient_launch<T>(h->d_coef.as<T>(), (const T *)coef, in, st));
  if (mass) HIP_TRY(fold_mass_launch<T>(h->d_mass.as<T>(), (const T *)mass, in, st));
  if (h->planes == PlaneKernel::none) return 0;
  return relayout_planes<T>(h, h->d_cell_batch.get(), h->d_cell_pos.get(), coef != nullptr, mass != nullptr, st);
}

template <typename T>
int create_arrays(mfgpu_handle *h, const mfgpu_desc &d) {
  const Plan &P = h->plan;
  const size_t ncell = P.n_cells, nd = (size_t)P.nd;
  size_t &acct = h->device_bytes;
  // n elements (DeviceArray<void>: bytes) to the device, counted in mfgpu_memory_consumption
  auto up = [&](auto &arr, const void *src, size_t n) {
    const int rc = arr.upload(src, n);
    acct += arr.bytes();
    return rc;
  };
  int rc;
  if ((rc = up(h->d_batch_cell_off, P.batch_cell_off.data(), P.batch_cell_off.size()))) return rc;
  if ((rc = up(h->d_batch_dof_off, P.batch_dof_off.data(), P.batch_dof_off.size()))) return rc;
  if ((rc = up(h->d_bdofs, P.bdofs.data(), P.bdofs.size()))) return rc;
  if ((rc = up(h->d_bflags, P.bflags.data(), P.bflags.size()))) return rc;
  if ((rc = up(h->d_lmap, P.lmap.data(), P.lmap.size()))) return rc;
  const bool general = h->batches == BatchKernel::g || h->batches == BatchKernel::g2;
  if (h->batches == BatchKernel::x && !h->hn) {
    const std::vector<uint16_t> perm = x_lane_permutation(P.n);  // (bank-conflict-free lanes of the y- and z-stage)
    if ((rc = up(h->d_perm, perm.data(), perm.size()))) return rc;
  }
  if (h->batches == BatchKernel::x || general) {
    const std::vector<uint16_t> lx = x_pencil_runs(P.lmap, P.n);
    if ((rc = up(h->d_lmapx, lx.data(), lx.size()))) return rc;
  }
  if (h->batches == BatchKernel::g2) {  // apply_batches_g2: the full 1D tables [S | Dt]
    std::vector<T> sd(2 * (size_t)P.n * P.n);
    for (int i = 0; i < P.n * P.n; ++i) {
      sd[i] = (T)h->S[i];
      sd[P.n * P.n + i] = (T)h->Dt[i];
    }
    if ((rc = up(h->d_tabsd, sd.data(), sd.size() * sizeof(T)))) return rc;
  }
  if (h->planes != PlaneKernel::none) {
    if ((rc = build_plane_records(h->plan, d.constraint_mask))) return rc;
    if (!P.pr_hn.empty()) {
      if ((rc = up(h->d_hnrec, P.pr_hn.data(), P.pr_hn.size()))) return rc;
      if ((rc = up(h->d_hn_slot, P.pr_hn_slot.data(), P.pr_hn_slot.size()))) return rc;
    }
    // The shared form where the plan chose it (by bytes) and the kernel family has the instantiation (kernel_exists).
    // The expanded arrays are then not uploaded at all.
    h->shared_records = P.sh_use && !(d.flags & MFGPU_NO_SHARED_RECORDS) &&
                        kernel_exists(h->planes, P.n, d.number_type, false, true, d.mass_coefficient != nullptr);
    const std::vector<uint32_t> &rd = h->shared_records ? P.sh_dofs : P.pr_dofs;
    const std::vector<uint32_t> &rx = h->shared_records ? P.sh_idx : P.pr_idx;
    if ((rc = up(h->d_bdofsp, rd.data(), rd.size()))) return rc;
    if ((rc = up(h->d_idxp, rx.data(), rx.size()))) return rc;
    if (h->shared_records && (rc = up(h->d_shtab, P.sh_batch.data(), P.sh_batch.size()))) return rc;
    h->record_bytes = h->d_bdofsp.bytes() + h->d_idxp.bytes() + h->d_shtab.bytes();
  }
  if ((rc = up(h->d_orphans, P.orphans.data(), P.orphans.size()))) return rc;
  if (h->twopass) {
    if ((rc = up(h->d_batch_nint, P.batch_nint.data(), P.batch_nint.size()))) return rc;
    if ((rc = up(h->d_halo_off, P.halo_off.data(), P.halo_off.size()))) return rc;
    if (h->planes != PlaneKernel::none && (uint64_t)P.halo_off.back() >= (1ull << 29)) {
      set_error("halo buffer too large for 32-bit byte offsets");
      return MFGPU_EUNSUPPORTED;
    }
    const size_t hb = ((size_t)P.halo_off.back() + 1) * sizeof(T);  // + the always-zero slot of the untouched dofs
    if ((rc = h->d_halo.alloc(hb, true))) return rc;
    acct += hb;
    h->halo_bytes = hb;
  }
  if (h->hn) {
    std::vector<uint32_t> cm(ncell);
    for (size_t i = 0; i < ncell; ++i) cm[i] = d.constraint_mask[P.cell_order[i]];
    if ((rc = up(h->d_cmask, cm.data(), ncell))) return rc;
    std::vector<T> w((size_t)h->n * h->n);
    for (size_t i = 0; i < w.size(); ++i) w[i] = (T)d.constraint_weights[i];
    if ((rc = up(h->d_hnw, w.data(), w.size() * sizeof(T)))) return rc;
  }
  // coefficient (given, or evaluated on the device from the quadrature points), then folded; the folds' other inputs
  // are temporaries unless the handle is updatable
  FoldGeometry geo;
  if ((rc = geo.upload(d.JxW, d.inv_jac, P.cell_order.data(), P.dim, (uint32_t)ncell, (uint32_t)nd, general,
                       d.number_type)))
    return rc;
  DeviceArray<T> metric;
  if ((rc = fold_coefficient<T>(metric, d.coefficient, d.quadrature_points, geo.inputs<T>()))) return rc;
  h->d_coef = std::move(metric);
  acct += h->d_coef.bytes();
  if (d.mass_coefficient) {
    DeviceArray<T> mass;
    if ((rc = fold_mass<T>(mass, d.mass_coefficient, geo.inputs<T>()))) return rc;
    h->d_mass = std::move(mass);
    acct += h->d_mass.bytes();
  }
  if (h->updatable) {
    acct += geo.bytes();
    h->geo = std::move(geo);
  }
  if (h->planes != PlaneKernel::none) {
    // the folded coefficient again, per batch [row y + n z][task]: the layout of stage B of apply_planes3
    // (d_coef in plan cell order stays: the diagonal kernel reads it)
    const int n = P.n, NT = p_cells_per_wave(n) * n;
    const size_t nbat = P.n_plane_batches, total = nbat * (size_t)(n * n) * NT;
    const size_t ncell_p = P.batch_cell_off[nbat];  // the plane batches' cells come first in plan order
    std::vector<uint32_t> cb(ncell_p), cp(ncell_p);
    for (size_t b = 0; b < nbat; ++b)
      for (uint32_t c = P.batch_cell_off[b]; c < P.batch_cell_off[b + 1]; ++c) {
        cb[c] = (uint32_t)b;
        cp[c] = c - P.batch_cell_off[b];
      }
    DeviceArray<uint32_t> t_cb, t_cp;
    if ((rc = t_cb.upload(cb.data(), ncell_p))) return rc;
    if ((rc = t_cp.upload(cp.data(), ncell_p))) return rc;
    if ((rc = h->d_coefp.alloc(total * sizeof(T), true))) return rc;
    acct += h->d_coefp.bytes();
    h->n_plane_cells = ncell_p;
    if (d.mass_coefficient) {  // the mass weight in the same layout (d_mass stays: diagonal, pencil batches)
      if ((rc = h->d_massp.alloc(total * sizeof(T), true))) return rc;
      acct += h->d_massp.bytes();
    }
    if ((rc = relayout_planes<T>(h, t_cb.get(), t_cp.get(), true, d.mass_coefficient != nullptr, nullptr))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (h->updatable) {
      acct += t_cb.bytes() + t_cp.bytes();
      h->d_cell_batch = std::move(t_cb);
      h->d_cell_pos = std::move(t_cp);
    }
  }
  // the kernels this handle launches, bound once
  int dev = 0;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  h->n_cus = (uint32_t)prop.multiProcessorCount;
  h->max_workgroups = d.max_workgroups;
  if (h->planes != PlaneKernel::none) {
    CellKernel<T> &plain = h->kernel<T>(mfgpu_handle::kPlain), &masked = h->kernel<T>(mfgpu_handle::kMasked);
    HIP_TRY(bind_kernel<T>(h, h->planes, BatchKernel::none, false, h->shared_records, &plain));
    h->lds = plain.lds;
    if (P.n_plain_plane_batches < P.n_plane_batches) {  // batches of masked cells: the <HN> instantiation
      HIP_TRY(bind_kernel<T>(h, h->planes, BatchKernel::none, true, false, &masked));
      h->lds = std::max(h->lds, masked.lds);
    }
  }
  if (h->batches == BatchKernel::none) return 0;
  CellKernel<T> &batch = h->kernel<T>(mfgpu_handle::kBatch);
  const hipError_t bind_batch_family = bind_kernel<T>(h, PlaneKernel::none, h->batches, h->hn, false, &batch);
  h->lds = batch.lds;
  if (h->lds > 160 * 1024) {  // (takes precedence over an error of the bind call)
    set_error("batch needs more than 160 KiB of LDS; lower max_dofs_per_batch");
    return MFGPU_EINVAL;
  }
  HIP_TRY(bind_batch_family);
  // the fused instantiations of the family (fused_kernel_exists), each bound like the kernel above; a width whose
  // batch arrays do not fit the LDS with this plan's batches stays unbound
  if (h->twopass && h->planes == PlaneKernel::none)
    for (const int w : kFusedWidths) {
      if (!fused_kernel_exists(h->batches, P.n, d.number_type, h->hn, h->d_mass.get() != nullptr, w)) continue;
      MultiKernel<T> &mk = h->multi<T>(w);
      if (g_bind_width<T>(P.n, h->hn, false, h->d_mass.get() != nullptr, w, P.max_batch_dofs, &mk) != hipSuccess) {
        (void)hipGetLastError();
        mk = MultiKernel<T>();
      } else
        h->multi_width = std::max(h->multi_width, w);
    }
  return 0;
}

// Segments of the cell loop (see mfgpu_handle::seg_end).  request = mfgpu_desc.cell_loop_segments: 0 the library's
// choice, 1 one segment (pass 2 strictly after the cell loop), k > 1 k segments of equal batch counts.  The choice:
// where two kernel families share the mesh (plane batches | pencil batches of the cells with a hanging-node mask) the
// family boundary -- the launch boundary exists anyway (C3 in round 2: 0.381 instead of 0.392 ms per vmult); two halves
// on hanging-node meshes at p = 4 (below); ONE segment otherwise.  Measured on C2 (profiles/r02_notes.md section 6): with the last 4 of 13 grid iterations as a second
// segment the two kernels do run side by side, but the cell loop slows down by what pass 2 takes (58.6 instead of
// 37 us for the segment; both are short of issue slots and memory latency, not of different resources), and the event
// record / cross-stream waits add three pipeline drains of 5-12 us per vmult: 0.171 instead of 0.156 ms.
void choose_segments(mfgpu_handle *h, uint32_t request) {
  const Plan &P = h->plan;
  const uint32_t nb = (uint32_t)(P.batch_cell_off.size() - 1);
  h->seg_end.assign(1, nb);
  if (!h->twopass || nb < 2 || request == 1) return;
  const uint32_t npl = P.n_plane_batches, nplain = P.n_plain_plane_batches;
  std::vector<uint32_t> cuts;
  if (npl > 0 && npl < nb) cuts.push_back(npl);
  if (nplain > 0 && nplain < npl) cuts.push_back(nplain);  // plain plane batches | plane batches of masked cells
  if (request > 1) {
    for (uint32_t i = 1; i < request; ++i) cuts.push_back((uint32_t)((uint64_t)nb * i / request));
  }
  // hanging-node meshes at p = 4 (batches of masked and unmasked cells interleaved, one instantiation): pass 2 also
  // writes the identity rows of the eliminated hanging-node dofs and is a third of the cell loop's time; its first
  // half beside the second half of the cell loop measures 0.267-0.269 instead of 0.274-0.278 ms on C3 (three segments:
  // 0.280; at p = 3: no difference) -- profiles/r03_notes.md section 8
  if (request == 0 && !P.pr_hn.empty() && nplain == 0 && P.n == 5) cuts.push_back(nb / 2);
  std::sort(cuts.begin(), cuts.end());
  h->seg_end.clear();
  for (uint32_t c : cuts)
    if (c > 0 && c < nb && (h->seg_end.empty() || h->seg_end.back() != c)) h->seg_end.push_back(c);
  h->seg_end.push_back(nb);
}

template <typename T>
int create_typed(mfgpu_handle *h, const mfgpu_desc &d) {
  int rc = create_arrays<T>(h, d);
  if (rc) return rc;
  choose_segments(h, d.cell_loop_segments);
  if (!h->twopass) return 0;
  if (h->seg_end.size() > 1) {
    // lowest priority: when a segment ends, the next segment's workgroups should be placed before the pass-2 waves,
    // which fill the remaining wave slots
    int prio_least = 0, prio_greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    if ((rc = h->side.create(hipStreamNonBlocking, prio_least))) return rc;
    if ((rc = h->ev_side.create(hipEventDisableTiming))) return rc;
    h->ev_seg.resize(h->seg_end.size() - 1);
    for (Event &e : h->ev_seg)
      if ((rc = e.create(hipEventDisableTiming))) return rc;
  }
  return upload_pass2(h, nullptr, 0);
}

// one vmult in three phases: the cell loop (with pass 2 of the earlier segments' dofs on the side stream); pass 2 of
// the priority dofs; pass 2 of the last segment's dofs and the join with the side stream.  mfgpu_vmult runs them back
// to back; mfgpu_vmult_dist_begin starts the exchange of the slab's interface planes between the last two.
template <typename T>
int launch_pass2_group(mfgpu_handle *h, size_t group, void *dst, const void *src, hipStream_t st, int add) {
  if (h->p2_shared && group == 1)  // owner batches in reverse execution order while the halo buffer fits the cache
    HIP_TRY(reduce_owner_batches_launch<T>((T *)dst, (const T *)src, h->d_halo.as<const T>(), h->d_p2rec.get(),
                                           h->d_p2tab.get(), (uint32_t)(h->plan.batch_cell_off.size() - 1),
                                           (uint32_t)p_hs(h->plan.n) * 64u, h->p2_reverse ? 1 : 0, add, st));
  HIP_TRY(reduce_classes_launch<T>((T *)dst, (const T *)src, h->d_halo.as<const T>(), h->d_p2arr[group].get(),
                                   h->d_p2tiles[group].get(), h->n_p2tiles[group], add, st));
  return 0;
}

template <typename T>
int vmult_pass2(mfgpu_handle *h, int phase, void *dst, const void *src, hipStream_t st, int add) {
  if (!h->twopass) return 0;
  if (phase == 0) return launch_pass2_group<T>(h, 0, dst, src, st, add);
  int rc = launch_pass2_group<T>(h, h->seg_end.size(), dst, src, st, add);
  if (!rc && h->side_pending) {
    HIP_TRY(hipStreamWaitEvent(st, h->ev_side.get(), 0));
    h->side_pending = false;
  }
  return rc;
}

// batches [b0, b1) of one scatter pass, each with the kernel family that owns it
template <typename T>
int launch_cells(mfgpu_handle *h, ApplyArgs<T> a, uint32_t b0, uint32_t b1, hipStream_t st) {
  const Plan &P = h->plan;
  const uint32_t npl = P.n_plane_batches, nplain = P.n_plain_plane_batches;
  if (b0 < nplain) {  // the batches of cells without a hanging-node mask (all batches on conforming meshes)
    a.batch0 = b0;
    a.batch_end = b1 < nplain ? b1 : nplain;
    if (const int rc = launch_bound(h, h->kernel<T>(mfgpu_handle::kPlain), a, a.batch_end - a.batch0, st)) return rc;
    b0 = a.batch_end;
  }
  if (b0 < npl && b0 < b1) {  // plane batches of cells WITH a mask
    a.batch0 = b0;
    a.batch_end = b1 < npl ? b1 : npl;
    if (const int rc = launch_bound(h, h->kernel<T>(mfgpu_handle::kMasked), a, a.batch_end - a.batch0, st)) return rc;
    b0 = a.batch_end;
  }
  if (b0 >= b1) return 0;
  a.batch0 = b0;
  a.batch_end = b1;
  return launch_bound(h, h->kernel<T>(mfgpu_handle::kBatch), a, b1 - b0, st);
}

template <typename T>
ApplyArgs<T> make_args(mfgpu_handle *h, void *dst, const void *src, int add) {
  const Plan &P = h->plan;
  ApplyArgs<T> a;
  a.batch_cell_off = h->d_batch_cell_off.get();
  a.batch_dof_off = h->d_batch_dof_off.get();
  a.bdofs = h->d_bdofs.get();
  a.bflags = h->d_bflags.get();
  a.lmap = h->d_lmap.get();
  a.lmapx = h->d_lmapx.get();
  a.perm = h->d_perm.get();
  a.bdofsp = h->d_bdofsp.get();
  a.idxp = h->d_idxp.get();
  a.shtab = h->shared_records ? h->d_shtab.get() : nullptr;
  a.hnrec = h->d_hnrec.get();
  a.hn_slot = h->d_hn_slot.get();
  a.coefp = h->d_coefp.as<const T>();
  a.coef = h->d_coef.as<const T>();
  a.mass = h->d_mass.as<const T>();
  a.massp = h->d_massp.as<const T>();
  a.cmask = h->d_cmask.get();
  a.hn_weights = h->d_hnw.as<const T>();
  a.tabS = h->d_tabsd.as<const T>();
  a.tabDt = a.tabS ? a.tabS + (size_t)P.n * P.n : nullptr;
  a.batch_nint = h->d_batch_nint.get();
  a.halo_off = h->d_halo_off.get();
  a.halo = h->d_halo.as<T>();
  a.dst = (T *)dst;
  a.src = (const T *)src;
  a.nb_max = P.max_batch_dofs;
  a.add = add;
  a.stamps = h->d_stamps.get();
  a.dbg = 0;
  return a;
}

template <typename T>
int vmult_main(mfgpu_handle *h, void *dst, const void *src, hipStream_t st, int add) {
  const Plan &P = h->plan;
  ApplyArgs<T> a = make_args<T>(h, dst, src, add);
  int rc;
  if (h->prof && (rc = h->t_cells.begin(st))) return rc;
  if (h->twopass) {
    // ONE sweep over all batches (no inter-batch dependency) in segments; after every segment but the last, the
    // shared-dof sums that are complete by then start on the side stream
    const size_t nseg = h->seg_end.size();
    if (h->side_pending) {  // (a caller that ran phase 0 twice without the closing phase)
      HIP_TRY(hipStreamWaitEvent(st, h->ev_side.get(), 0));
      h->side_pending = false;
    }
    for (size_t s = 0; s < nseg; ++s) {
      if ((rc = launch_cells<T>(h, a, s ? h->seg_end[s - 1] : 0u, h->seg_end[s], st))) return rc;
      if (s + 1 < nseg) {
        HIP_TRY(hipEventRecord(h->ev_seg[s].get(), st));
        HIP_TRY(hipStreamWaitEvent(h->side.get(), h->ev_seg[s].get(), 0));
        if ((rc = launch_pass2_group<T>(h, 1 + s, dst, src, h->side.get(), add))) return rc;
      }
    }
    if (nseg > 1) {
      HIP_TRY(hipEventRecord(h->ev_side.get(), h->side.get()));
      h->side_pending = true;
    }
  } else {
    // coloured mode: one launch per batch colour (first toucher stores, later colours add)
    for (size_t c = 0; c + 1 < P.color_batch_off.size(); ++c) {
      if (P.color_batch_off[c + 1] == P.color_batch_off[c]) continue;
      if ((rc = launch_cells<T>(h, a, P.color_batch_off[c], P.color_batch_off[c + 1], st))) return rc;
    }
  }
  if (h->prof && (rc = h->t_cells.end(st))) return rc;
  if (!h->twopass)  // coloured mode has no pass 2: the dofs no cell touches get their own small kernel
    HIP_TRY(orphan_launch<T>((T *)dst, (const T *)src, h->d_orphans.get(), (uint32_t)P.orphans.size(), add, st));
  if (h->prof) h->prof_vmults++;
  return 0;
}

template <typename T>
int vmult_typed(mfgpu_handle *h, void *dst, const void *src, hipStream_t st, int add) {
  int rc = vmult_main<T>(h, dst, src, st, add);
  if (rc) return rc;
  const bool timed = h->prof && h->twopass;
  if (timed && (rc = h->t_pass2.begin(st))) return rc;
  rc = vmult_pass2<T>(h, 0, dst, src, st, add);
  if (!rc) rc = vmult_pass2<T>(h, 1, dst, src, st, add);
  if (!rc && timed) rc = h->t_pass2.end(st);
  return rc;
}

// ---- mfgpu_vmult_multi
// Where the default mode fuses: measured per-vector time of fused groups against MFGPU_MULTI_LOOP on the BALL domain
// (tools/bench_multi.py, profiles/r08_bench_multi.json, profiles/r08_notes.md).  Fused only where it won by more than
// the run-to-run spread of that measurement; MFGPU_MULTI_FUSED reaches every bound instantiation regardless.
bool fused_by_default(int /*n*/, int /*number_type*/) { return false; }

// one fused group of nv vectors: the cell loop in one segment, then every pass-2 group, all on st
template <typename T>
int multi_fused_group(mfgpu_handle *h, T *dst, const T *src, int nv, size_t stride, hipStream_t st, int add) {
  const MultiKernel<T> &k = h->multi<T>(nv);
  if (!k.launch[0]) {
    set_error("fused kernel not bound");
    return MFGPU_EINVAL;
  }
  if (!h->d_halo_multi.get()) {
    const size_t bytes = (size_t)(h->multi_width - 1) * h->halo_bytes;
    // zeroed (the untouched dofs' slot stays zero), and complete before a kernel on a non-blocking stream reads the slot
    if (const int rc = h->d_halo_multi.alloc(bytes, true)) return rc;
    h->device_bytes += bytes;
  }
  if (h->side_pending) {
    HIP_TRY(hipStreamWaitEvent(st, h->ev_side.get(), 0));
    h->side_pending = false;
  }
  MultiArgs<T> a;
  static_cast<ApplyArgs<T> &>(a) = make_args<T>(h, dst, src, add);
  a.stride = stride;
  for (int v = 0; v < kMaxFusedWidth; ++v)
    a.halos[v] = v == 0 ? a.halo
                 : v < nv ? reinterpret_cast<T *>(static_cast<char *>(h->d_halo_multi.get()) + (size_t)(v - 1) * h->halo_bytes)
                          : nullptr;
  const uint32_t nbat = (uint32_t)(h->plan.batch_cell_off.size() - 1);
  a.batch0 = 0;
  a.batch_end = nbat;
  if (const int rc = launch_bound(h, k, a, nbat, st)) return rc;
  for (size_t g = 0; g < h->d_p2arr.size(); ++g)
    HIP_TRY(reduce_classes_multi_launch<T>(nv, dst, src, stride, a.halos, h->d_p2arr[g].get(), h->d_p2tiles[g].get(),
                                           h->n_p2tiles[g], add, st));
  return 0;
}

template <typename T>
int vmult_multi_typed(mfgpu_handle *h, void *dst, const void *src, uint32_t n_vectors, size_t stride, uint32_t flags,
                      hipStream_t st) {
  const int add = (flags & MFGPU_MULTI_ADD) ? 1 : 0;
  const bool can_fuse = h->multi_width > 1 && !h->p2_shared && n_vectors > 1;
  if ((flags & MFGPU_MULTI_FUSED) && !can_fuse) {
    set_error("mfgpu_vmult_multi: MFGPU_MULTI_FUSED, but nothing to fuse (no fused instantiation for this handle, or "
              "a single vector)");
    return MFGPU_EUNSUPPORTED;
  }
  const bool fuse = can_fuse && !(flags & MFGPU_MULTI_LOOP) &&
                    ((flags & MFGPU_MULTI_FUSED) || fused_by_default(h->n, h->number_type));
  std::vector<uint32_t> widths;
  if (fuse)
    for (const int w : kFusedWidths)
      if (h->multi<T>(w).launch[0]) widths.push_back((uint32_t)w);
  T *d = (T *)dst;
  const T *s = (const T *)src;
  for (const uint32_t g : multi_groups(n_vectors, widths)) {
    const int rc = g > 1 ? multi_fused_group<T>(h, d, s, (int)g, stride, st, add) : vmult_typed<T>(h, d, s, st, add);
    if (rc) return rc;
    d += (size_t)g * stride;
    s += (size_t)g * stride;
  }
  return 0;
}

}  // namespace

// ---- diagonal, set_constrained_values
namespace {
template <typename T>
int inverse_diagonal_typed(mfgpu_handle *h, void *diag, hipStream_t st) {
  const Plan &P = h->plan;
  const bool general = h->batches == BatchKernel::g || h->batches == BatchKernel::g2;
  if (!h->d_tab2.get()) {  // 1D tables T[2][n*n]: squared [S.^2 | G.^2], or plain [S | G] for the general-geometry path
    const int nn = h->n * h->n;
    std::vector<T> t2(2 * (size_t)nn);
    for (int i = 0; i < nn; ++i) {
      t2[i] = (T)(general ? h->sv[i] : h->sv[i] * h->sv[i]);
      t2[nn + i] = (T)(general ? h->sg[i] : h->sg[i] * h->sg[i]);
    }
    if (const int rc = h->d_tab2.upload(t2.data(), t2.size() * sizeof(T))) return rc;
    h->device_bytes += h->d_tab2.bytes();
  }
  // inv_diag.reinit(m()): zero  (laplace_operator_gpu.h:407)
  HIP_TRY(fill_launch<T>((T *)diag, P.n_dofs, T(0), st));
  // data.cell_loop(inv_diag, diag_loc_op)  (:409-410)
  const uint32_t nb = (uint32_t)(P.batch_cell_off.size() - 1), *cell_off = h->d_batch_cell_off.get();
  const uint32_t *dof_off = h->d_batch_dof_off.get(), *bdofs = h->d_bdofs.get(), *cmask = h->d_cmask.get();
  const uint16_t *lmap = h->d_lmap.get();
  const T *coef = h->d_coef.as<const T>(), *hnw = h->d_hnw.as<const T>(), *tab2 = h->d_tab2.as<const T>();
  if (h->batches == BatchKernel::g2)
    HIP_TRY(diag_general2_launch<T>(P.n, (T *)diag, nb, cell_off, dof_off, bdofs, lmap, coef, cmask, hnw, tab2, st));
  else if (h->batches == BatchKernel::g)
    HIP_TRY(diag_general_launch<T>(P.n, (T *)diag, nb, cell_off, dof_off, bdofs, lmap, coef, cmask, hnw, tab2, st));
  else
    HIP_TRY(diag_launch<T>(P.dim, P.n, (T *)diag, nb, cell_off, dof_off, bdofs, lmap, coef, cmask, hnw, tab2, st));
  // + the mass term's local diagonal, distributed the same way (tab2's first half: S, squared unless general)
  if (h->d_mass.get())
    HIP_TRY(diag_mass_launch<T>(P.dim, P.n, (T *)diag, nb, cell_off, dof_off, bdofs, lmap, h->d_mass.as<const T>(), cmask,
                                hnw, tab2, !general, st));
  // constraint_handler.set_constrained_values(inv_diag, 1.0)  (:412)
  HIP_TRY(set_values_launch<T>((T *)diag, h->d_constrained.get(), h->n_constrained, T(1), st));
  // inv_diag.invert()  (:414)
  HIP_TRY(vec_map_launch<T>(4, (T *)diag, nullptr, T(0), T(0), P.n_dofs, st));
  return 0;
}
}  // namespace


// ---- GpuVector BLAS-1 and reductions
namespace {
int vec_map(int op, void *v, const void *w, double s, double a, size_t n, int nt, void *stream) {
  if ((!v && n) || (!w && n && op <= 3)) {
    set_error("null vector");
    return MFGPU_EINVAL;
  }
  if (nt == MFGPU_F32)
    HIP_TRY(vec_map_launch<float>(op, (float *)v, (const float *)w, (float)s, (float)a, n, (hipStream_t)stream));
  else if (nt == MFGPU_F64)
    HIP_TRY(vec_map_launch<double>(op, (double *)v, (const double *)w, s, a, n, (hipStream_t)stream));
  else
    return MFGPU_EINVAL;
  return 0;
}
int vec_reduce(int op, void *v, const void *x, const void *w, double a, size_t n, int nt, void *stream, double *out) {
  if (!out || (n && (!v || (op != 2 && !w) || (op == 1 && !x)))) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  if (nt == MFGPU_F32)
    HIP_TRY(vec_reduce_launch<float>(op, (float *)v, (const float *)x, (const float *)w, (float)a, n, (hipStream_t)stream, out));
  else if (nt == MFGPU_F64)
    HIP_TRY(vec_reduce_launch<double>(op, (double *)v, (const double *)x, (const double *)w, a, n, (hipStream_t)stream, out));
  else
    return MFGPU_EINVAL;
  return 0;
}
}  // namespace


// ---- entry points of mfgpu_dist.hip (multi-GPU slab exchange) into the operator
namespace mfgpu {
int handle_number_type(const mfgpu_handle *h) { return h->number_type; }
int handle_set_priority_dofs(mfgpu_handle *h, const uint32_t *ids, uint32_t n) {
  return h->twopass ? upload_pass2(h, ids, n) : 0;
}
int handle_n_batches(const mfgpu_handle *h) { return (int)h->plan.batch_cell_off.size() - 1; }
bool handle_ranged_ok(const mfgpu_handle *h) { return h->twopass && h->seg_end.size() == 1; }
int handle_batches_touching(const mfgpu_handle *h, const uint32_t *ids, uint32_t n, std::vector<uint8_t> &flags) {
  const Plan &P = h->plan;
  std::vector<uint8_t> mark(P.n_dofs, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (ids[i] >= P.n_dofs) {
      set_error("interface dof out of range");
      return MFGPU_EINVAL;
    }
    mark[ids[i]] = 1;
  }
  const size_t nb = P.batch_cell_off.size() - 1;
  flags.assign(nb, 0);
  for (size_t b = 0; b < nb; ++b)
    for (uint32_t t = P.batch_dof_off[b]; t < P.batch_dof_off[b + 1]; ++t)
      if (mark[P.bdofs[t] & 0x7fffffffu]) {
        flags[b] = 1;
        break;
      }
  return 0;
}
int handle_cells_range(mfgpu_handle *h, uint32_t b0, uint32_t b1, void *dst, const void *src, void *stream, int add) {
  if (b0 >= b1) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (h->number_type == MFGPU_F64) return launch_cells<double>(h, make_args<double>(h, dst, src, add), b0, b1, st);
  return launch_cells<float>(h, make_args<float>(h, dst, src, add), b0, b1, st);
}
// batches [b0, b1) and [c0, c1), b1 <= c0: one launch with a hole when both lie in the plain plane batches
int handle_cells_two_ranges(mfgpu_handle *h, uint32_t b0, uint32_t b1, uint32_t c0, uint32_t c1, void *dst,
                            const void *src, void *stream, int add) {
  const uint32_t nplain = h->plan.n_plain_plane_batches, npl = h->plan.n_plane_batches;
  const bool plain = c1 <= nplain, masked = b0 >= nplain && c1 <= npl;  // both ranges in one instantiation's batches
  if (b0 >= b1 || c0 >= c1 || b1 > c0 || !(plain || masked)) {
    const int rc = handle_cells_range(h, b0, b1, dst, src, stream, add);
    return rc ? rc : handle_cells_range(h, c0, c1, dst, src, stream, add);
  }
  hipStream_t st = (hipStream_t)stream;
  auto run = [&](auto a) -> int {
    a.batch0 = b0;
    a.batch_end = c1;
    a.hole0 = b1;
    a.hole_len = c0 - b1;
    using T = typename std::remove_const<typename std::remove_pointer<decltype(a.src)>::type>::type;
    return launch_bound(h, h->kernel<T>(plain ? mfgpu_handle::kPlain : mfgpu_handle::kMasked), a, (b1 - b0) + (c1 - c0),
                        st);
  };
  return h->number_type == MFGPU_F64 ? run(make_args<double>(h, dst, src, add)) : run(make_args<float>(h, dst, src, add));
}
int handle_pass2_group(mfgpu_handle *h, int group, void *dst, const void *src, void *stream, int add) {
  if (!h->twopass) return 0;
  hipStream_t st = (hipStream_t)stream;
  return h->number_type == MFGPU_F64 ? launch_pass2_group<double>(h, (size_t)group, dst, src, st, add)
                                     : launch_pass2_group<float>(h, (size_t)group, dst, src, st, add);
}
int handle_vmult_phase(mfgpu_handle *h, int phase, void *dst, const void *src, void *stream, int add) {
  hipStream_t st = (hipStream_t)stream;
  if (h->number_type == MFGPU_F64)
    return phase == 0 ? vmult_main<double>(h, dst, src, st, add) : vmult_pass2<double>(h, phase - 1, dst, src, st, add);
  return phase == 0 ? vmult_main<float>(h, dst, src, st, add) : vmult_pass2<float>(h, phase - 1, dst, src, st, add);
}
}  // namespace mfgpu

extern "C" {

int mfgpu_create(const mfgpu_desc *desc, mfgpu_handle **out) {
  if (!desc || !out) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  const mfgpu_desc &d = *desc;
  if (!valid_number_type(d.number_type)) {
    set_error("number_type must be MFGPU_F64 or MFGPU_F32");
    return MFGPU_EINVAL;
  }
  const bool general = !(d.flags & MFGPU_UNIFORM_J0);
  if (general && (d.flags & MFGPU_COLORED_SCATTER)) {
    set_error("the general-Jacobian path (no MFGPU_UNIFORM_J0) is implemented in two-pass scatter mode only");
    return MFGPU_EUNSUPPORTED;
  }
  if (!d.JxW || !d.inv_jac || !d.shape_values || !d.shape_gradients ||
      (!d.coefficient && !d.quadrature_points)) {  // (mass_coefficient is optional)
    set_error("JxW, inv_jac, shape tables and coefficient (or quadrature_points) are required");
    return MFGPU_EINVAL;
  }
  const bool hn = (d.flags & MFGPU_HANGING_NODES) != 0;
  if (hn && (!d.constraint_mask || !d.constraint_weights)) {
    set_error("MFGPU_HANGING_NODES needs constraint_mask and constraint_weights");
    return MFGPU_EINVAL;
  }
  std::unique_ptr<mfgpu_handle, decltype(&mfgpu_destroy)> h(new mfgpu_handle(), mfgpu_destroy);
  int rc = choose_kernel_and_plan(d, h->planes, h->batches, h->plan);
  if (rc) return rc;
  h->dim = d.dim;
  h->n = d.degree + 1;
  h->nd = h->plan.nd;
  h->number_type = d.number_type;
  h->hn = hn;
  h->twopass = !(d.flags & MFGPU_COLORED_SCATTER);
  h->no_shared_records = (d.flags & MFGPU_NO_SHARED_RECORDS) != 0;
  h->updatable = (d.flags & MFGPU_UPDATABLE_COEFFICIENTS) != 0;
  const int nn = h->n * h->n;
  std::vector<double> sv(nn), sg(nn);
  for (int i = 0; i < nn; ++i) {
    sv[i] = d.number_type == MFGPU_F64 ? ((const double *)d.shape_values)[i] : ((const float *)d.shape_values)[i];
    sg[i] = d.number_type == MFGPU_F64 ? ((const double *)d.shape_gradients)[i] : ((const float *)d.shape_gradients)[i];
  }
  h->sv = sv;
  h->sg = sg;
  rc = derive_tables(h->n, sv.data(), sg.data(), h->S, h->Dt);
  if (!rc) rc = check_symmetrize(h->n, h->S, h->Dt);
  if (!rc) rc = d.number_type == MFGPU_F64 ? create_typed<double>(h.get(), d) : create_typed<float>(h.get(), d);
  if (!rc && d.n_constrained) {
    h->n_constrained = d.n_constrained;
    rc = h->d_constrained.upload(d.constrained_dofs, d.n_constrained);
    h->device_bytes += h->d_constrained.bytes();
  }
  if (rc) return rc;
  *out = h.release();
  return 0;
}

void mfgpu_destroy(mfgpu_handle *h) {
  if (!h) return;
  if (h->side.get()) hipStreamSynchronize(h->side.get());  // before any of the arrays it reads is released
  delete h;
}

int mfgpu_vmult(mfgpu_handle *h, void *dst, const void *src, void *stream) {
  if (!h || !dst || !src) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  if (dst == src) {
    set_error("vmult: dst and src must not alias");
    return MFGPU_EINVAL;
  }
  return h->number_type == MFGPU_F64 ? vmult_typed<double>(h, dst, src, (hipStream_t)stream, 0)
                                     : vmult_typed<float>(h, dst, src, (hipStream_t)stream, 0);
}

int mfgpu_vmult_add(mfgpu_handle *h, void *dst, const void *src, void *stream) {
  if (!h || !dst || !src) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  if (dst == src) {
    set_error("vmult_add: dst and src must not alias");
    return MFGPU_EINVAL;
  }
  return h->number_type == MFGPU_F64 ? vmult_typed<double>(h, dst, src, (hipStream_t)stream, 1)
                                     : vmult_typed<float>(h, dst, src, (hipStream_t)stream, 1);
}

int mfgpu_vmult_multi(mfgpu_handle *h, void *dst, const void *src, uint32_t n_vectors, size_t stride, uint32_t flags,
                      void *stream) {
  if (!h || !dst || !src) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  const size_t nd = h->plan.n_dofs;
  if (n_vectors == 0 || (n_vectors > 1 && stride < nd)) {
    set_error("mfgpu_vmult_multi: n_vectors must be >= 1 and stride >= n_dofs");
    return MFGPU_EINVAL;
  }
  if ((flags & ~(MFGPU_MULTI_ADD | MFGPU_MULTI_LOOP | MFGPU_MULTI_FUSED)) ||
      ((flags & MFGPU_MULTI_LOOP) && (flags & MFGPU_MULTI_FUSED))) {
    set_error("mfgpu_vmult_multi: bad flags (MFGPU_MULTI_LOOP and MFGPU_MULTI_FUSED exclude each other)");
    return MFGPU_EINVAL;
  }
  const size_t bytes = ((size_t)(n_vectors - 1) * stride + nd) * esize(h->number_type);
  const char *d0 = (const char *)dst, *s0 = (const char *)src;
  if (d0 < s0 + bytes && s0 < d0 + bytes) {
    set_error("mfgpu_vmult_multi: the dst range overlaps the src range");
    return MFGPU_EINVAL;
  }
  return h->number_type == MFGPU_F64 ? vmult_multi_typed<double>(h, dst, src, n_vectors, stride, flags, (hipStream_t)stream)
                                     : vmult_multi_typed<float>(h, dst, src, n_vectors, stride, flags, (hipStream_t)stream);
}

int mfgpu_multi_width(const mfgpu_handle *h) { return h ? h->multi_width : 0; }

int mfgpu_update_coefficients(mfgpu_handle *h, const void *coefficient_dev, const void *mass_coefficient_dev,
                              void *stream) {
  if (!h) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  if (!h->updatable) {
    set_error("mfgpu_update_coefficients: the handle was created without MFGPU_UPDATABLE_COEFFICIENTS");
    return MFGPU_EINVAL;
  }
  if (!coefficient_dev && !mass_coefficient_dev) {
    set_error("mfgpu_update_coefficients: coefficient_dev and mass_coefficient_dev are both NULL");
    return MFGPU_EINVAL;
  }
  if (mass_coefficient_dev && !h->d_mass.get()) {
    set_error("mfgpu_update_coefficients: the handle was created without a mass term (its kernels have no mass "
              "instantiation bound); create it with mass_coefficient");
    return MFGPU_EINVAL;
  }
  return h->number_type == MFGPU_F64 ? update_typed<double>(h, coefficient_dev, mass_coefficient_dev, (hipStream_t)stream)
                                     : update_typed<float>(h, coefficient_dev, mass_coefficient_dev, (hipStream_t)stream);
}

uint32_t mfgpu_n_dofs(const mfgpu_handle *h) { return h ? h->plan.n_dofs : 0; }

size_t mfgpu_memory_consumption(const mfgpu_handle *h) { return h ? h->device_bytes : 0; }

int mfgpu_plan_stats(const mfgpu_handle *h, uint64_t s[8]) {
  if (!h || !s) return MFGPU_EINVAL;
  const Plan &P = h->plan;
  s[0] = P.batch_cell_off.size() - 1;
  s[1] = P.color_batch_off.size() - 1;
  s[2] = P.bdofs.size();
  s[3] = P.max_batch_dofs;
  s[4] = P.max_batch_cells;
  s[5] = P.orphans.size();
  s[6] = P.n_first;
  s[7] = P.n_add;
  if (h->twopass) {  // two-pass mode reports shared dofs / halo partial sums instead
    // cell-loop launches per vmult: per segment one for each kernel instantiation that owns batches of it
    const uint32_t nb = (uint32_t)s[0], npl = P.n_plane_batches, nplain = P.n_plain_plane_batches;
    const uint32_t edge[4] = {0u, nplain, npl, nb};
    s[1] = 0;
    for (size_t g = 0; g < h->seg_end.size(); ++g) {
      const uint32_t s0 = g ? h->seg_end[g - 1] : 0u, s1 = h->seg_end[g];
      for (int f = 0; f < 3; ++f)
        if (std::max(s0, edge[f]) < std::min(s1, edge[f + 1])) ++s[1];
    }
    s[6] = P.sdofs.size();
    s[7] = P.halo_off.back();
  }
  return 0;
}

int mfgpu_record_stats(const mfgpu_handle *h, uint64_t s[4]) {
  if (!h || !s) return MFGPU_EINVAL;
  const Plan &P = h->plan;
  const size_t n = (size_t)P.n, nb = (size_t)p_kgu((int)n) * 64, nx = ((n * n + 1) / 2) * (p_cells_per_wave((int)n) * n);
  const bool planes = h->planes != PlaneKernel::none;
  s[0] = (h->shared_records ? 1 : 0) | (h->p2_shared ? 2 : 0);
  s[1] = planes ? P.sh_dofs.size() / nb : 0;
  s[2] = planes ? P.sh_idx.size() / nx : 0;
  s[3] = h->record_bytes;
  return 0;
}

const char *mfgpu_kernel_name(const mfgpu_handle *h) {
  if (!h) return "";
  const bool x = h->batches == BatchKernel::x;
  switch (h->planes) {
    case PlaneKernel::planes3: return x ? "apply_planes3+apply_batches_x" : "apply_planes3";
    case PlaneKernel::planes4: return x ? "apply_planes4+apply_batches_x" : "apply_planes4";
    default: break;
  }
  switch (h->batches) {
    case BatchKernel::x: return "apply_batches_x";
    case BatchKernel::g: return "apply_batches_g";
    case BatchKernel::g2: return "apply_batches_g2";
    default: return "apply_batches";
  }
}

int mfgpu_profile_enable(mfgpu_handle *h, int on) {
  if (!h) return MFGPU_EINVAL;
  h->prof = on != 0;
  h->t_cells.reset();
  h->t_pass2.reset();
  h->prof_vmults = 0;
  return 0;
}

int mfgpu_profile_read_pass2(mfgpu_handle *h, double *ms) {
  if (!h || !ms) return MFGPU_EINVAL;
  HIP_TRY(hipDeviceSynchronize());
  return h->t_pass2.drain(ms);
}

int mfgpu_profile_read(mfgpu_handle *h, double *ms, uint64_t *nv) {
  if (!h || !ms || !nv) return MFGPU_EINVAL;
  HIP_TRY(hipDeviceSynchronize());
  if (const int rc = h->t_cells.drain(ms)) return rc;
  *nv = h->prof_vmults;
  return 0;
}

#ifdef MFGPU_STAMPS
// diagnostic build only: allocate / read the per-workgroup phase stamps (16 u64 per batch)
int mfgpu_debug_stamps(mfgpu_handle *h, unsigned long long *out, size_t n_batches) {
  if (!h) return MFGPU_EINVAL;
  const size_t nbt = h->plan.batch_cell_off.size() - 1;
  if (!h->d_stamps.get()) return h->d_stamps.alloc(2 * nbt * 16, true);
  if (out && n_batches == nbt) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, h->d_stamps.get(), 2 * nbt * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  }
  return 0;
}
#endif

// ---- GpuVector pieces -----------------------------------------------------------------------

// ---- diagonal, set_constrained_values
int mfgpu_compute_inverse_diagonal(mfgpu_handle *h, void *inv_diag, void *stream) {
  if (!h || !inv_diag) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  return h->number_type == MFGPU_F64 ? inverse_diagonal_typed<double>(h, inv_diag, (hipStream_t)stream)
                                     : inverse_diagonal_typed<float>(h, inv_diag, (hipStream_t)stream);
}

int mfgpu_set_constrained_values(mfgpu_handle *h, void *vec, double value, void *stream) {
  if (!h || !vec) {
    set_error("null argument");
    return MFGPU_EINVAL;
  }
  if (h->number_type == MFGPU_F64)
    HIP_TRY(set_values_launch<double>((double *)vec, h->d_constrained.get(), h->n_constrained, value, (hipStream_t)stream));
  else
    HIP_TRY(set_values_launch<float>((float *)vec, h->d_constrained.get(), h->n_constrained, (float)value,
                                     (hipStream_t)stream));
  return 0;
}

// ---- GpuVector BLAS-1 and reductions
int mfgpu_vec_sadd(void *v, double s, double a, const void *w, size_t n, int nt, void *stream) {
  return vec_map(0, v, w, s, a, n, nt, stream);
}
int mfgpu_vec_equ(void *v, double a, const void *w, size_t n, int nt, void *stream) {
  return vec_map(1, v, w, 0.0, a, n, nt, stream);
}
int mfgpu_vec_scale(void *v, const void *w, size_t n, int nt, void *stream) {
  return vec_map(2, v, w, 0.0, 0.0, n, nt, stream);
}
int mfgpu_vec_divide(void *v, const void *w, size_t n, int nt, void *stream) {
  return vec_map(3, v, w, 0.0, 0.0, n, nt, stream);
}
int mfgpu_vec_invert(void *v, size_t n, int nt, void *stream) { return vec_map(4, v, nullptr, 0.0, 0.0, n, nt, stream); }
int mfgpu_vec_mul(void *v, double a, size_t n, int nt, void *stream) {
  return vec_map(5, v, nullptr, 0.0, a, n, nt, stream);
}
int mfgpu_vec_dot(const void *v, const void *w, size_t n, int nt, void *stream, double *result) {
  return vec_reduce(0, const_cast<void *>(v), nullptr, w, 0.0, n, nt, stream, result);
}
int mfgpu_vec_l2_norm(const void *v, size_t n, int nt, void *stream, double *result) {
  int rc = vec_reduce(0, const_cast<void *>(v), nullptr, v, 0.0, n, nt, stream, result);
  if (!rc) *result = std::sqrt(*result);
  return rc;
}
int mfgpu_vec_add_and_dot(void *v, double a, const void *x, const void *w, size_t n, int nt, void *stream,
                          double *result) {
  return vec_reduce(1, v, x, w, a, n, nt, stream, result);
}
int mfgpu_vec_all_zero(const void *v, size_t n, int nt, void *stream, int *result) {
  if (!result) return MFGPU_EINVAL;
  double cnt = 0.0;
  int rc = vec_reduce(2, const_cast<void *>(v), nullptr, nullptr, 0.0, n, nt, stream, &cnt);
  if (!rc) *result = cnt == 0.0;
  return rc;
}

int mfgpu_vec_alloc(void **dev, size_t n, int nt) {
  if (!dev) return MFGPU_EINVAL;
  *dev = nullptr;
  if (n == 0) return 0;
  HIP_TRY(hipMalloc(dev, n * esize(nt)));
  HIP_TRY(hipMemset(*dev, 0, n * esize(nt)));
  HIP_TRY(hipStreamSynchronize(nullptr));  // (as DeviceArray::alloc: zero for a reader on a non-blocking stream too)
  return 0;
}
int mfgpu_vec_free(void *dev) {
  if (dev) HIP_TRY(hipFree(dev));
  return 0;
}
int mfgpu_vec_fill(void *dev, size_t n, int nt, double value, void *stream) {
  if (!dev && n) return MFGPU_EINVAL;
  if (nt == MFGPU_F32)
    HIP_TRY(fill_launch<float>((float *)dev, n, (float)value, (hipStream_t)stream));
  else
    HIP_TRY(fill_launch<double>((double *)dev, n, value, (hipStream_t)stream));
  return 0;
}
int mfgpu_vec_from_host(void *dev, const void *host, size_t n, int nt) {
  if (n) HIP_TRY(hipMemcpy(dev, host, n * esize(nt), hipMemcpyHostToDevice));
  return 0;
}
int mfgpu_vec_to_host(void *host, const void *dev, size_t n, int nt) {
  if (n) HIP_TRY(hipMemcpy(host, dev, n * esize(nt), hipMemcpyDeviceToHost));
  return 0;
}
int mfgpu_device_synchronize(void) {
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}
int mfgpu_device_memory_info(size_t *free_bytes, size_t *total_bytes) {
  if (!free_bytes || !total_bytes) return MFGPU_EINVAL;
  HIP_TRY(hipMemGetInfo(free_bytes, total_bytes));
  return 0;
}

}  // extern "C"
