// poisson_amr: the adaptive loop solve -> estimate -> mark -> refine -> transfer -> solve on the
// reference's Poisson problem (poisson.cu: variable coefficient, right-hand side and Dirichlet values of Solution<dim>),
// started from the cube refined n_start_ref times.  Per cycle: the leaf mesh, its operator and integrator; the
// global-coarsening V-cycle of poisson_gc.cc (mfgpu_mesh_coarsen_leaves, mfgpu_transfer_create_h_hn_from_meshes,
// mfgpu_vcycle) under the device CG to 1e-12 |b|; the L2 error and the gradient-recovery indicator
// (mfgpu_integrator_recovery_indicator), eta = sqrt(sum eta_K^2); the ceil(fraction n) cells of largest eta_K^2 are marked
// (ties: the lower cell index; GridRefinement::refine_and_coarsen_fixed_number without coarsening) and refined by
// mfgpu_mesh_refine_leaves (execute_coarsening_and_refinement).  The solution is carried over like SolutionTransfer: its
// homogeneous part x (u = lift + x, x = 0 on the Dirichlet dofs) is prolongated by the h_hn transfer of the mesh pair,
// which reads the coarse Dirichlet dofs as 0.  The device CG starts from zero, so the next cycle solves
// A delta = b - A x~ for the correction of the prolongated x~; the same system is also solved from zero (A x = b) to show
// what the start is worth.  Written on the C-ABI alone.
// Output, one line per cycle:  cycle  cells  dofs  cg_iterations  cg_iterations_from_zero  l2_error  eta  seconds
// (seconds: set-up, solve, error and indicator of the cycle; the comparison solve from zero and the refinement are not in it)
// usage: poisson-amr-<dim>d-p<k> n_start_ref n_cycles [fraction = 0.3]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <iostream>
#include <memory>
#include <numeric>
#include <vector>

#include "mfgpu_shim_poisson.h"

using namespace mfgpu_shim;

#ifndef DEGREE_FE
#define DEGREE_FE 2
#endif
#ifndef DIMENSION
#define DIMENSION 2
#endif

namespace {

// the active mesh with its coarsenings, operators, transfers, V-cycle and CG; everything is released in reverse order
struct Level {
  std::vector<mfgpu_mesh *> meshes;  // coarse to fine; meshes.back() is the active mesh
  std::vector<mfgpu_handle *> ops;
  std::vector<mfgpu_transfer *> transfers;
  mfgpu_vcycle *vcycle = nullptr;
  mfgpu_cg *cg = nullptr;
  mfgpu_integrator *integrator = nullptr;
  ~Level() {
    mfgpu_integrator_destroy(integrator);
    mfgpu_cg_destroy(cg);
    mfgpu_vcycle_destroy(vcycle);
    for (mfgpu_transfer *t : transfers) mfgpu_transfer_destroy(t);
    for (mfgpu_handle *h : ops) mfgpu_destroy(h);
    for (mfgpu_mesh *m : meshes) mfgpu_mesh_destroy(m);
  }
  mfgpu_mesh *mesh() const { return meshes.back(); }
  mfgpu_handle *op() const { return ops.back(); }
};

std::unique_ptr<Level> build(int dim, int degree, const std::vector<uint32_t> &leaves) {
  std::unique_ptr<Level> L(new Level());
  mfgpu_mesh *m = nullptr;
  check(mfgpu_mesh_create_from_leaves(dim, degree, leaves.data(), (uint32_t)(leaves.size() / 4), MFGPU_F64, &m), "active mesh");
  L->meshes.push_back(m);
  for (;;) {  // -gc-'s set-up: fine to coarse first
    const uint32_t *lv = nullptr;
    const int64_t n_fine = mfgpu_mesh_cell_levels(L->meshes.back(), &lv) / 4;
    if (n_fine <= 1) break;
    std::vector<uint32_t> coarse((size_t)n_fine * 4);
    const int64_t n_coarse = mfgpu_mesh_coarsen_leaves(dim, lv, (uint32_t)n_fine, coarse.data());
    if (n_coarse < 0) check((int)n_coarse, "mfgpu_mesh_coarsen_leaves");
    if (n_coarse < (1 << dim)) break;
    check(mfgpu_mesh_create_from_leaves(dim, degree, coarse.data(), (uint32_t)n_coarse, MFGPU_F64, &m), "coarsened mesh");
    L->meshes.push_back(m);
  }
  std::reverse(L->meshes.begin(), L->meshes.end());
  const unsigned int nlevels = (unsigned int)L->meshes.size();
  std::vector<mfgpu_vcycle_level_desc> levels(nlevels);
  L->transfers.assign(nlevels, nullptr);
  for (unsigned int l = 0; l < nlevels; ++l) {
    mfgpu_desc d;
    check(mfgpu_mesh_desc(L->meshes[l], &d), "mesh desc");
    mfgpu_handle *op = nullptr;
    check(mfgpu_create(&d, &op), "level operator");
    L->ops.push_back(op);
    if (l > 0) check(mfgpu_transfer_create_h_hn_from_meshes(L->meshes[l - 1], L->meshes[l], &L->transfers[l]), "level transfer");
    levels[l] = mfgpu_vcycle_level_desc{};
    levels[l].op = op;
    levels[l].from_coarser = L->transfers[l];
  }
  mfgpu_vcycle_desc vd{};
  vd.n_levels = nlevels;
  vd.levels = levels.data();
  vd.active_type = MFGPU_F64;
  vd.n_active = mfgpu_n_dofs(L->op());
  vd.smoother_degree = 5;
  vd.smoothing_range = 15.;
  vd.eig_iterations = 15;
  vd.lambda_max = nullptr;
  vd.coarse = MFGPU_VCYCLE_COARSE_AUTO;
  check(mfgpu_vcycle_create(&vd, &L->vcycle), "mfgpu_vcycle_create");
  check(mfgpu_cg_create(L->op(), MFGPU_CG_CALLBACK, nullptr, 0, 0, 0, &L->cg), "mfgpu_cg_create");
  check(mfgpu_cg_set_vcycle(L->cg, L->vcycle), "mfgpu_cg_set_vcycle");
  mfgpu_desc d;
  check(mfgpu_mesh_desc(L->mesh(), &d), "mesh desc");
  d.flags |= MFGPU_UPDATABLE_COEFFICIENTS;  // the indicator needs inv_jac on the device
  check(mfgpu_integrator_create(&d, &L->integrator), "mfgpu_integrator_create");
  return L;
}

unsigned int cg_solve(Level &L, GpuVector<double> &x, const GpuVector<double> &b, double tolerance) {
  mfgpu_cg_info info{};
  check(mfgpu_cg_solve(L.cg, x.getData(), b.getDataRO(), tolerance, 1000, 10, nullptr, &info), "mfgpu_cg_solve");
  if (info.status != 1) throw std::runtime_error("poisson_amr: CG did not converge");
  return info.iterations;
}

template <int dim>
int run(int degree, int n_start_ref, int n_cycles, double fraction) {
  std::vector<uint32_t> leaves;
  const uint32_t n = 1u << n_start_ref;
  for (uint32_t k = 0; k < (dim == 3 ? n : 1u); ++k)
    for (uint32_t j = 0; j < n; ++j)
      for (uint32_t i = 0; i < n; ++i) leaves.insert(leaves.end(), {(uint32_t)n_start_ref, i, j, k});
  GpuVector<double> start;  // the prolongated homogeneous part of the previous cycle
  std::printf("# cycle cells dofs cg_iterations cg_iterations_from_zero l2_error eta seconds\n");
  for (int cycle = 0; cycle < n_cycles; ++cycle) {
    mfgpu_device_synchronize();
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_ptr<Level> L = build(dim, degree, leaves);
    mfgpu_desc d;
    check(mfgpu_mesh_desc(L->mesh(), &d), "mesh desc");
    const unsigned int N = d.n_dofs, n_cells = d.n_cells;
    // Dirichlet values (of every constrained dof; the hanging ones are never read), load vector with the lift
    const double *xy = nullptr;
    check(mfgpu_mesh_dof_coords(L->mesh(), &xy) < 0 ? -1 : 0, "mfgpu_mesh_dof_coords");
    std::vector<double> ub(N, 0.0);
    const Solution<dim> solution;
    for (uint32_t i = 0; i < d.n_constrained; ++i) ub[d.constrained_dofs[i]] = solution.value(xy + (size_t)d.constrained_dofs[i] * dim);
    GpuVector<double> lift(ub), b(N), x(N), delta(N), u(N);
    check(mfgpu_integrator_rhs(L->integrator, b.getData(), nullptr, lift.getDataRO(), nullptr), "mfgpu_integrator_rhs");
    const double tolerance = 1e-12 * b.l2_norm();
    unsigned int its = 0;
    if (cycle == 0) {
      its = cg_solve(*L, x, b, tolerance);
    } else {
      x.equ(1, start);
      check(mfgpu_set_constrained_values(L->op(), x.getData(), 0.0, nullptr), "set_constrained_values");
      GpuVector<double> r(N);
      check(mfgpu_vmult(L->op(), r.getData(), x.getDataRO(), nullptr), "vmult");
      r.sadd(-1, 1, b);  // b - A x~; 0 on the constrained rows, where x~ is 0
      its = cg_solve(*L, delta, r, tolerance);
      x.add(1, delta);
    }
    u.equ(1, x);
    u.add(1, lift);
    double l2 = 0;
    check(mfgpu_integrator_l2_error(L->integrator, u.getDataRO(), nullptr, nullptr, nullptr, &l2), "mfgpu_integrator_l2_error");
    GpuVector<double> eta2(n_cells);
    check(mfgpu_integrator_recovery_indicator(L->integrator, u.getDataRO(), nullptr, eta2.getData(), nullptr),
          "mfgpu_integrator_recovery_indicator");
    const std::vector<double> e = eta2.toVector();  // n_cells doubles read back once per cycle
    const double eta = std::sqrt(std::accumulate(e.begin(), e.end(), 0.0));
    mfgpu_device_synchronize();
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    // for the comparison only, outside the timed interval: the same system from zero
    const unsigned int its_zero = cycle == 0 ? its : cg_solve(*L, delta, b, tolerance);
    std::printf("%d %u %u %u %u %.10e %.10e %.4g\n", cycle, n_cells, N, its, its_zero, l2, eta, wall);
    if (cycle + 1 == n_cycles) break;
    // mark the ceil(fraction n) largest, ties to the lower index; refine; carry x over
    std::vector<uint32_t> order(n_cells);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t c) { return e[a] > e[c]; });
    const size_t n_mark = std::min<size_t>(n_cells, (size_t)std::ceil(fraction * n_cells));
    std::vector<uint8_t> flags(n_cells, 0);
    for (size_t i = 0; i < n_mark; ++i) flags[order[i]] = 1;
    const uint32_t *lv = nullptr;
    check(mfgpu_mesh_cell_levels(L->mesh(), &lv) < 0 ? -1 : 0, "mfgpu_mesh_cell_levels");
    std::vector<uint32_t> fine((size_t)n_cells * 4 << dim);
    const int64_t n_fine = mfgpu_mesh_refine_leaves(dim, lv, n_cells, flags.data(), 0, fine.data(), (uint64_t)n_cells << dim);
    if (n_fine < 0) check((int)n_fine, "mfgpu_mesh_refine_leaves");
    fine.resize((size_t)n_fine * 4);
    mfgpu_mesh *next = nullptr;
    check(mfgpu_mesh_create_from_leaves(dim, degree, fine.data(), (uint32_t)n_fine, MFGPU_F64, &next), "refined mesh");
    mfgpu_transfer *carry = nullptr;
    int rc = mfgpu_transfer_create_h_hn_from_meshes(L->mesh(), next, &carry);
    if (rc == 0) {
      mfgpu_desc nd;
      rc = mfgpu_mesh_desc(next, &nd);
      if (rc == 0) {
        start.reinit(nd.n_dofs);
        rc = mfgpu_transfer_prolongate(carry, start.getData(), x.getDataRO(), nullptr);
        mfgpu_device_synchronize();
      }
    }
    mfgpu_transfer_destroy(carry);
    mfgpu_mesh_destroy(next);
    check(rc, "solution transfer");
    leaves.swap(fine);
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  try {
    const int n_start_ref = argc > 1 ? atoi(argv[1]) : 2;
    const int n_cycles = argc > 2 ? atoi(argv[2]) : 3;
    const double fraction = argc > 3 ? atof(argv[3]) : 0.3;
    if (n_start_ref < 1 || n_start_ref > 12 || n_cycles < 1 || !(fraction >= 0.0 && fraction <= 1.0)) {
      std::cerr << "usage: poisson-amr n_start_ref (1..12) n_cycles (>= 1) [fraction in [0, 1]]" << std::endl;
      return 1;
    }
    return run<DIMENSION>(DEGREE_FE, n_start_ref, n_cycles, fraction);
  } catch (std::exception &exc) {
    std::cerr << "Exception on processing: " << exc.what() << std::endl;
    return 1;
  }
}
