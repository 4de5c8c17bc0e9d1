// heat_amr: a moving feature on a mesh that follows it.  u_t - Laplace u = f on the cube (-1, 1)^dim
// with the manufactured solution u(x, t) = exp(-|x - c(t)|^2 / w^2), c(t) = R (cos 2 pi t, sin 2 pi t, 0): a Gaussian whose
// centre moves along a circle; f and the Dirichlet values come from it.  Implicit Euler: per step the operator
// -Laplace + 1/dt (mfgpu_desc.mass_coefficient) is solved for the homogeneous part x of u = lift + x by the
// global-coarsening V-cycle of poisson_gc.cc under the device CG; the right-hand side is mfgpu_integrator_rhs of
// f(t_new) + u_old / dt at the quadrature points (u_old there by mfgpu_integrator_evaluate) with the lift of the new
// Dirichlet values.  Then the mesh is adapted in BOTH directions: the gradient-recovery indicator, the
// ceil(refine_fraction n) largest marked for refinement and the floor(coarsen_fraction n) smallest of the others for
// coarsening (ties: the lower cell index), mfgpu_mesh_adapt_leaves, and x carried over through the common coarsening:
// mfgpu_transfer_interpolate on (mid, old), mfgpu_transfer_prolongate on (mid, new).  Written on the C-ABI alone.
// Output, one line per step:  step  time  cells  dofs  families_coarsened  leaves_refined  cg_iterations  l2_error
// (families_coarsened and leaves_refined: what the adaptation AFTER the step's solve did); then, when the uniform mesh of
// the finest level reached has at most 2^16 cells, the same run on that mesh without adaptation.
// usage: heat-amr-<dim>d-p<k> n_start_ref n_steps [refine_fraction = 0.1 coarsen_fraction = 0.6 [dt = 0.05]]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <iostream>
#include <memory>
#include <numeric>
#include <vector>

#include "mfgpu_shim.h"

using namespace mfgpu_shim;

#ifndef DEGREE_FE
#define DEGREE_FE 2
#endif
#ifndef DIMENSION
#define DIMENSION 2
#endif

namespace {

const double kPi = 3.14159265358979323846, kRadius = 0.4, kWidth = 0.25;

template <int dim>
double exact(const double *x, double t) {
  const double c[3] = {kRadius * std::cos(2 * kPi * t), kRadius * std::sin(2 * kPi * t), 0.0};
  double r2 = 0;
  for (int d = 0; d < dim; ++d) r2 += (x[d] - c[d]) * (x[d] - c[d]);
  return std::exp(-r2 / (kWidth * kWidth));
}

// f = u_t - Laplace u
template <int dim>
double load(const double *x, double t) {
  const double w2 = kWidth * kWidth;
  const double c[3] = {kRadius * std::cos(2 * kPi * t), kRadius * std::sin(2 * kPi * t), 0.0};
  const double cdot[3] = {-2 * kPi * kRadius * std::sin(2 * kPi * t), 2 * kPi * kRadius * std::cos(2 * kPi * t), 0.0};
  double r2 = 0, drift = 0;
  for (int d = 0; d < dim; ++d) {
    r2 += (x[d] - c[d]) * (x[d] - c[d]);
    drift += (x[d] - c[d]) * cdot[d];
  }
  const double u = std::exp(-r2 / w2);
  return u * (2 * drift / w2 - 4 * r2 / (w2 * w2) + 2 * dim / w2);
}

// the active mesh with its coarsenings, operators (-Laplace + 1/dt), transfers, V-cycle and CG; released in reverse order
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

std::unique_ptr<Level> build(int dim, int degree, const std::vector<uint32_t> &leaves, double inv_dt) {
  std::unique_ptr<Level> L(new Level());
  mfgpu_mesh *m = nullptr;
  check(mfgpu_mesh_create_from_leaves(dim, degree, leaves.data(), (uint32_t)(leaves.size() / 4), MFGPU_F64, &m), "active mesh");
  L->meshes.push_back(m);
  for (;;) {
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
  std::vector<double> one, mass;
  for (unsigned int l = 0; l < nlevels; ++l) {
    mfgpu_desc d;
    check(mfgpu_mesh_desc(L->meshes[l], &d), "mesh desc");
    const size_t nq = (size_t)d.n_cells * (size_t)std::lround(std::pow(degree + 1, dim));
    one.assign(nq, 1.0);
    mass.assign(nq, inv_dt);
    d.coefficient = one.data();
    d.mass_coefficient = mass.data();
    mfgpu_handle *op = nullptr;
    check(mfgpu_create(&d, &op), "level operator");
    L->ops.push_back(op);
    if (l > 0) check(mfgpu_transfer_create_h_hn_from_meshes(L->meshes[l - 1], L->meshes[l], &L->transfers[l]), "level transfer");
    levels[l] = mfgpu_vcycle_level_desc{};
    levels[l].op = op;
    levels[l].from_coarser = L->transfers[l];
    if (l + 1 == nlevels) {
      d.flags |= MFGPU_UPDATABLE_COEFFICIENTS;  // the indicator needs inv_jac on the device
      check(mfgpu_integrator_create(&d, &L->integrator), "mfgpu_integrator_create");
    }
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
  return L;
}

// the exact solution at the constrained dofs (the hanging ones are never read), 0 elsewhere
template <int dim>
std::vector<double> dirichlet_values(const Level &L, const mfgpu_desc &d, double t) {
  const double *xy = nullptr;
  check(mfgpu_mesh_dof_coords(L.mesh(), &xy) < 0 ? -1 : 0, "mfgpu_mesh_dof_coords");
  std::vector<double> ub(d.n_dofs, 0.0);
  for (uint32_t i = 0; i < d.n_constrained; ++i) ub[d.constrained_dofs[i]] = exact<dim>(xy + (size_t)d.constrained_dofs[i] * dim, t);
  return ub;
}

std::vector<uint32_t> uniform_leaves(int dim, int level) {
  std::vector<uint32_t> leaves;
  const uint32_t n = 1u << level;
  for (uint32_t k = 0; k < (dim == 3 ? n : 1u); ++k)
    for (uint32_t j = 0; j < n; ++j)
      for (uint32_t i = 0; i < n; ++i) leaves.insert(leaves.end(), {(uint32_t)level, i, j, k});
  return leaves;
}

// the run; returns the finest level met.  adapt = false: the mesh stays as it is
template <int dim>
int run(int degree, std::vector<uint32_t> leaves, int n_steps, double refine_fraction, double coarsen_fraction, double dt,
        bool adapt) {
  const int nd = (int)std::lround(std::pow(degree + 1, dim)), ne = (int)std::lround(std::pow(degree + 2, dim));
  GpuVector<double> x;  // the homogeneous part of the solution at the current time, on the current mesh
  double t = 0;
  int finest = 0;
  std::printf("# step time cells dofs families_coarsened leaves_refined cg_iterations l2_error\n");
  for (int step = 0; step < n_steps; ++step) {
    std::unique_ptr<Level> L = build(dim, degree, leaves, 1.0 / dt);
    mfgpu_desc d;
    check(mfgpu_mesh_desc(L->mesh(), &d), "mesh desc");
    const unsigned int N = d.n_dofs, n_cells = d.n_cells;
    const uint32_t *lv = nullptr;
    check(mfgpu_mesh_cell_levels(L->mesh(), &lv) < 0 ? -1 : 0, "mfgpu_mesh_cell_levels");
    for (uint32_t c = 0; c < n_cells; ++c) finest = std::max(finest, (int)lv[4 * c]);
    if (step == 0) {  // the nodal interpolant of the initial value
      const double *xy = nullptr;
      check(mfgpu_mesh_dof_coords(L->mesh(), &xy) < 0 ? -1 : 0, "mfgpu_mesh_dof_coords");
      std::vector<double> u0(N);
      for (unsigned int i = 0; i < N; ++i) u0[i] = exact<dim>(xy + (size_t)i * dim, 0.0);
      x = u0;
    }
    check(mfgpu_set_constrained_values(L->op(), x.getData(), 0.0, nullptr), "set_constrained_values");
    // u_old at the quadrature points, then f(t_new) + u_old / dt there
    GpuVector<double> u(N), lift_old(dirichlet_values<dim>(*L, d, t)), old_qp((unsigned int)((size_t)n_cells * nd));
    u.equ(1, x);
    u.add(1, lift_old);
    check(mfgpu_integrator_evaluate(L->integrator, u.getDataRO(), old_qp.getData(), nullptr, nullptr), "mfgpu_integrator_evaluate");
    t += dt;
    const double *xq = static_cast<const double *>(d.quadrature_points);
    std::vector<double> f_host((size_t)n_cells * nd);
    for (size_t q = 0; q < f_host.size(); ++q) f_host[q] = load<dim>(xq + q * dim, t);
    GpuVector<double> f_qp(f_host), lift(dirichlet_values<dim>(*L, d, t)), b(N), x_new(N);
    f_qp.add(1.0 / dt, old_qp);
    check(mfgpu_integrator_rhs(L->integrator, b.getData(), f_qp.getDataRO(), lift.getDataRO(), nullptr), "mfgpu_integrator_rhs");
    mfgpu_cg_info info{};
    check(mfgpu_cg_solve(L->cg, x_new.getData(), b.getDataRO(), 1e-10 * b.l2_norm(), 1000, 10, nullptr, &info), "mfgpu_cg_solve");
    if (info.status != 1) throw std::runtime_error("heat_amr: CG did not converge");
    x.swap(x_new);
    u.equ(1, x);
    u.add(1, lift);
    // the L2 error against the exact solution at the error points
    GpuVector<double> points((unsigned int)((size_t)n_cells * ne * dim));
    check(mfgpu_integrator_error_points(L->integrator, points.getData(), nullptr), "mfgpu_integrator_error_points");
    const std::vector<double> pts = points.toVector();
    std::vector<double> ex((size_t)n_cells * ne);
    for (size_t q = 0; q < ex.size(); ++q) ex[q] = exact<dim>(pts.data() + q * dim, t);
    GpuVector<double> exact_dev(ex);
    double l2 = 0;
    check(mfgpu_integrator_l2_error(L->integrator, u.getDataRO(), exact_dev.getDataRO(), nullptr, nullptr, &l2), "mfgpu_integrator_l2_error");
    unsigned int families = 0, refined = 0;
    if (adapt && step + 1 < n_steps) {
      GpuVector<double> eta2(n_cells);
      check(mfgpu_integrator_recovery_indicator(L->integrator, u.getDataRO(), nullptr, eta2.getData(), nullptr),
            "mfgpu_integrator_recovery_indicator");
      const std::vector<double> e = eta2.toVector();
      // the ceil(fr n) largest for refinement, the floor(fc n) smallest of the others for coarsening, ties: the lower index
      std::vector<uint32_t> order(n_cells);
      std::iota(order.begin(), order.end(), 0u);
      std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t c) { return e[a] > e[c]; });
      const size_t n_refine = std::min<size_t>(n_cells, (size_t)std::ceil(refine_fraction * n_cells));
      std::vector<uint8_t> rf(n_cells, 0), cf(n_cells, 0);
      for (size_t i = 0; i < n_refine; ++i) rf[order[i]] = 1;
      std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t c) { return e[a] < e[c]; });
      size_t n_coarsen = (size_t)std::floor(coarsen_fraction * n_cells);
      for (size_t i = 0; i < n_cells && n_coarsen; ++i)
        if (!rf[order[i]]) cf[order[i]] = 1, --n_coarsen;
      std::vector<uint32_t> fresh((size_t)n_cells * 4 << dim), mid((size_t)n_cells * 4);
      uint32_t n_mid = 0;
      const int64_t n_new = mfgpu_mesh_adapt_leaves(dim, lv, n_cells, rf.data(), cf.data(), 0, fresh.data(), (uint64_t)n_cells << dim,
                                                    mid.data(), &n_mid);
      if (n_new < 0) check((int)n_new, "mfgpu_mesh_adapt_leaves");
      fresh.resize((size_t)n_new * 4);
      families = (n_cells - n_mid) / ((1u << dim) - 1);
      refined = ((uint32_t)n_new - n_mid) / ((1u << dim) - 1);
      // carry x over: interpolate on (mid, old), prolongate on (mid, new)
      mfgpu_mesh *m_mid = nullptr, *m_new = nullptr;
      mfgpu_transfer *down = nullptr, *up = nullptr;
      int rc = mfgpu_mesh_create_from_leaves(dim, degree, mid.data(), n_mid, MFGPU_F64, &m_mid);
      if (rc == 0) rc = mfgpu_mesh_create_from_leaves(dim, degree, fresh.data(), (uint32_t)n_new, MFGPU_F64, &m_new);
      if (rc == 0) rc = mfgpu_transfer_create_h_hn_interp_from_meshes(m_mid, L->mesh(), &down);
      if (rc == 0) rc = mfgpu_transfer_create_h_hn_from_meshes(m_mid, m_new, &up);
      if (rc == 0) {
        mfgpu_desc md, nw;
        rc = mfgpu_mesh_desc(m_mid, &md);
        if (rc == 0) rc = mfgpu_mesh_desc(m_new, &nw);
        if (rc == 0) {
          GpuVector<double> x_mid(md.n_dofs), start(nw.n_dofs);
          rc = mfgpu_transfer_interpolate(down, x_mid.getData(), x.getDataRO(), nullptr);
          if (rc == 0) rc = mfgpu_transfer_prolongate(up, start.getData(), x_mid.getDataRO(), nullptr);
          mfgpu_device_synchronize();
          x.swap(start);
        }
      }
      mfgpu_transfer_destroy(up);
      mfgpu_transfer_destroy(down);
      mfgpu_mesh_destroy(m_new);
      mfgpu_mesh_destroy(m_mid);
      check(rc, "solution transfer");
      leaves.swap(fresh);
    }
    std::printf("%d %.4f %u %u %u %u %u %.10e\n", step, t, n_cells, N, families, refined, info.iterations, l2);
  }
  return finest;
}

}  // namespace

int main(int argc, char **argv) {
  try {
    const int n_start_ref = argc > 1 ? atoi(argv[1]) : 3;
    const int n_steps = argc > 2 ? atoi(argv[2]) : 5;
    const double fr = argc > 3 ? atof(argv[3]) : 0.1, fc = argc > 4 ? atof(argv[4]) : 0.6;
    const double dt = argc > 5 ? atof(argv[5]) : 0.05;
    if (n_start_ref < 1 || n_start_ref > 12 || n_steps < 1 || !(fr >= 0.0 && fr <= 1.0) || !(fc >= 0.0 && fc <= 1.0) || !(dt > 0.0)) {
      std::cerr << "usage: heat-amr n_start_ref (1..12) n_steps (>= 1) [refine_fraction coarsen_fraction in [0, 1] [dt > 0]]"
                << std::endl;
      return 1;
    }
    const int finest = run<DIMENSION>(DEGREE_FE, uniform_leaves(DIMENSION, n_start_ref), n_steps, fr, fc, dt, true);
    if (DIMENSION * finest <= 16) {
      std::printf("# the uniform mesh of level %d, no adaptation\n", finest);
      run<DIMENSION>(DEGREE_FE, uniform_leaves(DIMENSION, finest), n_steps, fr, fc, dt, false);
    } else {
      std::printf("# the uniform mesh of level %d has more than 2^16 cells: not run\n", finest);
    }
    return 0;
  } catch (std::exception &exc) {
    std::cerr << "Exception on processing: " << exc.what() << std::endl;
    return 1;
  }
}
