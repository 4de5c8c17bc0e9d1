// poisson_pmg: the problem of poisson_mg.cc -- CG to 1e-12 |b| on the variable-coefficient Laplacian, b = A x* for a known
// x* -- preconditioned by one V-cycle over a HYBRID hierarchy: h-levels at degree 1 up to the mesh
// of n_ref, then on that mesh the degrees that halve down from DEGREE_FE (rounding down) until 1, e.g. 1 -> 2 -> 4.  The
// p-steps are mfgpu_transfer_create_p_hn_from_meshes (on conforming meshes mfgpu_transfer_create_p_from_meshes), the h-steps mfgpu_transfer_create_from_meshes; the V-cycle is the
// library's mfgpu_vcycle (Chebyshev(5, range 15) smoothers with estimated lambda_max, level 0 solved on the device) under
// the device CG, so the solve stops the host only in mfgpu_cg_status.  Written on the C-ABI: the shim's classes are
// templated on one degree.
// CUBE: the h-levels run from 2 cells per direction (one cell at degree 1 has no free dof); BALL (-DBALL_GRID): from
// n_ref 0.
// ADAPTIVE (-DADAPTIVE_GRID): the adaptively refined cube of bmop / poisson with its hanging nodes,
// an active mesh without a level hierarchy.  No h-levels: the levels are that ONE mesh at the halving degrees, 1 -> 2 -> 4,
// joined by mfgpu_transfer_create_p_hn_from_meshes.  Level 0 is the whole mesh at degree 1, so above
// MFGPU_VCYCLE_DENSE_MAX dofs its solve is the unpreconditioned device CG, capped by the second argument.
// Output:  dim  degree  n_dofs  levels  cg_iterations  wall_seconds  rel_error
// usage: poisson-pmg-<dim>d-p<k>[-ball] n_ref          poisson-pmg-<dim>d-p<k>-adaptive n_ref [coarse_max_iterations]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <iostream>
#include <vector>

#include "mfgpu_shim.h"

using namespace mfgpu_shim;

#ifndef DEGREE_FE
#define DEGREE_FE 4
#endif
#ifndef DIMENSION
#define DIMENSION 3
#endif

namespace {

mfgpu_mesh *create_mesh(int dim, int degree, int n_ref) {
  mfgpu_mesh *m = nullptr;
#if defined(ADAPTIVE_GRID)
  check(mfgpu_mesh_create_adaptive(dim, degree, n_ref, MFGPU_F64, &m), "level mesh");
#elif defined(BALL_GRID)
  check(mfgpu_mesh_create_ball(dim, degree, n_ref, MFGPU_F64, &m), "level mesh");
#else
  const uint32_t nper[3] = {1u << n_ref, 1u << n_ref, 1u << n_ref};
  check(mfgpu_mesh_create_uniform(dim, degree, nper, -1.0, 1.0, 0, 0, MFGPU_F64, &m), "level mesh");
#endif
  return m;
}

// the level meshes, operators and transfers of the hybrid hierarchy; everything is released in reverse order
struct Hierarchy {
  std::vector<mfgpu_mesh *> meshes;
  std::vector<mfgpu_handle *> ops;
  std::vector<mfgpu_transfer *> transfers;  // transfers[l]: level l - 1 -> l (nullptr on level 0)
  mfgpu_vcycle *vcycle = nullptr;
  mfgpu_cg *cg = nullptr;
  ~Hierarchy() {
    mfgpu_cg_destroy(cg);
    mfgpu_vcycle_destroy(vcycle);
    for (mfgpu_transfer *t : transfers) mfgpu_transfer_destroy(t);
    for (mfgpu_handle *h : ops) mfgpu_destroy(h);
    for (mfgpu_mesh *m : meshes) mfgpu_mesh_destroy(m);
  }
};

int run(int dim, int fe_degree, int n_ref, unsigned int coarse_max_iterations) {
#if defined(ADAPTIVE_GRID)
  const int first_ref = n_ref;  // the one mesh at degree 1
#elif defined(BALL_GRID)
  const int first_ref = 0;
#else
  const int first_ref = 1;
#endif
  if (n_ref < first_ref) throw std::runtime_error("n_ref is below the coarsest level of the hybrid hierarchy");
  Hierarchy H;
  std::vector<bool> p_step;  // how level l is reached from level l - 1
  for (int r = first_ref; r <= n_ref; ++r) {
    H.meshes.push_back(create_mesh(dim, 1, r));
    p_step.push_back(false);
  }
  std::vector<int> degrees;  // above 1, descending: fe_degree, fe_degree / 2, ...
  for (int p = fe_degree; p > 1; p /= 2) degrees.push_back(p);
  for (auto it = degrees.rbegin(); it != degrees.rend(); ++it) {
    H.meshes.push_back(create_mesh(dim, *it, n_ref));
    p_step.push_back(true);
  }
  const unsigned int nlevels = (unsigned int)H.meshes.size();
  std::vector<mfgpu_vcycle_level_desc> levels(nlevels);
  H.transfers.assign(nlevels, nullptr);
  for (unsigned int l = 0; l < nlevels; ++l) {
    mfgpu_desc d;
    check(mfgpu_mesh_desc(H.meshes[l], &d), "mesh desc");
    mfgpu_handle *op = nullptr;
    check(mfgpu_create(&d, &op), "level operator");
    H.ops.push_back(op);
    if (l > 0)
      check(p_step[l] ? mfgpu_transfer_create_p_hn_from_meshes(H.meshes[l - 1], H.meshes[l], &H.transfers[l])
                      : mfgpu_transfer_create_from_meshes(H.meshes[l - 1], H.meshes[l], &H.transfers[l]),
            "level transfer");
    levels[l] = mfgpu_vcycle_level_desc{};
    levels[l].op = op;
    levels[l].from_coarser = H.transfers[l];
  }
  mfgpu_handle *system_matrix = H.ops.back();
  const unsigned int N = mfgpu_n_dofs(system_matrix);

  mfgpu_vcycle_desc vd{};
  vd.n_levels = nlevels;
  vd.levels = levels.data();
  vd.active_type = MFGPU_F64;
  vd.n_active = N;
  vd.smoother_degree = 5;
  vd.smoothing_range = 15.;
  vd.eig_iterations = 15;
  vd.lambda_max = nullptr;  // estimated, as PreconditionChebyshev does in poisson_mg.cc
  vd.coarse = MFGPU_VCYCLE_COARSE_AUTO;
  vd.coarse_max_iterations = coarse_max_iterations;  // (0: n_dofs(0); read by the CG mode only)
  check(mfgpu_vcycle_create(&vd, &H.vcycle), "mfgpu_vcycle_create");
  check(mfgpu_cg_create(system_matrix, MFGPU_CG_CALLBACK, nullptr, 0, 0, 0, &H.cg), "mfgpu_cg_create");
  check(mfgpu_cg_set_vcycle(H.cg, H.vcycle), "mfgpu_cg_set_vcycle");

  // x*: zero on the Dirichlet dofs; b = A x*
  std::vector<double> xs(N);
  for (unsigned int i = 0; i < N; ++i) xs[i] = std::sin(0.37 * i) + 0.5 * std::cos(0.011 * i);
  GpuVector<double> x_star(xs), b(N), x(N);
  check(mfgpu_set_constrained_values(system_matrix, x_star.getData(), 0.0, nullptr), "set_constrained_values");
  check(mfgpu_vmult(system_matrix, b.getData(), x_star.getDataRO(), nullptr), "vmult");

  mfgpu_device_synchronize();
  const auto t0 = std::chrono::steady_clock::now();
  mfgpu_cg_info info{};
  check(mfgpu_cg_solve(H.cg, x.getData(), b.getDataRO(), 1e-12 * b.l2_norm(), 1000, 10, nullptr, &info), "mfgpu_cg_solve");
  mfgpu_device_synchronize();
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  const unsigned int it = info.status == 1 ? info.iterations : 1001;
  x.add(-1, x_star);
  const double err = x.l2_norm() / x_star.l2_norm();
  printf("%8d %8d %12u %8u %8u %14.8g %12.4g\n", dim, fe_degree, N, nlevels, it, wall, err);
  return (it <= 1000 && err < 1e-8) ? 0 : 2;
}

}  // namespace

int main(int argc, char **argv) {
  try {
    const int n_ref = argc > 1 ? atoi(argv[1]) : 3;
    const int coarse_cap = argc > 2 ? atoi(argv[2]) : 0;
    return run(DIMENSION, DEGREE_FE, n_ref, coarse_cap > 0 ? (unsigned int)coarse_cap : 0u);
  } catch (std::exception &exc) {
    std::cerr << "Exception on processing: " << exc.what() << std::endl;
    return 1;
  }
}
