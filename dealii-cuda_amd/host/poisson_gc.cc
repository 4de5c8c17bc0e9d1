// poisson_gc: the problem of poisson_mg.cc -- CG to 1e-12 |b| on the variable-coefficient Laplacian, b = A x* for a known
// x* -- on the adaptively refined cube of bmop / poisson, preconditioned by one V-cycle of GLOBAL-COARSENING multigrid
// (DESIGN.md section 20): the levels are complete meshes with hanging nodes, made from the active mesh alone by
// mfgpu_mesh_coarsen_leaves until a step would leave fewer than 2^dim cells, and joined by
// mfgpu_transfer_create_h_hn_from_meshes.  No level hierarchy, no refinement edges, no copy pairs: what a caller with
// deal.II's MGTransferGlobalCoarsening has.  With the optional second argument `p` the coarsened meshes are at degree 1
// and the active mesh follows at the degrees that halve down from DEGREE_FE, 1 -> 2 -> 4, joined by
// mfgpu_transfer_create_p_hn_from_meshes (section 19).  The V-cycle is the library's mfgpu_vcycle (Chebyshev(5, range 15)
// smoothers with estimated lambda_max, level 0 solved on the device) under the device CG.  Written on the C-ABI alone.
// Output:  dim  degree  n_dofs  levels  cg_iterations  wall_seconds  rel_error
// usage: poisson-gc-<dim>d-p<k>-adaptive n_ref [p]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// the level meshes, operators and transfers; everything is released in reverse order
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

int run(int dim, int fe_degree, int n_ref, bool p_levels) {
  Hierarchy H;
  const int h_degree = p_levels ? 1 : fe_degree;  // the degree of the coarsened meshes
  // fine to coarse first: the active mesh at h_degree, then its coarsenings
  mfgpu_mesh *m = nullptr;
  check(mfgpu_mesh_create_adaptive(dim, h_degree, n_ref, MFGPU_F64, &m), "active mesh");
  H.meshes.push_back(m);
  for (;;) {
    const uint32_t *lv = nullptr;
    const int64_t n_fine = mfgpu_mesh_cell_levels(H.meshes.back(), &lv) / 4;
    if (n_fine <= 1) break;
    std::vector<uint32_t> coarse((size_t)n_fine * 4);
    const int64_t n_coarse = mfgpu_mesh_coarsen_leaves(dim, lv, (uint32_t)n_fine, coarse.data());
    if (n_coarse < 0) check((int)n_coarse, "mfgpu_mesh_coarsen_leaves");
    if (n_coarse < (1 << dim)) break;  // (one cell at degree 1 has no free dof)
    check(mfgpu_mesh_create_from_leaves(dim, h_degree, coarse.data(), (uint32_t)n_coarse, MFGPU_F64, &m), "coarsened mesh");
    H.meshes.push_back(m);
  }
  std::reverse(H.meshes.begin(), H.meshes.end());
  std::vector<bool> p_step(H.meshes.size(), false);  // how level l is reached from level l - 1
  if (p_levels) {
    std::vector<int> degrees;  // above 1, descending: fe_degree, fe_degree / 2, ...
    for (int p = fe_degree; p > 1; p /= 2) degrees.push_back(p);
    for (auto it = degrees.rbegin(); it != degrees.rend(); ++it) {
      check(mfgpu_mesh_create_adaptive(dim, *it, n_ref, MFGPU_F64, &m), "active mesh");
      H.meshes.push_back(m);
      p_step.push_back(true);
    }
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
                      : mfgpu_transfer_create_h_hn_from_meshes(H.meshes[l - 1], H.meshes[l], &H.transfers[l]),
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
    const bool p_levels = argc > 2 && std::strcmp(argv[2], "p") == 0;
    return run(DIMENSION, DEGREE_FE, n_ref, p_levels);
  } catch (std::exception &exc) {
    std::cerr << "Exception on processing: " << exc.what() << std::endl;
    return 1;
  }
}
