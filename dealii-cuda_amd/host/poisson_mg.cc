// poisson_mg: conjugate gradients preconditioned by one geometric-multigrid V-cycle, assembled as the reference's
// poisson_mg.cu / bmop_mg.cu assemble it (:199-209 level matrices, :325-326 transfer, :334-335 coarse CG, :343-362
// Chebyshev smoothers of degree 5 with smoothing range 15, :369-380 Multigrid + PreconditionMG, CG to 1e-12).  deal.II's
// classes are the stand-ins of mfgpu_shim.h / mfgpu_shim_mg.h; everything on the device goes through the C-ABI.  The
// right-hand side is A x* for a known x*, so the driver checks its own answer.
// Output:  dim  degree  n_dofs  levels  cg_iterations  wall_seconds  rel_error
// usage: poisson-mg-<dim>d-p<k> n_ref          (-DBALL_GRID: the BALL domain; -DADAPTIVE_GRID: the pseudo-adaptive
// mesh with hanging nodes, local smoothing with refinement-edge matrices, poisson_mg.cu:365-375)
// -DMG_LEVEL_FLOAT: the whole multigrid hierarchy in float under the double CG (the reference's commented
// `typedef float level_number;`, bmop_mg.cu:58-59); -DMG_FUSED_SMOOTHER: the Chebyshev smoothers with fused vector
// updates.  With either, two more columns:  mg_bytes (level operators, inverse diagonals, transfers, level vectors)
// vcycle_ms (mean of 10 preconditioner applications after the solve, each between two device synchronisations)
// -DPOISSON_DEVICE_MG (-devmg): the V-cycle is the library's mfgpu_vcycle (MultigridPreconditionerDevice: same smoothers'
// lambda_max, the coarse level solved on the device) under the device CG, so the whole solve stops the host only in
// mfgpu_cg_status; same arguments and output lines as the counterpart without the suffix
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <iostream>
#include <limits>
#include <type_traits>

#ifdef POISSON_DEVICE_MG
#define POISSON_DEVICE_CG 1
#endif
#ifdef POISSON_DEVICE_CG
#include "mfgpu_shim_poisson.h"  // SolverCGDevice: the outer CG on the device, the V-cycle through its callback (-devcg)
#else
#include "mfgpu_shim_mg.h"
#endif

using namespace mfgpu_shim;

#ifndef DEGREE_FE
#define DEGREE_FE 4
#endif
#ifndef DIMENSION
#define DIMENSION 3
#endif
typedef double number;
#ifdef MG_LEVEL_FLOAT
typedef float level_number;
#else
typedef double level_number;
#endif
#if defined(MG_LEVEL_FLOAT) || defined(MG_FUSED_SMOOTHER)
#define MG_REPORT 1
#endif
typedef GpuVector<number> VectorType;

// coarse solver (poisson_mg.cu:61-83): unpreconditioned CG to a relative max(1e-10, 100 eps) -- 1e-10 in double, what
// float can reach in float -- or as many iterations as the coarse level has dofs
template <typename MatrixType>
class MGCoarseIterative {
public:
  typedef typename MatrixType::value_type Number;
  typedef GpuVector<Number> LevelVectorType;
  void initialize(const MatrixType &matrix) {
    coarse_matrix = &matrix;
    const unsigned int N = matrix.m();
    r.reinit(N);
    p.reinit(N);
    q.reinit(N);
  }
  void operator()(const unsigned int, LevelVectorType &dst, const LevelVectorType &src) const {
    dst = Number(0);
    r.equ(1, src);
    p.equ(1, r);
    Number rr = r * r;
    const Number tol = std::max(1e-10, 100. * std::numeric_limits<Number>::epsilon()) * std::sqrt(rr);
    for (unsigned int it = 0; it < coarse_matrix->m() && std::sqrt(rr) > tol; ++it) {
      coarse_matrix->vmult(q, p);
      const Number alpha = rr / (p * q);
      dst.add(alpha, p);
      r.add(-alpha, q);
      const Number rr_new = r * r;
      p.sadd(rr_new / rr, 1, r);
      rr = rr_new;
    }
  }
  std::size_t memory_consumption() const {
    return r.memory_consumption() + p.memory_consumption() + q.memory_consumption();
  }
  const MatrixType *coarse_matrix = nullptr;
  mutable LevelVectorType r, p, q;
};

// the system matrix of a globally refined mesh is the finest level's when both are of one number type
template <typename S, typename L>
const S *finest_level_as_system(const L &finest) {
  if constexpr (std::is_same<S, L>::value)
    return &finest;
  else
    return nullptr;
}

template <int dim, int fe_degree>
int run(int n_ref) {
  typedef LevelOperatorGpu<dim, fe_degree, level_number> LevelMatrixType;
  typedef LevelOperatorGpu<dim, fe_degree, number> SystemMatrixType;
  Triangulation<dim> triangulation;
#if defined(BALL_GRID)
  bmop_setup_mesh(triangulation, BALL, false, n_ref);
#elif defined(ADAPTIVE_GRID)
  bmop_setup_mesh(triangulation, CUBE, true, n_ref);
#else
  bmop_setup_mesh(triangulation, CUBE, false, n_ref);
#endif
  FE_Q<dim> fe(fe_degree);
  MGDoFHandler<dim> dof_handler(triangulation);
  dof_handler.distribute_mg_dofs(fe, number_type<level_number>(), number_type<number>());
  const unsigned int nlevels = dof_handler.n_levels();

  MGConstrainedDoFs mg_constrained_dofs;
  MGLevelObject<LevelMatrixType> mg_matrices;
  mg_matrices.resize(0, nlevels - 1);
  for (unsigned int level = 0; level < nlevels; ++level) {
    mg_matrices[level].reinit(dof_handler, mg_constrained_dofs, level);
    mg_matrices[level].compute_diagonal();
  }
  // the system matrix: on a globally refined mesh the finest level's (the active mesh's operator in its own type when
  // the levels are float); on the adaptive mesh the active cells' operator with hanging nodes
  SystemMatrixType active_matrix;
  const SystemMatrixType *finest = finest_level_as_system<SystemMatrixType>(mg_matrices[nlevels - 1]);
  if (dof_handler.is_adaptive() || !finest) active_matrix.reinit_active(dof_handler);
  const SystemMatrixType &system_matrix = dof_handler.is_adaptive() || !finest ? active_matrix : *finest;
  const unsigned int N = system_matrix.n();

  MGTransferMatrixFreeGpu<dim, level_number> mg_transfer(mg_constrained_dofs);
  mg_transfer.build(dof_handler);
  MGCoarseIterative<LevelMatrixType> mg_coarse;
  mg_coarse.initialize(mg_matrices[0]);
  typedef PreconditionChebyshev<LevelMatrixType, GpuVector<level_number>> SMOOTHER;
  MGLevelObject<SMOOTHER> mg_smoother;
  mg_smoother.resize(0, nlevels - 1);
  for (unsigned int level = 0; level < nlevels; ++level) {
    typename SMOOTHER::AdditionalData sd;
    sd.smoothing_range = 15.;
    sd.degree = 5;
    sd.eig_cg_n_iterations = 15;
    sd.preconditioner = mg_matrices[level].get_diagonal_inverse();
#ifdef MG_FUSED_SMOOTHER
    sd.fused_updates = true;
#endif
    mg_smoother[level].initialize(mg_matrices[level], sd);
  }
#ifdef POISSON_DEVICE_MG
  MultigridPreconditionerDevice<dim, LevelMatrixType, level_number, MGCoarseIterative<LevelMatrixType>, number> preconditioner(
      dof_handler, mg_matrices, mg_coarse, mg_transfer, mg_smoother);
#else
  MultigridPreconditioner<dim, LevelMatrixType, level_number, MGCoarseIterative<LevelMatrixType>> preconditioner(
      dof_handler, mg_matrices, mg_coarse, mg_transfer, mg_smoother);
#endif

  // x*: zero on the Dirichlet dofs; b = A x*
  std::vector<number> xs(N);
  for (unsigned int i = 0; i < N; ++i) xs[i] = std::sin(0.37 * i) + 0.5 * std::cos(0.011 * i);
  VectorType x_star(xs), b(N), x(N), z(N);
  system_matrix.set_constrained_values(x_star, 0);
  system_matrix.vmult(b, x_star);

  mfgpu_device_synchronize();
  const auto t0 = std::chrono::steady_clock::now();
#ifdef POISSON_DEVICE_CG
  unsigned int it = 0;
  {
    SolverControl solver_control(1000, 1e-12 * b.l2_norm());
    SolverCGDevice<VectorType> cg(solver_control);
    try {
      cg.solve(system_matrix, x, b, preconditioner);
      it = solver_control.last_step();
    } catch (std::runtime_error &) {
      if (solver_control.last_step() < 1000) throw;
      it = 1001;  // no convergence: what the host loop below leaves in `it`
    }
  }
#else
  VectorType r(N), p(N), q(N);
  x = number(0);
  r.equ(1, b);
  preconditioner.vmult(z, r);
  p.equ(1, z);
  number rz = r * z;
  const number tol = 1e-12 * b.l2_norm();
  unsigned int it = 0;
  for (it = 1; it <= 1000; ++it) {
    system_matrix.vmult(q, p);
    const number alpha = rz / (p * q);
    x.add(alpha, p);
    r.add(-alpha, q);
    if (r.l2_norm() <= tol) break;
    preconditioner.vmult(z, r);
    const number rz_new = r * z;
    p.sadd(rz_new / rz, 1, z);
    rz = rz_new;
  }
#endif
  mfgpu_device_synchronize();
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  x.add(-1, x_star);
  const double err = x.l2_norm() / x_star.l2_norm();
#ifdef MG_REPORT
  std::size_t mg_bytes = mg_transfer.memory_consumption() + preconditioner.memory_consumption() + mg_coarse.memory_consumption();
  for (unsigned int level = 0; level < nlevels; ++level)
    mg_bytes += mg_matrices[level].memory_consumption() + mg_matrices[level].get_diagonal_inverse()->get_vector().memory_consumption() +
                mg_smoother[level].memory_consumption();
  double vcycle_ms = 0;
  for (int k = 0; k < 10; ++k) {
    mfgpu_device_synchronize();
    const auto v0 = std::chrono::steady_clock::now();
    preconditioner.vmult(z, b);
    mfgpu_device_synchronize();
    vcycle_ms += 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - v0).count() / 10;
  }
  printf("%8d %8d %12u %8u %8u %14.8g %12.4g %12zu %10.4f\n", dim, fe_degree, N, nlevels, it, wall, err, mg_bytes, vcycle_ms);
#else
  printf("%8d %8d %12u %8u %8u %14.8g %12.4g\n", dim, fe_degree, N, nlevels, it, wall, err);
#endif
  return (it <= 1000 && err < 1e-8) ? 0 : 2;
}

int main(int argc, char **argv) {
  try {
    const int n_ref = argc > 1 ? atoi(argv[1]) : 3;
    return run<DIMENSION, DEGREE_FE>(n_ref);
  } catch (std::exception &exc) {
    std::cerr << "Exception on processing: " << exc.what() << std::endl;
    return 1;
  }
}
