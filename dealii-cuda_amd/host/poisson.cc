// poisson: the reference's poisson.cu on the C-ABI -- a variable-coefficient Poisson problem with the analytic solution
// Solution<dim> (poisson_common.cc:5-175), solved and measured against it.
//   mesh      create_mesh (poisson_common.h:89-103): hyper_cube(-1,1), refine_global(1 + (3 - dim)), then one uniform
//             refinement per cycle.  -DBALL_GRID: hyper_ball, refine_global(3 - dim), one refinement per cycle.
//             -DADAPTIVE_GRID: the pseudo-adaptive stand-in mesh with hanging nodes, n_ref = 6 - dim + cycle (its first
//             hanging nodes appear at n_ref = 3 in 2D, 4 in 3D).
//   assembly  u_b = Solution on the constrained dofs (poisson.cu:157-160), rhs = int phi f - int grad phi . a grad u_b
//             (poisson.cu:182-221), both integrals on the device (mfgpu_integrator)
//   solve     CG to 1e-12 |rhs| (poisson.cu:246-254), preconditioned by PreconditionChebyshev on the inverse diagonal.
//             The reference leaves the Chebyshev parameters at deal.II's defaults; the shim's PreconditionChebyshev is
//             the one poisson_mg configures (degree 5, smoothing range 15, power-iteration eigenvalue estimate).  The
//             preconditioner changes the iteration count, not the solution: any fixed SPD polynomial in D^-1 A gives
//             the same CG limit, so the L2 error column is comparable, the iteration column is not.
//   error     u = u_b + x, L2 error on QGauss(p+2) (poisson.cu:277-292)
//             -DPOISSON_DEVICE_CG (the -devcg binaries): the same CG with its loop on the device, SolverCGDevice
// usage: poisson-<dim>d-p<k> [-q] [min_cycle] [max_cycle]     (default max_cycle 6 - dim)
// -q prints one line per cycle (poisson.cu:271-272) with the L2 error appended:
//   dim  degree  n_dofs  iterations  wall_seconds  l2_error
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <iostream>

#include "mfgpu_shim_poisson.h"

using namespace mfgpu_shim;

#ifndef DEGREE_FE
#define DEGREE_FE 4
#endif
#ifndef DIMENSION
#define DIMENSION 3
#endif
typedef double number;

static bool QUIET = false;

template <int dim, int fe_degree>
void run_cycle(unsigned int cycle) {
  typedef GpuVector<number> VectorType;
  Triangulation<dim> triangulation;
#if defined(BALL_GRID)
  bmop_setup_mesh(triangulation, BALL, false, (3 - dim) + 1 + (int)cycle);
#elif defined(ADAPTIVE_GRID)
  bmop_setup_mesh(triangulation, CUBE, true, 6 - dim + (int)cycle);
#else
  bmop_setup_mesh(triangulation, CUBE, false, 1 + (3 - dim) + 1 + (int)cycle);
#endif
  FE_Q<dim> fe(fe_degree);
  DoFHandler<dim> dof_handler(triangulation);
  ConstraintMatrix constraints;
  dof_handler.distribute_dofs(fe, number_type<number>());
  constraints.close();
  if (!QUIET) {
    std::cout << "Cycle " << cycle << std::endl;
    std::cout << "   Number of active cells:       " << dof_handler.desc.n_cells << std::endl;
    std::cout << "   Number of degrees of freedom: " << dof_handler.n_dofs() << std::endl;
  }

  // setup_system + assemble_system (poisson.cu:115-229)
  LaplaceOperatorGpu<dim, fe_degree, number> system_matrix;
  system_matrix.reinit(dof_handler, constraints);
  const unsigned int N = system_matrix.n();
  std::vector<number> ub_host(N, 0.0);
  VectorTools::interpolate_boundary_values(dof_handler, Solution<dim>(), ub_host);
  VectorType solution(ub_host), solution_update(N), system_rhs(N);
  PoissonIntegrator<dim> integrator(dof_handler);
  VectorTools::create_right_hand_side(integrator, system_rhs, &solution);
  system_matrix.compute_diagonal();

  // solve (poisson.cu:232-260)
  typedef PreconditionChebyshev<LaplaceOperatorGpu<dim, fe_degree, number>, VectorType> PreconditionType;
  PreconditionType preconditioner;
  typename PreconditionType::AdditionalData additional_data;
  additional_data.preconditioner = system_matrix.get_diagonal_inverse();
  preconditioner.initialize(system_matrix, additional_data);
  SolverControl solver_control(10000, 1e-12 * system_rhs.l2_norm());
#ifdef POISSON_DEVICE_CG
  SolverCGDevice<VectorType> cg(solver_control);  // the CG loop on the device (mfgpu_cg): the -devcg binaries
#else
  SolverCG<VectorType> cg(solver_control);
#endif
  mfgpu_device_synchronize();
  const auto t0 = std::chrono::steady_clock::now();
  cg.solve(system_matrix, solution_update, system_rhs, preconditioner);
  mfgpu_device_synchronize();
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

  // u = u_b + x (the update is zero on every constrained dof), L2 error against Solution
  solution += solution_update;
  const double l2 = VectorTools::integrate_difference(integrator, solution);
  if (!QUIET) {
    std::cout << "Time solve (" << solver_control.last_step() << " iterations)  (wall) " << wall << "s\n";
    // the reference prints difference_per_cell.norm_sqr() (poisson.cu:285-289): the SQUARE of the L2 norm
    std::cout.precision(6);
    std::cout << "L2 error: " << l2 * l2 << std::endl;
  } else {
    printf("%8d %8d %12u %8u %14.8g %14.8g\n", dim, fe_degree, N, solver_control.last_step(), wall, l2);
  }
}

int main(int argc, char **argv) {
  try {
    int a = 1;
    if (argc > 1 && std::strcmp(argv[1], "-q") == 0) {
      QUIET = true;
      ++a;
    }
    const unsigned int min_cycle = argc > a ? (unsigned int)atoi(argv[a]) : 0;
    const unsigned int max_cycle = argc > a + 1 ? (unsigned int)atoi(argv[a + 1]) : 6 - DIMENSION;
    for (unsigned int cycle = min_cycle; cycle <= max_cycle; ++cycle) run_cycle<DIMENSION, DEGREE_FE>(cycle);
    return 0;
  } catch (std::exception &exc) {
    std::cerr << "Exception on processing: " << exc.what() << std::endl;
    return 1;
  }
}
