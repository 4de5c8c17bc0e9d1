// helmholtz: poisson.cc with a mass term -- the reaction-diffusion problem  -div(a grad u) + c u = f  with
// c(x) = 1 + |x|^2, the coefficient a of the Poisson problem and the same analytic solution Solution<dim>
// (poisson_common.cc:5-175), solved and measured against it.
//   mesh      as poisson.cc (create_mesh, poisson_common.h:89-103; -DBALL_GRID, -DADAPTIVE_GRID)
//   operator  HelmholtzOperatorGpu: mfgpu_desc.mass_coefficient = c at the quadrature points
//   assembly  u_b = Solution on the constrained dofs, f = RightHandSide + c Solution evaluated on the host at the
//             quadrature points, rhs = int phi f - int grad phi . a grad u_b - int c phi u_b on the device
//             (mfgpu_integrator created from the description with the same mass_coefficient)
//   solve     CG to 1e-12 |rhs|, preconditioned by PreconditionChebyshev on the inverse diagonal (of K + M)
//   error     u = u_b + x, L2 error on QGauss(p+2)
// usage: helmholtz-<dim>d-p<k> [-q] [min_cycle] [max_cycle]     (default max_cycle 6 - dim)
// -q prints one line per cycle:  dim  degree  n_dofs  iterations  wall_seconds  l2_error
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <iostream>

#include "mfgpu_shim_helmholtz.h"

using namespace mfgpu_shim;

#ifndef DEGREE_FE
#define DEGREE_FE 4
#endif
#ifndef DIMENSION
#define DIMENSION 3
#endif
typedef double number;

static bool QUIET = false;

template <int dim>
static double mass_function(const double *x) {
  double xx = 0;
  for (int d = 0; d < dim; ++d) xx += x[d] * x[d];
  return 1.0 + xx;
}

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

  // setup_system + assemble_system
  HelmholtzOperatorGpu<dim, fe_degree, number> system_matrix;
  system_matrix.reinit(dof_handler, constraints, mass_function<dim>);
  const unsigned int N = system_matrix.n();
  std::vector<number> ub_host(N, 0.0);
  VectorTools::interpolate_boundary_values(dof_handler, Solution<dim>(), ub_host);
  VectorType solution(ub_host), solution_update(N), system_rhs(N);
  // the load at the quadrature points, on the host
  const std::vector<number> &c_qp = system_matrix.mass_coefficient();
  std::vector<number> f_host(c_qp.size());
  const number *xq = static_cast<const number *>(dof_handler.desc.quadrature_points);
  const Solution<dim> exact;
  const RightHandSide<dim> poisson_load;
  for (size_t q = 0; q < f_host.size(); ++q) f_host[q] = poisson_load.value(xq + q * dim) + c_qp[q] * exact.value(xq + q * dim);
  VectorType f_qp(f_host);
  // the integrator's description carries the mass term too: its lift subtracts int c phi u_b
  PoissonIntegrator<dim> integrator(dof_handler, c_qp.data());
  VectorTools::create_right_hand_side(integrator, system_rhs, f_qp, &solution);
  system_matrix.compute_diagonal();

  // solve
  typedef PreconditionChebyshev<HelmholtzOperatorGpu<dim, fe_degree, number>, VectorType> PreconditionType;
  PreconditionType preconditioner;
  typename PreconditionType::AdditionalData additional_data;
  additional_data.preconditioner = system_matrix.get_diagonal_inverse();
  preconditioner.initialize(system_matrix, additional_data);
  SolverControl solver_control(10000, 1e-12 * system_rhs.l2_norm());
  SolverCG<VectorType> cg(solver_control);
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
