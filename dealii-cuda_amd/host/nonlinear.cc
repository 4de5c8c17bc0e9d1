// nonlinear: a quasilinear problem on the C-ABI -- -div((1 + u^2) grad u) = f on hyper_cube(-1,1) with the analytic
// solution Solution<dim> (poisson_common.cc:5-175), solved by a Picard iteration whose coefficient never leaves the
// device.  The reference has no such program: its coefficient is fixed at reinit (laplace_operator_gpu.h:191-211).
//   mesh      as poisson: refine_global(1 + (3 - dim)), then one uniform refinement per cycle
//   load      f = -(1 + u*^2) lap u* - 2 u* |grad u*|^2 at the quadrature points, computed once on the host
//   Picard    u_0 = u* on the boundary, 0 inside.  Step k: u_k at the quadrature points (mfgpu_integrator_evaluate),
//             a = 1 + u_k^2 by vector operations on that array, new coefficient for the operator and for the lift
//             (mfgpu_update_coefficients, mfgpu_integrator_update_coefficients), inverse diagonal, right-hand side with
//             the lift, Chebyshev-preconditioned CG to 1e-12 |rhs| as in poisson, u_{k+1} = u_b + x.
//             Stops at |u_{k+1} - u_k| / |u_{k+1}| <= 1e-10.  Only norms and dot products return to the host.
//   error     L2 error of the last iterate on QGauss(p+2)
// usage: nonlinear-<dim>d-p<k> [-q] [min_cycle] [max_cycle]     (default max_cycle 6 - dim)
// -q prints one line per cycle:
//   dim  degree  n_dofs  picard_steps  inner_iterations  wall_seconds  l2_error
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <iostream>

#include "mfgpu_shim_nonlinear.h"

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
  bmop_setup_mesh(triangulation, CUBE, false, 1 + (3 - dim) + 1 + (int)cycle);
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

  // setup: operator and integrator keep what a coefficient update needs; the load on the host, once
  UpdatableOperatorGpu<dim, fe_degree, number> system_matrix;
  system_matrix.reinit(dof_handler, constraints);
  const unsigned int N = system_matrix.n();
  const size_t nq = system_matrix.n_quadrature_points();
  std::vector<number> ub_host(N, 0.0);
  VectorTools::interpolate_boundary_values(dof_handler, Solution<dim>(), ub_host);
  VectorType solution(ub_host), lift(ub_host), previous(N), solution_update(N), system_rhs(N);
  std::vector<number> f_host(nq);
  const number *xq = static_cast<const number *>(dof_handler.desc.quadrature_points);
  const Solution<dim> exact;
  for (size_t q = 0; q < nq; ++q) {
    double g[dim], gg = 0;
    const double u = exact.value(xq + q * dim);
    exact.gradient(xq + q * dim, g);
    for (int d = 0; d < dim; ++d) gg += g[d] * g[d];
    f_host[q] = -(1.0 + u * u) * exact.laplacian(xq + q * dim) - 2.0 * u * gg;
  }
  VectorType f_qp(f_host), u_qp((unsigned int)nq), a_qp((unsigned int)nq), ones_qp((unsigned int)nq);
  ones_qp = 1.0;
  mfgpu_desc integrator_desc = dof_handler.desc;
  const std::vector<number> ones_host(nq, 1.0);
  integrator_desc.coefficient = ones_host.data();  // a = 1 until the first update, as the operator
  integrator_desc.flags |= MFGPU_UPDATABLE_COEFFICIENTS;
  PoissonIntegrator<dim> integrator(integrator_desc);

  typedef PreconditionChebyshev<UpdatableOperatorGpu<dim, fe_degree, number>, VectorType> PreconditionType;
  PreconditionType preconditioner;
  unsigned int picard = 0, inner = 0;
  mfgpu_device_synchronize();
  const auto t0 = std::chrono::steady_clock::now();
  for (; picard < 100;) {
    // a = 1 + u^2 at the quadrature points
    VectorTools::point_values(integrator, solution, u_qp);
    a_qp.equ(1, u_qp);
    a_qp.scale(u_qp);
    a_qp.sadd(1, 1, ones_qp);
    system_matrix.update_coefficients(a_qp);
    update_coefficients(integrator, a_qp);
    system_matrix.compute_diagonal();
    VectorTools::create_right_hand_side(integrator, system_rhs, f_qp, &lift);
    typename PreconditionType::AdditionalData additional_data;
    additional_data.preconditioner = system_matrix.get_diagonal_inverse();
    preconditioner.initialize(system_matrix, additional_data);
    SolverControl solver_control(10000, 1e-12 * system_rhs.l2_norm());
    SolverCG<VectorType> cg(solver_control);
    cg.solve(system_matrix, solution_update, system_rhs, preconditioner);
    inner += solver_control.last_step();
    ++picard;
    // u_{k+1} = u_b + x (the update is zero on every constrained dof)
    previous.equ(1, solution);
    solution.equ(1, lift);
    solution += solution_update;
    previous -= solution;
    const double change = previous.l2_norm() / solution.l2_norm();
    if (!QUIET) std::cout << "   Picard step " << picard << ": " << solver_control.last_step() << " CG iterations, relative update " << change << std::endl;
    if (change <= 1e-10) break;
  }
  mfgpu_device_synchronize();
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

  const double l2 = VectorTools::integrate_difference(integrator, solution);
  if (!QUIET) {
    std::cout << "Time solve (" << picard << " Picard steps, " << inner << " iterations)  (wall) " << wall << "s\n";
    std::cout.precision(6);
    std::cout << "L2 error: " << l2 * l2 << std::endl;
  } else {
    printf("%8d %8d %12u %8u %8u %14.8g %14.8g\n", dim, fe_degree, N, picard, inner, wall, l2);
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
