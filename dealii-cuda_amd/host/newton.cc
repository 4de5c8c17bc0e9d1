// newton: nonlinear.cc's problem -- -div((1 + u^2) grad u) = f on hyper_cube(-1,1) with the analytic solution
// Solution<dim> (poisson_common.cc:5-175) -- by Newton's method on the user-operator surface of the C-ABI.  The
// reference has no such program.
//   mesh, load, start, stopping rule     as nonlinear: u_0 = u* on the boundary, 0 inside; stops at
//             |u_{k+1} - u_k| / |u_{k+1}| <= 1e-10
//   residual  R(u)_i = int grad phi_i . (1 + u^2) grad u - phi_i f: u and grad u at the quadrature points
//             (mfgpu_integrator_evaluate), the flux by vector operations, mfgpu_integrator_integrate(-f, flux)
//   Jacobian  J(u) w = int grad phi_i . ((1 + u^2) grad w + 2 u grad u w): a QpOperatorGpu with scalar diffusion 1 + u^2
//             and flux gamma = 2 u grad u, both formed on the device from the same two arrays
//   solve     J d = -R by BiCGStab preconditioned with the inverse diagonal, to 1e-12 |R|; u += d (d is zero on every
//             constrained dof).  Only norms and dot products return to the host.
//             -DNEWTON_DEVICE_BICGSTAB (the -devbicg binaries): the same solver with its loop on the device,
//             SolverBicgstabDevice; same arguments and output lines
//   error     L2 error of the last iterate on QGauss(p+2)
// usage: newton-<dim>d-p<k> [-q] [min_cycle] [max_cycle]     (default max_cycle 6 - dim)
// -q prints one line per cycle:
//   dim  degree  n_dofs  newton_steps  inner_iterations  wall_seconds  l2_error
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <iostream>

#include "mfgpu_shim_qop.h"

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

  const unsigned int N = dof_handler.n_dofs();
  size_t nq = dof_handler.desc.n_cells;
  for (int i = 0; i < dim; ++i) nq *= fe_degree + 1;
  std::vector<number> ub_host(N, 0.0);
  VectorTools::interpolate_boundary_values(dof_handler, Solution<dim>(), ub_host);
  VectorType solution(ub_host), update(N), residual(N);
  std::vector<number> mf_host(nq);  // -f
  const number *xq = static_cast<const number *>(dof_handler.desc.quadrature_points);
  const Solution<dim> exact;
  for (size_t q = 0; q < nq; ++q) {
    double g[dim], gg = 0;
    const double u = exact.value(xq + q * dim);
    exact.gradient(xq + q * dim, g);
    for (int d = 0; d < dim; ++d) gg += g[d] * g[d];
    mf_host[q] = (1.0 + u * u) * exact.laplacian(xq + q * dim) + 2.0 * u * gg;
  }
  const unsigned int nqu = (unsigned int)nq, nqd = (unsigned int)(nq * dim);
  VectorType minus_f_qp(mf_host), u_qp(nqu), a_qp(nqu), ones_qp(nqu), grad_qp(nqd), u_rep(nqd), flux_qp(nqd), gamma_qp(nqd);
  ones_qp = 1.0;
  mfgpu_desc integrator_desc = dof_handler.desc;
  integrator_desc.flags |= MFGPU_UPDATABLE_COEFFICIENTS;  // inv_jac on the device: gradients, and the folds of the operator
  PoissonIntegrator<dim> integrator(integrator_desc);
  QuadraturePointReplicator replicator(nq, dim);
  QpOperatorGpu<dim, fe_degree> jacobian;
  jacobian.reinit(dof_handler, integrator, MFGPU_QOP_DIFFUSION_SCALAR | MFGPU_QOP_FLUX);

  unsigned int newton = 0, inner = 0;
  mfgpu_device_synchronize();
  const auto t0 = std::chrono::steady_clock::now();
  for (; newton < 50;) {
    // u, grad u, a = 1 + u^2 at the quadrature points; flux = a grad u, gamma = 2 u grad u
    VectorTools::point_values_and_gradients(integrator, solution, u_qp, grad_qp);
    a_qp.equ(1, u_qp);
    a_qp.scale(u_qp);
    a_qp.sadd(1, 1, ones_qp);
    replicator.replicate(u_rep, u_qp);
    gamma_qp.equ(2, u_rep);
    gamma_qp.scale(grad_qp);
    replicator.replicate(flux_qp, a_qp);
    flux_qp.scale(grad_qp);
    VectorTools::integrate_point_data(integrator, residual, &minus_f_qp, &flux_qp);
    jacobian.set_coefficients(&a_qp, nullptr, &gamma_qp, nullptr);
    jacobian.compute_diagonal();
    residual *= -1.0;
    SolverControl solver_control(10000, 1e-12 * residual.l2_norm());
#ifdef NEWTON_DEVICE_BICGSTAB
    SolverBicgstabDevice<VectorType> bicgstab(solver_control);  // the loop on the device (mfgpu_bicgstab): -devbicg
#else
    SolverBicgstab<VectorType> bicgstab(solver_control);
#endif
    bicgstab.solve(jacobian, update, residual, *jacobian.get_diagonal_inverse());
    inner += solver_control.last_step();
    ++newton;
    solution += update;
    const double change = update.l2_norm() / solution.l2_norm();
    if (!QUIET) std::cout << "   Newton step " << newton << ": " << solver_control.last_step() << " BiCGStab iterations, relative update " << change << std::endl;
    if (change <= 1e-10) break;
  }
  mfgpu_device_synchronize();
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

  const double l2 = VectorTools::integrate_difference(integrator, solution);
  if (!QUIET) {
    std::cout << "Time solve (" << newton << " Newton steps, " << inner << " iterations)  (wall) " << wall << "s\n";
    std::cout.precision(6);
    std::cout << "L2 error: " << l2 * l2 << std::endl;
  } else {
    printf("%8d %8d %12u %8u %8u %14.8g %14.8g\n", dim, fe_degree, N, newton, inner, wall, l2);
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
