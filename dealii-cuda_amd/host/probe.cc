// poisson-probe: the Poisson problem of poisson.cc solved once, then sampled at points of the caller's choosing --
// mfgpu_points (include/mfgpu.h) from C++, the counterpart of deal.II's VectorTools::point_value on a solution vector.
//   mesh      hyper_cube(-1,1) with 2^n_ref cells per direction; -DBALL_GRID: hyper_ball after n_ref refinements;
//             -DADAPTIVE_GRID: the pseudo-adaptive stand-in mesh with hanging nodes at n_ref
//   solve     as poisson.cc (lift, right-hand side, Chebyshev-preconditioned CG), but to 1e-14 |rhs|: the point values
//             are compared across implementations to 1e-10, so the solver runs to its rounding floor
//   probe     n_points points of a fixed seeded set inside the domain (xorshift32 from 2463534242; coordinates in
//             (-0.999, 0.999) on the cube, in (-0.3, 0.3) on the ball, which lies inside the mesh at every n_ref),
//             located and evaluated by mfgpu_points_create / mfgpu_points_evaluate
// usage: poisson-probe-<dim>d-p<k>[-adaptive|-ball] n_ref n_points
// prints, next to the L2 error in poisson.cc's style, the number of points found and max |u_h - Solution| over them.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <iostream>
#include <vector>

#include "mfgpu_shim_poisson.h"

using namespace mfgpu_shim;

#ifndef DEGREE_FE
#define DEGREE_FE 4
#endif
#ifndef DIMENSION
#define DIMENSION 3
#endif
typedef double number;

template <int dim, int fe_degree>
void run(int n_ref, unsigned int n_points) {
  typedef GpuVector<number> VectorType;
  Triangulation<dim> triangulation;
#if defined(BALL_GRID)
  bmop_setup_mesh(triangulation, BALL, false, n_ref);
  const double extent = 0.3;
#elif defined(ADAPTIVE_GRID)
  bmop_setup_mesh(triangulation, CUBE, true, n_ref);
  const double extent = 0.999;
#else
  bmop_setup_mesh(triangulation, CUBE, false, n_ref);
  const double extent = 0.999;
#endif
  FE_Q<dim> fe(fe_degree);
  DoFHandler<dim> dof_handler(triangulation);
  ConstraintMatrix constraints;
  dof_handler.distribute_dofs(fe, number_type<number>());
  constraints.close();
  std::cout << "Cycle " << n_ref << std::endl;
  std::cout << "   Number of active cells:       " << dof_handler.desc.n_cells << std::endl;
  std::cout << "   Number of degrees of freedom: " << dof_handler.n_dofs() << std::endl;

  LaplaceOperatorGpu<dim, fe_degree, number> system_matrix;
  system_matrix.reinit(dof_handler, constraints);
  const unsigned int N = system_matrix.n();
  std::vector<number> ub_host(N, 0.0);
  VectorTools::interpolate_boundary_values(dof_handler, Solution<dim>(), ub_host);
  VectorType solution(ub_host), solution_update(N), system_rhs(N);
  PoissonIntegrator<dim> integrator(dof_handler);
  VectorTools::create_right_hand_side(integrator, system_rhs, &solution);
  system_matrix.compute_diagonal();

  typedef PreconditionChebyshev<LaplaceOperatorGpu<dim, fe_degree, number>, VectorType> PreconditionType;
  PreconditionType preconditioner;
  typename PreconditionType::AdditionalData additional_data;
  additional_data.preconditioner = system_matrix.get_diagonal_inverse();
  preconditioner.initialize(system_matrix, additional_data);
  SolverControl solver_control(10000, 1e-14 * system_rhs.l2_norm());
  SolverCG<VectorType> cg(solver_control);
  mfgpu_device_synchronize();
  const auto t0 = std::chrono::steady_clock::now();
  cg.solve(system_matrix, solution_update, system_rhs, preconditioner);
  mfgpu_device_synchronize();
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  solution += solution_update;
  const double l2 = VectorTools::integrate_difference(integrator, solution);
  std::cout << "Time solve (" << solver_control.last_step() << " iterations)  (wall) " << wall << "s\n";
  std::cout.precision(6);
  std::cout << "L2 error: " << l2 * l2 << std::endl;

  // the probe points
  std::vector<double> x((size_t)n_points * dim);
  uint32_t state = 2463534242u;
  for (double &v : x) {
    state ^= state << 13;
    state ^= state >> 17;
    state ^= state << 5;
    v = -extent + 2 * extent * (state / 4294967296.0);
  }
  mfgpu_points *points = nullptr;
#ifdef PROBE_DEVICE_LOCATE
  // the points uploaded, located by the locator's kernel, and the object built from the device arrays
  mfgpu_locator *locator = nullptr;
  check(mfgpu_locator_create(integrator.it, &dof_handler.desc, &locator), "mfgpu_locator_create");
  VectorType x_dev(x.empty() ? std::vector<double>(1, 0.0) : x), xi_dev((size_t)n_points * dim + 1);
  GpuVector<float> cell_dev(n_points + 1);  // 4-byte device memory: holds the uint32 cells
  const auto t1 = std::chrono::steady_clock::now();
  check(mfgpu_locator_locate(locator, x_dev.getDataRO(), n_points, nullptr, (uint32_t *)cell_dev.getData(),
                             xi_dev.getData(), nullptr, nullptr), "mfgpu_locator_locate");
  check(mfgpu_points_create_located(integrator.it, (const uint32_t *)cell_dev.getDataRO(), xi_dev.getDataRO(), n_points,
                                    nullptr, &points), "mfgpu_points_create_located");
  const double t_create = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
  {  // against the host location of the same points
    std::vector<uint32_t> cell_host(n_points);
    std::vector<double> xi_host((size_t)n_points * dim);
    check(mfgpu_locate_points(&dof_handler.desc, x.data(), n_points, cell_host.data(), xi_host.data(), nullptr),
          "mfgpu_locate_points");
    const std::vector<number> xi_got = xi_dev.toVector();
    const uint32_t *cell_got = nullptr;
    mfgpu_points_cells(points, &cell_got);
    unsigned int differing = 0;
    double worst_xi = 0;
    for (unsigned int k = 0; k < n_points; ++k) {
      differing += cell_got[k] != cell_host[k];
      for (int d = 0; d < dim; ++d)
        worst_xi = std::max(worst_xi, std::fabs(xi_got[(size_t)k * dim + d] - xi_host[(size_t)k * dim + d]));
    }
    std::printf("device location: %u cells differ from the host's, max |xi_dev - xi_host| %.3e\n", differing, worst_xi);
  }
  mfgpu_locator_destroy(locator);
#else
  const auto t1 = std::chrono::steady_clock::now();
  check(mfgpu_points_create(integrator.it, &dof_handler.desc, x.data(), n_points, &points), "mfgpu_points_create");
  const double t_create = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
#endif
  VectorType values(n_points ? n_points : 1);
  check(mfgpu_points_evaluate(points, solution.getDataRO(), values.getData(), nullptr, nullptr), "mfgpu_points_evaluate");
  mfgpu_device_synchronize();
  const std::vector<number> v_host = values.toVector();
  const uint32_t *cell = nullptr;
  mfgpu_points_cells(points, &cell);
  const Solution<dim> exact;
  double worst = 0;
  for (unsigned int k = 0; k < n_points; ++k)
    if (cell[k] != MFGPU_POINT_NOT_FOUND) worst = std::max(worst, std::fabs(v_host[k] - exact.value(&x[(size_t)k * dim])));
  const unsigned int found = n_points - mfgpu_points_n_not_found(points);
  mfgpu_points_destroy(points);
  std::printf("points found: %u of %u (located in %.3g s)\n", found, n_points, t_create);
  std::printf("max point error: %.12e\n", worst);
}

int main(int argc, char **argv) {
  try {
    if (argc < 3) {
      std::cerr << "usage: " << argv[0] << " n_ref n_points" << std::endl;
      return 2;
    }
    run<DIMENSION, DEGREE_FE>(atoi(argv[1]), (unsigned int)atoi(argv[2]));
    return 0;
  } catch (std::exception &exc) {
    std::cerr << "Exception on processing: " << exc.what() << std::endl;
    return 1;
  }
}
