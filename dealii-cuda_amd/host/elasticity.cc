// elasticity: -div sigma(u) = f on hyper_cube(-1,1), clamped on the whole boundary, with the isotropic law
// sigma = lambda (div u) I + mu (grad u + grad u^T) and smoothly varying Lame parameters mu = 1 + |x|^2 / 2,
// lambda = 2 mu, on the vector-valued operator of the C-ABI (mfgpu_vqop).  The reference has no such program.
//   solution  manufactured: u_a = (a + 1) prod_k sin(pi x_k), zero on the boundary; f is derived from it below
//   field     dim components in blocks, u[a * n_dofs + i]
//   rhs       one mfgpu_integrator_integrate per component (values f_a at the quadrature points)
//   solve     CG preconditioned with the inverse diagonal, to 1e-12 |b|.  Only norms and dot products return to the host.
//   error     L2 error per component on QGauss(p+2) (mfgpu_integrator_l2_error with the exact values supplied)
// usage: elasticity-<dim>d-p<k> [-q] [min_cycle] [max_cycle]     (default max_cycle 6 - dim)
// -q prints one line per cycle:
//   dim  degree  n_entries  cg_iterations  wall_seconds  l2_error_0 ... l2_error_{dim-1}
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <iostream>

#include "mfgpu_shim_vqop.h"

using namespace mfgpu_shim;

#ifndef DEGREE_FE
#define DEGREE_FE 4
#endif
#ifndef DIMENSION
#define DIMENSION 3
#endif

static bool QUIET = false;

template <int dim>
struct Manufactured {
  static double mu(const double *x) {
    double r2 = 0;
    for (int k = 0; k < dim; ++k) r2 += x[k] * x[k];
    return 1.0 + 0.5 * r2;
  }
  static double lambda(const double *x) { return 2.0 * mu(x); }
  static double shape(const double *x) {  // S = prod_k sin(pi x_k); u_a = (a + 1) S
    double s = 1;
    for (int k = 0; k < dim; ++k) s *= std::sin(M_PI * x[k]);
    return s;
  }
  // f_a = -d_k sigma_ak = -[ d_a lambda div u + lambda d_a div u + d_k mu (d_k u_a + d_a u_k) + mu (lap u_a + d_a div u) ]
  static void load(const double *x, double *f) {
    double s[dim], c[dim], G[dim], H[dim][dim];
    for (int k = 0; k < dim; ++k) s[k] = std::sin(M_PI * x[k]), c[k] = std::cos(M_PI * x[k]);
    for (int k = 0; k < dim; ++k)
      for (int l = 0; l < dim; ++l) {
        double v = M_PI * M_PI;
        for (int j = 0; j < dim; ++j) v *= (k == l ? (j == k ? -s[j] : s[j]) : (j == k || j == l ? c[j] : s[j]));
        H[k][l] = v;  // d_k d_l S
      }
    for (int k = 0; k < dim; ++k) {
      double v = M_PI;
      for (int j = 0; j < dim; ++j) v *= j == k ? c[j] : s[j];
      G[k] = v;  // d_k S
    }
    const double m = mu(x), lam = lambda(x);
    double div = 0, lap = 0;
    for (int b = 0; b < dim; ++b) div += (b + 1) * G[b], lap += H[b][b];
    for (int a = 0; a < dim; ++a) {
      double ddiv = 0, dmu_term = 0;
      for (int b = 0; b < dim; ++b) ddiv += (b + 1) * H[a][b];
      for (int k = 0; k < dim; ++k) dmu_term += x[k] * ((a + 1) * G[k] + (k + 1) * G[a]);  // d_k mu = x_k
      f[a] = -(2.0 * x[a] * div + lam * ddiv + dmu_term + m * ((a + 1) * lap + ddiv));      // d_a lambda = 2 x_a
    }
  }
};

template <int dim, int fe_degree>
void run_cycle(unsigned int cycle) {
  typedef GpuVector<double> VectorType;
  Triangulation<dim> triangulation;
  bmop_setup_mesh(triangulation, CUBE, false, 1 + (3 - dim) + 1 + (int)cycle);
  FE_Q<dim> fe(fe_degree);
  DoFHandler<dim> dof_handler(triangulation);
  ConstraintMatrix constraints;
  dof_handler.distribute_dofs(fe, number_type<double>());
  constraints.close();
  const unsigned int N = dof_handler.n_dofs(), n_cells = dof_handler.desc.n_cells;
  if (!QUIET) {
    std::cout << "Cycle " << cycle << std::endl;
    std::cout << "   Number of active cells:       " << n_cells << std::endl;
    std::cout << "   Number of degrees of freedom: " << dim * N << " (" << dim << " x " << N << ")" << std::endl;
  }
  size_t nq = n_cells, ne = n_cells;
  for (int i = 0; i < dim; ++i) nq *= fe_degree + 1, ne *= fe_degree + 2;

  mfgpu_desc integrator_desc = dof_handler.desc;
  integrator_desc.flags |= MFGPU_UPDATABLE_COEFFICIENTS;  // inv_jac on the device: the stress terms need it
  PoissonIntegrator<dim> integrator(integrator_desc);

  // lambda, mu and the load at the quadrature points
  const double *xq = static_cast<const double *>(dof_handler.desc.quadrature_points);
  std::vector<double> lam_host(nq), mu_host(nq);
  std::vector<std::vector<double>> f_host(dim, std::vector<double>(nq));
  for (size_t q = 0; q < nq; ++q) {
    double f[dim];
    Manufactured<dim>::load(xq + q * dim, f);
    lam_host[q] = Manufactured<dim>::lambda(xq + q * dim);
    mu_host[q] = Manufactured<dim>::mu(xq + q * dim);
    for (int a = 0; a < dim; ++a) f_host[a][q] = f[a];
  }
  VectorType lam_qp(lam_host), mu_qp(mu_host);
  VectorQpOperatorGpu<dim, fe_degree> elasticity;
  elasticity.reinit(dof_handler, integrator, MFGPU_VQOP_ISOTROPIC);
  elasticity.set_coefficients(&lam_qp, &mu_qp, nullptr, nullptr);
  elasticity.compute_diagonal();

  VectorType rhs(dim * N), solution(dim * N);
  for (int a = 0; a < dim; ++a) {
    VectorType f_qp(f_host[a]), rhs_a = component(rhs, a, N);
    VectorTools::integrate_point_data(integrator, rhs_a, &f_qp, nullptr);
    mfgpu_device_synchronize();  // f_qp is freed at the end of the iteration
  }

  mfgpu_device_synchronize();
  const auto t0 = std::chrono::steady_clock::now();
  SolverControl solver_control(20000, 1e-12 * rhs.l2_norm());
  SolverCG<VectorType> cg(solver_control);
  cg.solve(elasticity, solution, rhs, *elasticity.get_diagonal_inverse());
  mfgpu_device_synchronize();
  const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

  // the exact components at the error points
  VectorType points((unsigned int)(ne * dim));
  check(mfgpu_integrator_error_points(integrator.it, points.getData(), nullptr), "mfgpu_integrator_error_points");
  const std::vector<double> xe = points.toVector();
  std::vector<double> s_host(ne);
  for (size_t k = 0; k < ne; ++k) s_host[k] = Manufactured<dim>::shape(xe.data() + k * dim);
  double l2[dim];
  for (int a = 0; a < dim; ++a) {
    std::vector<double> exact_host(ne);
    for (size_t k = 0; k < ne; ++k) exact_host[k] = (a + 1) * s_host[k];
    VectorType exact(exact_host), u_a = component(solution, a, N);
    check(mfgpu_integrator_l2_error(integrator.it, u_a.getDataRO(), exact.getDataRO(), nullptr, nullptr, &l2[a]),
          "mfgpu_integrator_l2_error");
  }
  if (!QUIET) {
    std::cout << "Time solve (" << solver_control.last_step() << " CG iterations)  (wall) " << wall << "s\n";
    for (int a = 0; a < dim; ++a) std::cout << "L2 error of component " << a << ": " << l2[a] << std::endl;
  } else {
    printf("%8d %8d %12u %8u %14.8g", dim, fe_degree, dim * N, solver_control.last_step(), wall);
    for (int a = 0; a < dim; ++a) printf(" %14.8g", l2[a]);
    printf("\n");
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
