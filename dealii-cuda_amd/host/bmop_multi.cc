// bmop for a block of vectors: bmop.cc's protocol (100 consecutive applies, swap of source and destination before each,
// wall time around the loop) with LaplaceOperatorGpu::vmult_multi on n_vectors vectors laid out one after the other.
// Arguments: n_ref n_vectors [mode], mode = 0 the library's choice (default), 1 MFGPU_MULTI_LOOP, 2 MFGPU_MULTI_FUSED.
// Output: bmop's line with the seconds per block apply, and behind it n_vectors and DoFs x vectors per second.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <iostream>

#include "mfgpu_shim.h"

using namespace mfgpu_shim;

#define N_ITERATIONS 100

#ifdef DEGREE_FE
const unsigned int degree_finite_element = DEGREE_FE;
#else
const unsigned int degree_finite_element = 4;
#endif

#ifdef DIMENSION
const unsigned int dimension = DIMENSION;
#else
const unsigned int dimension = 3;
#endif

#ifdef BMOP_USE_FLOATS
typedef float number;
#else
typedef double number;
#endif

template <int dim, int fe_degree>
class LaplaceBlockProblem {
public:
  LaplaceBlockProblem() : fe(fe_degree), dof_handler(triangulation) {}
  void run(int n_ref, unsigned int n_vectors, unsigned int flags) {
#ifdef BALL_GRID
    const domain_case_t domain = BALL;
#else
    const domain_case_t domain = CUBE;
#endif
    bmop_setup_mesh(triangulation, domain, false, n_ref);
    system_matrix.clear();
    dof_handler.distribute_dofs(fe, number_type<number>());
    constraints.clear();
    constraints.close();
    system_matrix.reinit(dof_handler, constraints);
    const std::size_t stride = system_matrix.n();
    dst.reinit((unsigned int)(stride * n_vectors));
    src.reinit((unsigned int)(stride * n_vectors));
    dst = number(0.1);
    src = number(0.1);
    system_matrix.vmult_multi(dst, src, n_vectors, stride, flags);  // (allocates the group's halo buffers)
    mfgpu_device_synchronize();
    const auto t0 = std::chrono::steady_clock::now();
    dst = number(0.1);  // IC
    for (unsigned int i = 0; i < N_ITERATIONS; ++i) {
      dst.swap(src);
      system_matrix.vmult_multi(dst, src, n_vectors, stride, flags);
    }
    mfgpu_device_synchronize();
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / N_ITERATIONS;
    printf("%d\t%d\t%u\t%g\t%u\t%g\n", dim, fe_degree, dof_handler.n_dofs(), wall, n_vectors,
           (double)dof_handler.n_dofs() * n_vectors / wall);
  }

private:
  Triangulation<dim> triangulation;
  FE_Q<dim> fe;
  DoFHandler<dim> dof_handler;
  ConstraintMatrix constraints;
  LaplaceOperatorGpu<dim, fe_degree, number> system_matrix;
  GpuVector<number> src, dst;
};

int main(int argc, char **argv) {
  try {
    const int n_ref = argc > 1 ? atoi(argv[1]) : 1;
    const int n_vectors = argc > 2 ? atoi(argv[2]) : 3;
    const int mode = argc > 3 ? atoi(argv[3]) : 0;
    if (n_vectors < 1 || mode < 0 || mode > 2) {
      std::cerr << "usage: bmop-multi n_ref n_vectors [0 auto | 1 loop | 2 fused]" << std::endl;
      return 2;
    }
    LaplaceBlockProblem<dimension, degree_finite_element> problem;
    problem.run(n_ref, (unsigned int)n_vectors, mode == 1 ? MFGPU_MULTI_LOOP : mode == 2 ? MFGPU_MULTI_FUSED : 0u);
  } catch (std::exception &exc) {
    std::cerr << "\n\n----------------------------------------------------\n"
              << "Exception on processing: \n" << exc.what() << "\nAborting!\n"
              << "----------------------------------------------------" << std::endl;
    return 1;
  }
  return 0;
}
