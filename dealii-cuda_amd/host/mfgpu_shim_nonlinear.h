// Nonlinear side of the shim: an operator -div(a grad u) whose coefficient a lives on the device and changes between
// solves (a = a(u) in a Picard or Newton loop, a = a(t) in a time loop).
//   UpdatableOperatorGpu<dim, fe_degree, Number>   the member set of LaplaceOperatorGpu (laplace_operator_gpu.h:85-95) on
//                                          a handle created with MFGPU_UPDATABLE_COEFFICIENTS, plus
//                                          update_coefficients(a_qp): the new coefficient at the quadrature points, a
//                                          device vector [n_cells * (p+1)^dim]; the plan and the index uploads are kept.
//                                          The reference evaluates its coefficient once in reinit
//                                          (laplace_operator_gpu.h:191-211) and has no counterpart.
//   VectorTools::point_values / point_gradients    the field at the quadrature points (mfgpu_integrator_evaluate: the
//                                          read_dof_values + evaluate + get_value / get_gradient half of FEEvaluationGpu)
//   update_coefficients(integrator, a_qp)  the same coefficient for the Dirichlet lift of create_right_hand_side
#ifndef MFGPU_SHIM_NONLINEAR_H
#define MFGPU_SHIM_NONLINEAR_H

#include "mfgpu_shim_helmholtz.h"

namespace mfgpu_shim {

template <int dim, int fe_degree, typename Number>
class UpdatableOperatorGpu {
public:
  typedef Number value_type;
  typedef GpuVector<Number> VectorType;

  UpdatableOperatorGpu() = default;
  UpdatableOperatorGpu(const UpdatableOperatorGpu &) = delete;
  UpdatableOperatorGpu &operator=(const UpdatableOperatorGpu &) = delete;
  ~UpdatableOperatorGpu() { clear(); }

  void clear() {
    mfgpu_destroy(handle);
    handle = nullptr;
    diagonal_is_available = false;
  }

  // the operator with a = 1 until the first update_coefficients
  void reinit(const DoFHandler<dim> &dof_handler, const ConstraintMatrix &constraints) {
    if ((int)dof_handler.degree != fe_degree) throw std::runtime_error("FE degree mismatch");
    clear();
    mfgpu_desc d = dof_handler.desc;
    if (d.number_type != number_type<Number>()) throw std::runtime_error("mesh / operator number type mismatch");
    n_qp = d.n_cells;
    for (int i = 0; i < dim; ++i) n_qp *= fe_degree + 1;
    const std::vector<Number> ones(n_qp, Number(1));
    d.coefficient = ones.data();
    d.flags |= MFGPU_UPDATABLE_COEFFICIENTS;
    check(mfgpu_create(&d, &handle), "UpdatableOperatorGpu::reinit");
    n_dofs = d.n_dofs;
    constraint_handler.reinit(constraints, dof_handler.desc);
  }
  // quadrature points of the mesh: the length of a coefficient vector
  std::size_t n_quadrature_points() const { return n_qp; }
  // asynchronous; the inverse diagonal of the old coefficient is stale afterwards
  void update_coefficients(const VectorType &a_qp) {
    if (a_qp.size() != n_qp) throw std::runtime_error("update_coefficients: one value per quadrature point");
    check(mfgpu_update_coefficients(handle, a_qp.getDataRO(), nullptr, nullptr), "update_coefficients");
    diagonal_is_available = false;
  }

  unsigned int m() const { return n_dofs; }
  unsigned int n() const { return n_dofs; }
  void vmult(VectorType &dst, const VectorType &src) const {
    check(mfgpu_vmult(handle, dst.getData(), src.getDataRO(), nullptr), "vmult");
  }
  void Tvmult(VectorType &dst, const VectorType &src) const { vmult(dst, src); }  // symmetric
  void vmult_add(VectorType &dst, const VectorType &src) const {
    check(mfgpu_vmult_add(handle, dst.getData(), src.getDataRO(), nullptr), "vmult_add");
  }
  void Tvmult_add(VectorType &dst, const VectorType &src) const { vmult_add(dst, src); }
  Number el(unsigned int, unsigned int) const { throw std::runtime_error("matrix-free: no element access"); }
  void compute_diagonal() {
    if (!inverse_diagonal_matrix) inverse_diagonal_matrix = std::make_shared<DiagonalMatrix<Number>>();
    VectorType &inv_diag = inverse_diagonal_matrix->get_vector();
    if (inv_diag.size() != m()) inv_diag.reinit(m());
    check(mfgpu_compute_inverse_diagonal(handle, inv_diag.getData(), nullptr), "compute_diagonal");
    diagonal_is_available = true;
  }
  const std::shared_ptr<DiagonalMatrix<Number>> get_diagonal_inverse() const {
    if (!diagonal_is_available) throw std::runtime_error("get_diagonal_inverse: call compute_diagonal first");
    return inverse_diagonal_matrix;
  }
  std::size_t memory_consumption() const {
    return mfgpu_memory_consumption(handle) + constraint_handler.memory_consumption();
  }

private:
  mfgpu_handle *handle = nullptr;
  unsigned int n_dofs = 0;
  std::size_t n_qp = 0;
  mutable ConstraintHandlerGpu<Number> constraint_handler;
  std::shared_ptr<DiagonalMatrix<Number>> inverse_diagonal_matrix;
  bool diagonal_is_available = false;
};

// the coefficient of the Dirichlet lift (integrator created from a description with MFGPU_UPDATABLE_COEFFICIENTS)
template <int dim>
void update_coefficients(PoissonIntegrator<dim> &integrator, const GpuVector<double> &a_qp) {
  check(mfgpu_integrator_update_coefficients(integrator.it, a_qp.getDataRO(), nullptr, nullptr),
        "update_coefficients (integrator)");
}

namespace VectorTools {
// values_qp[cell][q] = u(x_q), [n_cells * (p+1)^dim]
template <int dim>
void point_values(PoissonIntegrator<dim> &integrator, const GpuVector<double> &u, GpuVector<double> &values_qp) {
  check(mfgpu_integrator_evaluate(integrator.it, u.getDataRO(), values_qp.getData(), nullptr, nullptr), "point_values");
}
// gradients_qp[cell][q][d] = du/dx_d(x_q), [n_cells * (p+1)^dim * dim]
template <int dim>
void point_gradients(PoissonIntegrator<dim> &integrator, const GpuVector<double> &u, GpuVector<double> &gradients_qp) {
  check(mfgpu_integrator_evaluate(integrator.it, u.getDataRO(), nullptr, gradients_qp.getData(), nullptr),
        "point_gradients");
}
// both in one pass over the cells
template <int dim>
void point_values_and_gradients(PoissonIntegrator<dim> &integrator, const GpuVector<double> &u, GpuVector<double> &values_qp,
                                GpuVector<double> &gradients_qp) {
  check(mfgpu_integrator_evaluate(integrator.it, u.getDataRO(), values_qp.getData(), gradients_qp.getData(), nullptr),
        "point_values_and_gradients");
}
}  // namespace VectorTools

}  // namespace mfgpu_shim
#endif
