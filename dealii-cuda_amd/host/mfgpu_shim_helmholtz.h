// Helmholtz side of the shim: the operator -div(a grad u) + c u behind the member set of LaplaceOperatorGpu.
//   HelmholtzOperatorGpu<dim, fe_degree, Number>   LaplaceOperatorGpu (laplace_operator_gpu.h:85-95) plus a mass term:
//                                          reinit(dof_handler, constraints, mass_function) evaluates c at the quadrature
//                                          points and hands it to mfgpu_create as mfgpu_desc.mass_coefficient.  The
//                                          reference has no such operator; this is what a caller of its FEEvaluationGpu
//                                          would write with get_value / submit_value next to the gradient calls.
//   RightHandSide<dim>                     poisson_common.h:277-296 on the host (the load of the Poisson problem)
//   VectorTools::create_right_hand_side    overload with the load given at the quadrature points
// LaplaceOperatorGpu itself is untouched (mfgpu_shim.h).
#ifndef MFGPU_SHIM_HELMHOLTZ_H
#define MFGPU_SHIM_HELMHOLTZ_H

#include "mfgpu_shim_poisson.h"

namespace mfgpu_shim {

template <int dim, int fe_degree, typename Number>
class HelmholtzOperatorGpu {
public:
  typedef Number value_type;
  typedef GpuVector<Number> VectorType;

  HelmholtzOperatorGpu() = default;
  HelmholtzOperatorGpu(const HelmholtzOperatorGpu &) = delete;
  HelmholtzOperatorGpu &operator=(const HelmholtzOperatorGpu &) = delete;
  ~HelmholtzOperatorGpu() { clear(); }

  void clear() {
    mfgpu_destroy(handle);
    handle = nullptr;
    diagonal_is_available = false;
  }

  // mass_function: double(const double *x) -> c(x), called once per quadrature point on the host
  template <typename MassFunction>
  void reinit(const DoFHandler<dim> &dof_handler, const ConstraintMatrix &constraints, const MassFunction &mass_function) {
    if ((int)dof_handler.degree != fe_degree) throw std::runtime_error("FE degree mismatch");
    clear();
    mfgpu_desc d = dof_handler.desc;
    if (d.number_type != number_type<Number>()) throw std::runtime_error("mesh / operator number type mismatch");
    if (!d.quadrature_points) throw std::runtime_error("HelmholtzOperatorGpu: the mesh has no quadrature points");
    unsigned int nd = 1;
    for (int i = 0; i < dim; ++i) nd *= fe_degree + 1;
    const size_t nq = (size_t)d.n_cells * nd;
    const Number *xq = static_cast<const Number *>(d.quadrature_points);
    mass_values.resize(nq);
    for (size_t q = 0; q < nq; ++q) {
      double x[dim];
      for (int e = 0; e < dim; ++e) x[e] = (double)xq[q * dim + e];
      mass_values[q] = (Number)mass_function(x);
    }
    d.mass_coefficient = mass_values.data();
#ifdef MATRIX_FREE_COLOR
    d.flags |= MFGPU_COLORED_SCATTER;
#endif
    check(mfgpu_create(&d, &handle), "HelmholtzOperatorGpu::reinit");
    n_dofs = d.n_dofs;
    constraint_handler.reinit(constraints, dof_handler.desc);
  }
  // the values of c at the quadrature points [n_cells * (p+1)^dim], e.g. for the description of an mfgpu_integrator
  // (valid until the next reinit)
  const std::vector<Number> &mass_coefficient() const { return mass_values; }

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
    inv_diag.reinit(m());
    check(mfgpu_compute_inverse_diagonal(handle, inv_diag.getData(), nullptr), "compute_diagonal");
    diagonal_is_available = true;
  }
  const std::shared_ptr<DiagonalMatrix<Number>> get_diagonal_inverse() const {
    if (!diagonal_is_available) throw std::runtime_error("get_diagonal_inverse: call compute_diagonal first");
    return inverse_diagonal_matrix;
  }
  void set_constrained_values(VectorType &v, Number value) const {
    check(mfgpu_set_constrained_values(handle, v.getData(), (double)value, nullptr), "set_constrained_values");
  }
  std::size_t memory_consumption() const {
    return mfgpu_memory_consumption(handle) + constraint_handler.memory_consumption();
  }

private:
  mfgpu_handle *handle = nullptr;
  unsigned int n_dofs = 0;
  std::vector<Number> mass_values;
  mutable ConstraintHandlerGpu<Number> constraint_handler;
  std::shared_ptr<DiagonalMatrix<Number>> inverse_diagonal_matrix;
  bool diagonal_is_available = false;
};

// RightHandSide<dim>::value (poisson_common.h:277-296): -(laplacian(u) a + grad a . grad u) with the coefficient
// a = 1 / (0.05 + 2 |x|^2) (poisson_common.h:146-170) and u = Solution<dim>
template <int dim>
class RightHandSide {
public:
  double value(const double *p) const {
    const Solution<dim> u;
    double xx = 0, g[dim], ga_gu = 0;
    for (int d = 0; d < dim; ++d) xx += p[d] * p[d];
    const double den = 0.05 + 2. * xx;
    u.gradient(p, g);
    for (int d = 0; d < dim; ++d) ga_gu += (4. / (den * den)) * (-p[d]) * g[d];
    return -(u.laplacian(p) / den + ga_gu);
  }
};

namespace VectorTools {
// rhs = int phi_i f - lift terms, f given at the quadrature points of every cell [n_cells * (p+1)^dim] (device)
template <int dim>
void create_right_hand_side(PoissonIntegrator<dim> &integrator, GpuVector<double> &rhs, const GpuVector<double> &f_qp,
                            const GpuVector<double> *lift) {
  check(mfgpu_integrator_rhs(integrator.it, rhs.getData(), f_qp.getDataRO(), lift ? lift->getDataRO() : nullptr, nullptr),
        "create_right_hand_side");
}
}  // namespace VectorTools

}  // namespace mfgpu_shim
#endif
