// Vector-valued side of the shim: the elasticity operator on quadrature-point coefficients (include/mfgpu.h,
// "mfgpu_vqop").  A field has dim components in blocks, u[a * n_dofs + i]; component(v, a) is the scalar vector of one.
//   VectorQpOperatorGpu<dim, fe_degree>   (A u)_(a,i) = sum_q JxW [sum_k d_k phi_i sigma_ak + phi_i rho u_a] in the member
//                                         style of QpOperatorGpu: vmult, Tvmult (isotropic operators only: they are
//                                         symmetric, so Tvmult is vmult; a TENSOR4 operator throws -- transpose C
//                                         instead), compute_diagonal, get_diagonal_inverse, set_coefficients(...).  The
//                                         SolverCG and SolverBicgstab templates take it as it is, SolverBicgstabDevice
//                                         through its callback path.
#ifndef MFGPU_SHIM_VQOP_H
#define MFGPU_SHIM_VQOP_H

#include "mfgpu_shim_qop.h"

namespace mfgpu_shim {

// component a of a block vector as a scalar vector of n_dofs entries (borrowed memory)
inline GpuVector<double> component(GpuVector<double> &v, unsigned int a, unsigned int n_dofs) {
  return GpuVector<double>(v.getData() + (std::size_t)a * n_dofs, n_dofs, GpuVector<double>::borrowed_t());
}

template <int dim, int fe_degree>
class VectorQpOperatorGpu {
public:
  typedef double value_type;
  typedef GpuVector<double> VectorType;

  VectorQpOperatorGpu() = default;
  VectorQpOperatorGpu(const VectorQpOperatorGpu &) = delete;
  VectorQpOperatorGpu &operator=(const VectorQpOperatorGpu &) = delete;
  ~VectorQpOperatorGpu() { clear(); }

  void clear() {
    mfgpu_vqop_destroy(vqop);
    vqop = nullptr;
    diagonal_is_available = false;
  }

  // terms: MFGPU_VQOP_* bits.  constrained: ascending block indices, or nullptr for the description's list in every
  // component.  The integrator (created with MFGPU_UPDATABLE_COEFFICIENTS unless the operator is a mass term alone) must
  // outlive the operator.
  void reinit(const DoFHandler<dim> &dof_handler, PoissonIntegrator<dim> &integrator, uint32_t terms,
              const std::vector<uint32_t> *constrained = nullptr) {
    if ((int)dof_handler.degree != fe_degree) throw std::runtime_error("FE degree mismatch");
    clear();
    static const uint32_t none = 0;
    check(mfgpu_vqop_create(integrator.it, terms, constrained ? (constrained->empty() ? &none : constrained->data()) : nullptr,
                            constrained ? constrained->size() : 0, &vqop),
          "VectorQpOperatorGpu::reinit");
    n_entries = dim * dof_handler.desc.n_dofs;
    symmetric = !(terms & MFGPU_VQOP_TENSOR4);
  }
  // device vectors at the quadrature points, nullptr = keep the term's last values (or the term is absent); lambda and
  // mu go together; asynchronous.  The inverse diagonal of the old coefficients is stale afterwards.
  void set_coefficients(const VectorType *lambda, const VectorType *mu, const VectorType *tensor, const VectorType *mass) {
    mfgpu_vqop_coefficients c;
    c.lambda = lambda ? lambda->getDataRO() : nullptr;
    c.mu = mu ? mu->getDataRO() : nullptr;
    c.tensor = tensor ? tensor->getDataRO() : nullptr;
    c.mass = mass ? mass->getDataRO() : nullptr;
    check(mfgpu_vqop_set_coefficients(vqop, &c, nullptr), "VectorQpOperatorGpu::set_coefficients");
    diagonal_is_available = false;
  }

  unsigned int m() const { return n_entries; }
  unsigned int n() const { return n_entries; }
  void vmult(VectorType &dst, const VectorType &src) const {
    check(mfgpu_vqop_vmult(vqop, dst.getData(), src.getDataRO(), nullptr), "VectorQpOperatorGpu::vmult");
  }
  void Tvmult(VectorType &dst, const VectorType &src) const {
    if (!symmetric) throw std::runtime_error("VectorQpOperatorGpu::Tvmult: a TENSOR4 operator has no transpose apply");
    vmult(dst, src);
  }
  double el(unsigned int, unsigned int) const { throw std::runtime_error("matrix-free: no element access"); }
  void set_constrained_values(VectorType &v, double value) const {
    check(mfgpu_vqop_set_constrained_values(vqop, v.getData(), value, nullptr), "VectorQpOperatorGpu::set_constrained_values");
  }
  void compute_diagonal() {
    if (!inverse_diagonal_matrix) inverse_diagonal_matrix = std::make_shared<DiagonalMatrix<double>>();
    VectorType &inv_diag = inverse_diagonal_matrix->get_vector();
    if (inv_diag.size() != m()) inv_diag.reinit(m());
    check(mfgpu_vqop_compute_inverse_diagonal(vqop, inv_diag.getData(), nullptr), "VectorQpOperatorGpu::compute_diagonal");
    diagonal_is_available = true;
  }
  const std::shared_ptr<DiagonalMatrix<double>> get_diagonal_inverse() const {
    if (!diagonal_is_available) throw std::runtime_error("get_diagonal_inverse: call compute_diagonal first");
    return inverse_diagonal_matrix;
  }
  std::size_t memory_consumption() const { return mfgpu_vqop_memory_consumption(vqop); }
  mfgpu_vqop *get_vqop() const { return vqop; }

private:
  mfgpu_vqop *vqop = nullptr;
  unsigned int n_entries = 0;
  bool symmetric = true;
  std::shared_ptr<DiagonalMatrix<double>> inverse_diagonal_matrix;
  bool diagonal_is_available = false;
};

}  // namespace mfgpu_shim
#endif
