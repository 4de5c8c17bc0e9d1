// User-operator side of the shim: the general linear second-order operator on quadrature-point coefficients
// (include/mfgpu.h, "mfgpu_qop") and the integrate half of FEEvaluationGpu for point data the caller formed.
//   QpOperatorGpu<dim, fe_degree>          (A u)_i = sum_q JxW [grad phi_i . (D grad u + gamma u) + phi_i (beta . grad u + c u)]
//                                          on an integrator's mesh, in the member style of UpdatableOperatorGpu: vmult,
//                                          Tvmult, compute_diagonal, get_diagonal_inverse, plus set_coefficients(...) with
//                                          device vectors at the quadrature points.  What a deal.II LocOp computes between
//                                          evaluate and integrate is here the term set.
//   VectorTools::integrate_point_data      dst_i = sum_q JxW (phi_i v_q + grad phi_i . g_q) (mfgpu_integrator_integrate)
//   SolverBicgstab<VectorType>             right-preconditioned BiCGStab, a host loop over the vector operations, in the
//                                          shape of SolverCG (mfgpu_shim_poisson.h): for the non-symmetric operators above
//   QuadraturePointReplicator              u_qp [n_qp] -> [n_qp * dim] with every value repeated dim times, so that
//                                          products of a scalar field with a vector field at the points are vector
//                                          operations (mfgpu_vec_copy_pairs)
#ifndef MFGPU_SHIM_QOP_H
#define MFGPU_SHIM_QOP_H

#include "mfgpu_shim_nonlinear.h"

namespace mfgpu_shim {

template <int dim, int fe_degree>
class QpOperatorGpu {
public:
  typedef double value_type;
  typedef GpuVector<double> VectorType;

  QpOperatorGpu() = default;
  QpOperatorGpu(const QpOperatorGpu &) = delete;
  QpOperatorGpu &operator=(const QpOperatorGpu &) = delete;
  ~QpOperatorGpu() { clear(); }

  void clear() {
    mfgpu_qop_destroy(qop);
    qop = nullptr;
    diagonal_is_available = false;
  }

  // terms: MFGPU_QOP_* bits.  The integrator (created with MFGPU_UPDATABLE_COEFFICIENTS unless the operator is a
  // reaction term alone) must outlive the operator.
  void reinit(const DoFHandler<dim> &dof_handler, PoissonIntegrator<dim> &integrator, uint32_t terms) {
    if ((int)dof_handler.degree != fe_degree) throw std::runtime_error("FE degree mismatch");
    clear();
    check(mfgpu_qop_create(integrator.it, terms, &qop), "QpOperatorGpu::reinit");
    n_dofs = dof_handler.desc.n_dofs;
  }
  // device vectors at the quadrature points, nullptr = keep the term's last values (or the term is absent); asynchronous.
  // The inverse diagonal of the old coefficients is stale afterwards.
  void set_coefficients(const VectorType *diffusion, const VectorType *convection, const VectorType *flux,
                        const VectorType *reaction) {
    mfgpu_qop_coefficients c;
    c.diffusion = diffusion ? diffusion->getDataRO() : nullptr;
    c.convection = convection ? convection->getDataRO() : nullptr;
    c.flux = flux ? flux->getDataRO() : nullptr;
    c.reaction = reaction ? reaction->getDataRO() : nullptr;
    check(mfgpu_qop_set_coefficients(qop, &c, nullptr), "QpOperatorGpu::set_coefficients");
    diagonal_is_available = false;
  }

  unsigned int m() const { return n_dofs; }
  unsigned int n() const { return n_dofs; }
  void vmult(VectorType &dst, const VectorType &src) const {
    check(mfgpu_qop_vmult(qop, dst.getData(), src.getDataRO(), 0, nullptr), "QpOperatorGpu::vmult");
  }
  void Tvmult(VectorType &dst, const VectorType &src) const {
    check(mfgpu_qop_vmult(qop, dst.getData(), src.getDataRO(), MFGPU_QOP_TRANSPOSE, nullptr), "QpOperatorGpu::Tvmult");
  }
  double el(unsigned int, unsigned int) const { throw std::runtime_error("matrix-free: no element access"); }
  void compute_diagonal() {
    if (!inverse_diagonal_matrix) inverse_diagonal_matrix = std::make_shared<DiagonalMatrix<double>>();
    VectorType &inv_diag = inverse_diagonal_matrix->get_vector();
    if (inv_diag.size() != m()) inv_diag.reinit(m());
    check(mfgpu_qop_compute_inverse_diagonal(qop, inv_diag.getData(), nullptr), "QpOperatorGpu::compute_diagonal");
    diagonal_is_available = true;
  }
  const std::shared_ptr<DiagonalMatrix<double>> get_diagonal_inverse() const {
    if (!diagonal_is_available) throw std::runtime_error("get_diagonal_inverse: call compute_diagonal first");
    return inverse_diagonal_matrix;
  }
  std::size_t memory_consumption() const { return mfgpu_qop_memory_consumption(qop); }
  mfgpu_qop *get_qop() const { return qop; }  // SolverBicgstabDevice

private:
  mfgpu_qop *qop = nullptr;
  unsigned int n_dofs = 0;
  std::shared_ptr<DiagonalMatrix<double>> inverse_diagonal_matrix;
  bool diagonal_is_available = false;
};

namespace VectorTools {
// dst_i = sum_q JxW_q (phi_i v_q + grad phi_i . g_q); values_qp [n_qp] or nullptr, gradients_qp [n_qp * dim] or nullptr;
// constrained rows 0
template <int dim>
void integrate_point_data(PoissonIntegrator<dim> &integrator, GpuVector<double> &dst, const GpuVector<double> *values_qp,
                          const GpuVector<double> *gradients_qp) {
  check(mfgpu_integrator_integrate(integrator.it, dst.getData(), values_qp ? values_qp->getDataRO() : nullptr,
                                   gradients_qp ? gradients_qp->getDataRO() : nullptr, nullptr),
        "integrate_point_data");
}
}  // namespace VectorTools

// out[q * dim + k] = in[q]
class QuadraturePointReplicator {
public:
  QuadraturePointReplicator(std::size_t n_qp, int dim) {
    std::vector<uint32_t> dst(n_qp * dim), src(n_qp * dim);
    for (std::size_t i = 0; i < dst.size(); ++i) dst[i] = (uint32_t)i, src[i] = (uint32_t)(i / dim);
    check(mfgpu_index_pairs_create(dst.data(), src.data(), (uint32_t)dst.size(), &pairs), "QuadraturePointReplicator");
  }
  ~QuadraturePointReplicator() { mfgpu_index_pairs_destroy(pairs); }
  QuadraturePointReplicator(const QuadraturePointReplicator &) = delete;
  QuadraturePointReplicator &operator=(const QuadraturePointReplicator &) = delete;
  void replicate(GpuVector<double> &out, const GpuVector<double> &in) const {
    check(mfgpu_vec_copy_pairs(pairs, out.getData(), in.getDataRO(), MFGPU_F64, nullptr), "replicate");
  }

private:
  mfgpu_index_pairs *pairs = nullptr;
};

// BiCGStab with right preconditioning, zero start (x is overwritten), until |r| <= control.tolerance; one step = two
// operator applications.  Only dot products and norms return to the host.
template <typename VectorType>
class SolverBicgstab {
public:
  explicit SolverBicgstab(SolverControl &control) : control(control) {}
  template <typename MatrixType, typename PreconditionerType>
  void solve(const MatrixType &A, VectorType &x, const VectorType &b, const PreconditionerType &prec) {
    typedef typename VectorType::value_type Number;
    const unsigned int N = b.size();
    VectorType r(N), r0(N), p(N), v(N), y(N), s(N), z(N), t(N);
    x = Number(0);
    r.equ(1, b);
    r0.equ(1, b);
    control.steps = 0;
    if (r.l2_norm() <= control.tolerance) return;
    Number rho = 1, alpha = 1, omega = 1;
    for (unsigned int it = 1; it <= control.max_steps; ++it) {
      const Number rho_new = r0 * r;
      const Number beta = (rho_new / rho) * (alpha / omega);
      rho = rho_new;
      p.add(-omega, v);  // p = r + beta (p - omega v)
      p.sadd(beta, 1, r);
      prec.vmult(y, p);
      A.vmult(v, y);
      alpha = rho / (r0 * v);
      s.equ(1, r);
      s.add(-alpha, v);
      control.steps = it;
      if (s.l2_norm() <= control.tolerance) {
        x.add(alpha, y);
        return;
      }
      prec.vmult(z, s);
      A.vmult(t, z);
      omega = (t * s) / (t * t);
      x.add(alpha, y);
      x.add(omega, z);
      r.equ(1, s);
      r.add(-omega, t);
      if (r.l2_norm() <= control.tolerance) return;
    }
    throw std::runtime_error("SolverBicgstab: no convergence in " + std::to_string(control.max_steps) + " steps");
  }

private:
  SolverControl &control;
};

// The same solver with its loop on the device (mfgpu_bicgstab, include/mfgpu.h), as SolverCGDevice is to SolverCG: the
// scalars stay in a device state block, the host reads them once every check_every iterations.  A matrix with get_qop()
// (QpOperatorGpu) is applied inside the library, any other through its vmult; DiagonalMatrix maps to MFGPU_CG_JACOBI,
// MultigridPreconditionerDevice to mfgpu_bicgstab_set_vcycle, anything else with a vmult(z, r) is called back twice per
// iteration.
template <typename VectorType>
class SolverBicgstabDevice {
public:
  typedef typename VectorType::value_type Number;
  explicit SolverBicgstabDevice(SolverControl &control, unsigned int check_every = 10)
      : control(control), check_every(check_every) {}
  template <typename MatrixType>
  void solve(const MatrixType &A, VectorType &x, const VectorType &b, const DiagonalMatrix<Number> &prec) {
    Run run(b.size(), MFGPU_CG_JACOBI, prec.get_vector().getDataRO());
    Callback<MatrixType> op{&A, b.size(), &run.error};
    set_operator(run, A, op, 0);
    finish(run, x, b);
  }
  template <typename MatrixType, int dim, typename LevelMatrixType, typename LevelNumber, typename CoarseSolver>
  void solve(const MatrixType &A, VectorType &x, const VectorType &b,
             const MultigridPreconditionerDevice<dim, LevelMatrixType, LevelNumber, CoarseSolver, Number> &prec) {
    Run run(b.size(), MFGPU_CG_CALLBACK, nullptr);
    Callback<MatrixType> op{&A, b.size(), &run.error};
    set_operator(run, A, op, 0);
    check(mfgpu_bicgstab_set_vcycle(run.s, prec.get_vcycle()), "SolverBicgstabDevice");
    finish(run, x, b);
  }
  template <typename MatrixType, typename PreconditionerType>
  void solve(const MatrixType &A, VectorType &x, const VectorType &b, const PreconditionerType &prec) {
    Run run(b.size(), MFGPU_CG_CALLBACK, nullptr);
    Callback<MatrixType> op{&A, b.size(), &run.error};
    Callback<PreconditionerType> pc{&prec, b.size(), &run.error};
    set_operator(run, A, op, 0);
    check(mfgpu_bicgstab_set_callback(run.s, &Callback<PreconditionerType>::call, &pc), "SolverBicgstabDevice");
    finish(run, x, b);
  }

private:
  // the solver object of one solve, destroyed with it
  struct Run {
    mfgpu_bicgstab *s = nullptr;
    std::string error;  // of a callback: no exception crosses the C-ABI
    Run(unsigned int n, int preconditioner, const void *inv_diag) {
      check(mfgpu_bicgstab_create(n, number_type<Number>(), preconditioner, inv_diag, &s), "SolverBicgstabDevice");
    }
    ~Run() { mfgpu_bicgstab_destroy(s); }
    Run(const Run &) = delete;
    Run &operator=(const Run &) = delete;
  };
  // dst = object.vmult(src) on the solver's vectors: the operator, or z = prec^-1 r
  template <typename ObjectType>
  struct Callback {
    const ObjectType *object;
    unsigned int n;
    std::string *error;
    static int call(void *ctx, void *dst_dev, const void *src_dev, void *) {
      Callback *self = static_cast<Callback *>(ctx);
      try {
        VectorType dst(dst_dev, self->n, typename VectorType::borrowed_t()),
            src(const_cast<void *>(src_dev), self->n, typename VectorType::borrowed_t());
        self->object->vmult(dst, src);
        return 0;
      } catch (std::exception &e) {
        *self->error = e.what();
        return MFGPU_EHIP;
      }
    }
  };
  template <typename MatrixType>
  static auto set_operator(Run &run, const MatrixType &A, Callback<MatrixType> &, int) -> decltype(A.get_qop(), void()) {
    check(mfgpu_bicgstab_set_operator_qop(run.s, A.get_qop(), 0), "SolverBicgstabDevice");
  }
  template <typename MatrixType>
  static void set_operator(Run &run, const MatrixType &, Callback<MatrixType> &op, long) {
    check(mfgpu_bicgstab_set_operator(run.s, &Callback<MatrixType>::call, &op), "SolverBicgstabDevice");
  }
  void finish(Run &run, VectorType &x, const VectorType &b) {
    if (x.size() != b.size()) x.reinit(b.size());
    mfgpu_cg_info info{};
    const int rc = mfgpu_bicgstab_solve(run.s, x.getData(), b.getDataRO(), control.tolerance, control.max_steps,
                                        check_every, nullptr, &info);
    if (rc != 0 && !run.error.empty()) throw std::runtime_error("SolverBicgstabDevice: " + run.error);
    check(rc, "SolverBicgstabDevice");
    control.steps = info.iterations;
    if (info.status == 2)
      throw std::runtime_error("SolverBicgstab: no convergence in " + std::to_string(control.max_steps) + " steps");
    if (info.status == 3) throw std::runtime_error("SolverBicgstab: breakdown, r0.v, t.t or rho is zero or not finite");
  }
  SolverControl &control;
  unsigned int check_every;
};

}  // namespace mfgpu_shim
#endif
