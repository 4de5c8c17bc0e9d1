// Poisson side of the shim: what poisson.cu needs around the operator besides vmult and the inverse diagonal.
//   Solution<dim>                          poisson_common.cc:5-175 (three Gaussians; value, gradient, laplacian)
//   VectorTools::interpolate_boundary_values   Solution at the support points of the constrained dofs
//                                          (mfgpu_mesh_dof_coords; poisson.cu:157-160)
//   VectorTools::create_right_hand_side    the load vector with the Dirichlet lift (poisson.cu:182-221) on the device
//   VectorTools::integrate_difference      L2 error on QGauss(p+2) (poisson.cu:277-292) on the device
//   SolverControl / SolverCG               deal.II's, in the shape poisson.cu:246-251 uses them
// The two integrals go through mfgpu_integrator (include/mfgpu.h); double only.
#ifndef MFGPU_SHIM_POISSON_H
#define MFGPU_SHIM_POISSON_H

#include <cmath>

#include "mfgpu_shim_mg.h"

namespace mfgpu_shim {

template <int dim>
class Solution {
public:
  static constexpr double width = 1. / 3.;
  static const double *center(unsigned int i) {
    static const double c2[3][2] = {{-0.5, +0.5}, {-0.5, -0.5}, {+0.5, -0.5}};
    static const double c3[3][3] = {{-0.5, +0.5, 0.25}, {-0.6, -0.5, -0.125}, {+0.5, -0.5, 0.5}};
    return dim == 2 ? c2[i] : c3[i];
  }
  static double norm() { return std::pow(std::sqrt(2 * M_PI) * width, dim); }
  double value(const double *p) const {
    double r = 0;
    for (unsigned int i = 0; i < 3; ++i) r += std::exp(-dist2(p, i) / (width * width));
    return r / norm();
  }
  void gradient(const double *p, double *g) const {
    for (int d = 0; d < dim; ++d) g[d] = 0;
    for (unsigned int i = 0; i < 3; ++i) {
      const double e = -2 / (width * width) * std::exp(-dist2(p, i) / (width * width));
      for (int d = 0; d < dim; ++d) g[d] += e * (p[d] - center(i)[d]);
    }
    for (int d = 0; d < dim; ++d) g[d] /= norm();
  }
  double laplacian(const double *p) const {
    double r = 0;
    for (unsigned int i = 0; i < 3; ++i) {
      const double r2 = dist2(p, i);
      r += (-2 * dim + 4 * r2 / (width * width)) / (width * width) * std::exp(-r2 / (width * width));
    }
    return r / norm();
  }

private:
  static double dist2(const double *p, unsigned int i) {
    double s = 0;
    for (int d = 0; d < dim; ++d) s += (p[d] - center(i)[d]) * (p[d] - center(i)[d]);
    return s;
  }
};

// the device object behind create_right_hand_side / integrate_difference, built from the DoFHandler's description
template <int dim>
class PoissonIntegrator {
public:
  explicit PoissonIntegrator(const DoFHandler<dim> &dof_handler) {
    check(mfgpu_integrator_create(&dof_handler.desc, &it), "mfgpu_integrator_create");
  }
  // ... with a mass term: mass_coefficient = c at the quadrature points [n_cells * (p+1)^dim] (mfgpu_desc.mass_coefficient);
  // the lift of create_right_hand_side then also subtracts int c phi_i u_b
  PoissonIntegrator(const DoFHandler<dim> &dof_handler, const double *mass_coefficient) {
    mfgpu_desc d = dof_handler.desc;
    d.mass_coefficient = mass_coefficient;
    check(mfgpu_integrator_create(&d, &it), "mfgpu_integrator_create");
  }
  // ... from a description the caller has adjusted (flags, coefficient, mass_coefficient)
  explicit PoissonIntegrator(const mfgpu_desc &d) { check(mfgpu_integrator_create(&d, &it), "mfgpu_integrator_create"); }
  ~PoissonIntegrator() { mfgpu_integrator_destroy(it); }
  PoissonIntegrator(const PoissonIntegrator &) = delete;
  PoissonIntegrator &operator=(const PoissonIntegrator &) = delete;
  mfgpu_integrator *it = nullptr;
};

namespace VectorTools {
// boundary_values of poisson.cu:157-160 written into `values` (host, n_dofs): Solution at the support points of every
// constrained dof (Dirichlet and hanging -- the hanging ones are never read, their values come by interpolation)
template <int dim>
void interpolate_boundary_values(const DoFHandler<dim> &dof_handler, const Solution<dim> &f, std::vector<double> &values) {
  const double *xy = nullptr;
  check(mfgpu_mesh_dof_coords(dof_handler.mesh, &xy) < 0 ? -1 : 0, "mfgpu_mesh_dof_coords");
  values.resize(dof_handler.n_dofs());
  const mfgpu_desc &d = dof_handler.desc;
  for (uint32_t i = 0; i < d.n_constrained; ++i) values[d.constrained_dofs[i]] = f.value(xy + (size_t)d.constrained_dofs[i] * dim);
}
// rhs = int phi_i f - int grad phi_i . a grad lift, f = RightHandSide<dim> (poisson.cu:182-221); constrained rows 0
template <int dim>
void create_right_hand_side(PoissonIntegrator<dim> &integrator, GpuVector<double> &rhs, const GpuVector<double> *lift) {
  check(mfgpu_integrator_rhs(integrator.it, rhs.getData(), nullptr, lift ? lift->getDataRO() : nullptr, nullptr),
        "create_right_hand_side");
}
// || u - Solution ||_L2 on QGauss(p+2) (VectorTools::integrate_difference with L2_norm); per_cell: squared cell errors
template <int dim>
double integrate_difference(PoissonIntegrator<dim> &integrator, const GpuVector<double> &u,
                            GpuVector<double> *per_cell = nullptr) {
  double l2 = 0;
  check(mfgpu_integrator_l2_error(integrator.it, u.getDataRO(), nullptr, per_cell ? per_cell->getData() : nullptr,
                                  nullptr, &l2),
        "integrate_difference");
  return l2;
}
}  // namespace VectorTools

class SolverControl {
public:
  SolverControl(unsigned int max_steps, double tolerance) : max_steps(max_steps), tolerance(tolerance) {}
  unsigned int last_step() const { return steps; }
  unsigned int max_steps;
  double tolerance;
  unsigned int steps = 0;
};

// preconditioned conjugate gradients, zero start as poisson.cu:253-254 calls it (solution_update is zero)
template <typename VectorType>
class SolverCG {
public:
  explicit SolverCG(SolverControl &control) : control(control) {}
  template <typename MatrixType, typename PreconditionerType>
  void solve(const MatrixType &A, VectorType &x, const VectorType &b, const PreconditionerType &prec) {
    typedef typename VectorType::value_type Number;
    const unsigned int N = b.size();
    VectorType r(N), z(N), p(N), q(N);
    x = Number(0);
    r.equ(1, b);
    control.steps = 0;
    if (r.l2_norm() <= control.tolerance) return;
    prec.vmult(z, r);
    p.equ(1, z);
    Number rz = r * z;
    for (unsigned int it = 1; it <= control.max_steps; ++it) {
      A.vmult(q, p);
      const Number alpha = rz / (p * q);
      x.add(alpha, p);
      r.add(-alpha, q);
      control.steps = it;
      if (r.l2_norm() <= control.tolerance) return;
      prec.vmult(z, r);
      const Number rz_new = r * z;
      p.sadd(rz_new / rz, 1, z);
      rz = rz_new;
    }
    throw std::runtime_error("SolverCG: no convergence in " + std::to_string(control.max_steps) + " steps");
  }

private:
  SolverControl &control;
};

// The same solver with its loop on the device (mfgpu_cg, include/mfgpu.h): the scalars stay in a device state block, the
// host reads them once every check_every iterations.  PreconditionChebyshev maps to MFGPU_CG_CHEBYSHEV (its sweep, from
// its lambda_max, degree and smoothing range; A must be the matrix it was initialised with), DiagonalMatrix to
// MFGPU_CG_JACOBI, MultigridPreconditionerDevice to mfgpu_cg_set_vcycle, anything else with a vmult(z, r) is called back
// once per iteration (a V-cycle composed in the shim).  A must give its mfgpu_handle (get_handle()).
template <typename VectorType>
class SolverCGDevice {
public:
  typedef typename VectorType::value_type Number;
  explicit SolverCGDevice(SolverControl &control, unsigned int check_every = 10) : control(control), check_every(check_every) {}
  template <typename MatrixType, typename ChebyshevMatrixType>
  void solve(const MatrixType &A, VectorType &x, const VectorType &b,
             const PreconditionChebyshev<ChebyshevMatrixType, VectorType> &prec) {
    const auto &d = prec.get_additional_data();
    mfgpu_cg *cg = nullptr;
    check(mfgpu_cg_create(A.get_handle(), MFGPU_CG_CHEBYSHEV, d.preconditioner->get_vector().getDataRO(), d.degree,
                          prec.lambda_max, d.smoothing_range, &cg), "SolverCGDevice");
    run(cg, x, b);
  }
  template <typename MatrixType>
  void solve(const MatrixType &A, VectorType &x, const VectorType &b, const DiagonalMatrix<Number> &prec) {
    mfgpu_cg *cg = nullptr;
    check(mfgpu_cg_create(A.get_handle(), MFGPU_CG_JACOBI, prec.get_vector().getDataRO(), 0, 0, 0, &cg), "SolverCGDevice");
    run(cg, x, b);
  }
  // the library's V-cycle object: its own callback inside the library, no trip through the shim per iteration
  template <typename MatrixType, int dim, typename LevelMatrixType, typename LevelNumber, typename CoarseSolver>
  void solve(const MatrixType &A, VectorType &x, const VectorType &b,
             const MultigridPreconditionerDevice<dim, LevelMatrixType, LevelNumber, CoarseSolver, Number> &prec) {
    mfgpu_cg *cg = nullptr;
    check(mfgpu_cg_create(A.get_handle(), MFGPU_CG_CALLBACK, nullptr, 0, 0, 0, &cg), "SolverCGDevice");
    const int rc = mfgpu_cg_set_vcycle(cg, prec.get_vcycle());
    if (rc != 0) {
      mfgpu_cg_destroy(cg);
      check(rc, "SolverCGDevice");
    }
    run(cg, x, b);
  }
  template <typename MatrixType, typename PreconditionerType>
  void solve(const MatrixType &A, VectorType &x, const VectorType &b, const PreconditionerType &prec) {
    mfgpu_cg *cg = nullptr;
    check(mfgpu_cg_create(A.get_handle(), MFGPU_CG_CALLBACK, nullptr, 0, 0, 0, &cg), "SolverCGDevice");
    Callback<PreconditionerType> ctx{&prec, b.size(), std::string()};
    const int rc = mfgpu_cg_set_callback(cg, &Callback<PreconditionerType>::call, &ctx);
    if (rc != 0) {
      mfgpu_cg_destroy(cg);
      check(rc, "SolverCGDevice");
    }
    run(cg, x, b, &ctx.error);
  }

private:
  // z = prec^-1 r on the solver's vectors; no exception crosses the C-ABI
  template <typename PreconditionerType>
  struct Callback {
    const PreconditionerType *prec;
    unsigned int n;
    std::string error;
    static int call(void *ctx, void *z_dev, const void *r_dev, void *) {
      Callback *self = static_cast<Callback *>(ctx);
      try {
        VectorType z(z_dev, self->n, typename VectorType::borrowed_t()),
            r(const_cast<void *>(r_dev), self->n, typename VectorType::borrowed_t());
        self->prec->vmult(z, r);
        return 0;
      } catch (std::exception &e) {
        self->error = e.what();
        return MFGPU_EHIP;
      }
    }
  };
  void run(mfgpu_cg *cg, VectorType &x, const VectorType &b, const std::string *callback_error = nullptr) {
    if (x.size() != b.size()) x.reinit(b.size());
    mfgpu_cg_info info{};
    const int rc = mfgpu_cg_solve(cg, x.getData(), b.getDataRO(), control.tolerance, control.max_steps, check_every,
                                  nullptr, &info);
    mfgpu_cg_destroy(cg);
    if (rc != 0 && callback_error && !callback_error->empty()) throw std::runtime_error("SolverCGDevice: " + *callback_error);
    check(rc, "SolverCGDevice");
    control.steps = info.iterations;
    if (info.status == 2) throw std::runtime_error("SolverCG: no convergence in " + std::to_string(control.max_steps) + " steps");
    if (info.status == 3) throw std::runtime_error("SolverCG: breakdown, p.Ap is not a positive finite number");
  }
  SolverControl &control;
  unsigned int check_every;
};

}  // namespace mfgpu_shim
#endif
