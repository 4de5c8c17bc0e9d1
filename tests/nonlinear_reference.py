"""numpy reference for the device-side coefficient loop (checker for mfgpu_integrator_evaluate and the update calls; small
meshes only), built on poisson_reference.Cells:

  evaluate(cells, u)   u and its real-space gradient at the quadrature points (hanging-node interpolated nodal values,
                       dense tables, grad_x = J^-T grad_xi)
  picard(cells, ...)   Picard iteration for -div((1 + u^2) grad u) = f with u* = Solution<dim>, boundary values u*:
                       a_k = 1 + u_k^2 at the quadrature points, solve the linear problem with a_k for u_{k+1}"""
import copy

import numpy as np
import scipy.sparse.linalg as spla

import poisson_reference as pr
from oracle import mf_oracle as o


def evaluate(cells: "pr.Cells", u):
    """(values [cell, q], gradients [cell, q, dim]) of the field with dof vector u, read on every dof a cell references"""
    od, dim = cells.od, cells.dim
    u = np.asarray(u, np.float64)
    vals = np.zeros((od.n_cells, od.nd))
    grads = np.zeros((od.n_cells, od.nd, dim))
    for c in range(od.n_cells):
        uc = cells._hn(c, u[od.loc2glob[c]], False)
        vals[c] = cells.Phi @ uc
        g = np.stack([G @ uc for G in cells.Gt])              # [e, q] reference gradients
        if od.uniform_j0:
            grads[c] = (float(od.inv_jac[c]) * g).T
        else:
            grads[c] = np.einsum("qek,eq->qk", od.inv_jac[c].astype(np.float64), g)  # J^-1[e][k] = dxi_e / dx_k
    return vals, grads


def coefficient(u_qp):
    return 1.0 + u_qp ** 2


def load(x):
    """f = -div((1 + u*^2) grad u*) = -(1 + u*^2) lap u* - 2 u* |grad u*|^2"""
    u, g = pr.solution(x), pr.solution_gradient(x)
    return -(1.0 + u * u) * pr.solution_laplacian(x) - 2.0 * u * np.sum(g * g, axis=-1)


def with_coefficient(cells: "pr.Cells", a):
    """a shallow copy of cells whose oracle description carries the coefficient a [cell, q]"""
    c = copy.copy(cells)
    c.od = copy.copy(cells.od)
    c.od.coefficient = np.ascontiguousarray(a, dtype=np.float64).reshape(c.od.n_cells, c.od.nd)
    return c


def direct_solve(A, b):
    return spla.spsolve(A.tocsc(), b)


def jacobi_pcg(A, b, rtol=1e-12):
    """the GPU tests' solver on the assembled operator: Jacobi-preconditioned CG, zero start, until |r| <= rtol |b|"""
    dinv = 1.0 / A.diagonal()
    x, r = np.zeros_like(b), b.copy()
    z = dinv * r
    p, rz, tol = z.copy(), r @ z, rtol * np.linalg.norm(b)
    for _ in range(20000):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        if np.linalg.norm(r) <= tol:
            return x
        z = dinv * r
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    raise RuntimeError("CG did not converge")


def picard(cells: "pr.Cells", steps=None, tol=1e-10, solve=direct_solve, max_steps=100):
    """u_0 = u* on the constrained dofs, 0 elsewhere.  `steps` fixed steps, or (steps=None) until
    |u_{k+1} - u_k| / |u_{k+1}| <= tol.  Returns (u, [relative update norms])"""
    ub = cells.lift()
    f = load(cells.qpts)
    u, hist = ub.copy(), []
    for _ in range(max_steps if steps is None else steps):
        ck = with_coefficient(cells, coefficient(evaluate(cells, u)[0]))
        x = solve(o.assemble(ck.od), ck.rhs(f, ub))
        u_new = ub + x
        hist.append(np.linalg.norm(u_new - u) / np.linalg.norm(u_new))
        u = u_new
        if steps is None and hist[-1] <= tol:
            break
    return u, hist
