"""numpy restatement of the two cell integrals of a Poisson solve (checker for mfgpu_integrator, small meshes only).

  rhs_i = sum_cells int phi_i f - int grad phi_i . a grad u_b      poisson.cu:182-221 (QGauss(p+1))
  |u - u*|_L2 on QGauss(p+2)                                       poisson.cu:277-292 (integrate_difference)

Built from the stand-in mesh arrays and oracle.mf_oracle (dense per-cell tables, hn_resolve, assemble).  The analytic
solution is Solution<dim> of poisson_common.cc:5-175 (three Gaussians), the load RightHandSide<dim> of
poisson_common.h:277-296 with the coefficient 1 / (0.05 + 2 |x|^2)."""
import numpy as np
import scipy.sparse.linalg as spla

import pymfgpu as mf
from oracle import mf_oracle as o

WIDTH = 1.0 / 3.0
CENTERS = {2: np.array([[-0.5, 0.5], [-0.5, -0.5], [0.5, -0.5]]),
           3: np.array([[-0.5, 0.5, 0.25], [-0.6, -0.5, -0.125], [0.5, -0.5, 0.5]])}


def _norm(dim):
    return (np.sqrt(2 * np.pi) * WIDTH) ** dim


def solution(x):
    """Solution<dim>::value, x[..., dim]"""
    dim = x.shape[-1]
    r = sum(np.exp(-np.sum((x - c) ** 2, axis=-1) / WIDTH ** 2) for c in CENTERS[dim])
    return r / _norm(dim)


def solution_gradient(x):
    dim = x.shape[-1]
    g = sum(-2 / WIDTH ** 2 * np.exp(-np.sum((x - c) ** 2, axis=-1) / WIDTH ** 2)[..., None] * (x - c)
            for c in CENTERS[dim])
    return g / _norm(dim)


def solution_laplacian(x):
    dim = x.shape[-1]
    lap = 0.0
    for c in CENTERS[dim]:
        r2 = np.sum((x - c) ** 2, axis=-1)
        lap = lap + (-2 * dim + 4 * r2 / WIDTH ** 2) / WIDTH ** 2 * np.exp(-r2 / WIDTH ** 2)
    return lap / _norm(dim)


def right_hand_side(x):
    """RightHandSide<dim>::value = -(lap u a + grad a . grad u)"""
    xx = np.sum(x * x, axis=-1)
    a = 1.0 / (0.05 + 2.0 * xx)
    grad_a = (4.0 / (0.05 + 2.0 * xx) ** 2)[..., None] * (-x)
    return -(solution_laplacian(x) * a + np.sum(grad_a * solution_gradient(x), axis=-1))


def _kron_tables(tabs):
    """dense [k, i] of a tensor product of 1D tables tabs[d][k_d, i_d], x fastest"""
    M = np.ones((1, 1))
    for T in tabs:
        M = np.kron(T, M)
    return M


class Cells:
    """per-cell data of a stand-in mesh: oracle description, quadrature points, error-point geometry"""

    def __init__(self, mesh: "mf.Mesh"):
        from util import oracle_desc_from_mesh
        self.mesh = mesh  # the description arrays are views into the mesh
        a = mesh.arrays()
        self.od = od = oracle_desc_from_mesh(mesh, dtype=np.float64)
        self.dim, self.p = od.dim, od.degree
        self.qpts = a["quadrature_points"].astype(np.float64).copy()  # [cell, q, dim]
        self.dof_coords = mesh.dof_coords().copy()
        dim, n, m = od.dim, od.n, od.n + 1
        sv, _, xq, _, nodes = o.shape_info(self.p)
        self.ym, wm = o.gauss_01(m)
        E1 = o.lagrange_eval(nodes, self.ym)[0].T          # [k, i] FE_Q shape functions at the error points
        Lv1, Ld1 = (t.T for t in o.lagrange_eval(xq, self.ym))  # Lagrange basis on the QGauss(p+1) points
        self.E = _kron_tables([E1] * dim)
        self.wm = _kron_tables([wm[:, None]] * dim)[:, 0]
        # x and dx/dxi at the error points from the quadrature points (exact for mappings of degree <= p)
        self.xe = np.einsum("ki,cid->ckd", _kron_tables([Lv1] * dim), self.qpts)
        J = np.stack([np.einsum("ki,cid->ckd", _kron_tables([Ld1 if r == e else Lv1 for r in range(dim)]), self.qpts)
                      for e in range(dim)], axis=-1)  # [cell, k, d, e] = dx_d / dxi_e
        self.jxw_e = self.wm[None, :] * np.abs(np.linalg.det(J))
        self.Phi = _kron_tables([sv.reshape(n, n).T] * dim)  # [q, i]
        self.Gt = o._dense_grad_tables(od)                   # [d][q, i]

    def _hn(self, c, v, transpose):
        od = self.od
        if od.constraint_mask is None or od.constraint_mask[c] == 0:
            return v
        return o.hn_resolve(v.reshape((od.n,) * od.dim), int(od.constraint_mask[c]), od.dim, od.degree, od.weights,
                            transpose).reshape(-1)

    def rhs(self, f_qp=None, u_b=None):
        """f_qp [cell, q] or None = right_hand_side at the quadrature points; u_b [n_dofs] or None"""
        od, dim = self.od, self.dim
        f = right_hand_side(self.qpts) if f_qp is None else np.asarray(f_qp, np.float64).reshape(od.n_cells, od.nd)
        loc = (f * od.JxW) @ self.Phi                        # [cell, i]
        if u_b is not None:
            a = od.coefficient * od.JxW
            for c in range(od.n_cells):
                uc = self._hn(c, np.asarray(u_b, np.float64)[od.loc2glob[c]], False)
                g = np.stack([G @ uc for G in self.Gt])      # [e, q] reference gradients
                if od.uniform_j0:
                    fl = a[c] * od.inv_jac[c] ** 2 * g
                else:
                    Ji = od.inv_jac[c]                       # [q, d1, d2]
                    Mq = np.einsum("qak,qbk->qab", Ji, Ji) * a[c][:, None, None]
                    fl = np.einsum("qab,bq->aq", Mq, g)
                loc[c] -= sum(self.Gt[e].T @ fl[e] for e in range(dim))
        out = np.zeros(od.n_dofs)
        for c in range(od.n_cells):
            np.add.at(out, od.loc2glob[c], self._hn(c, loc[c], True))
        out[od.constrained] = 0.0
        return out

    def l2_error(self, u, exact=None):
        """(l2, per-cell squared errors); exact [cell, k] or None = solution at the error points"""
        od = self.od
        ue = np.stack([self.E @ self._hn(c, np.asarray(u, np.float64)[od.loc2glob[c]], False)
                       for c in range(od.n_cells)])
        ex = solution(self.xe) if exact is None else np.asarray(exact, np.float64).reshape(ue.shape)
        per = np.sum((ue - ex) ** 2 * self.jxw_e, axis=1)
        return np.sqrt(per.sum()), per

    def interpolant(self, fun=solution):
        return fun(self.dof_coords)

    def lift(self):
        """u_b: Solution on the constrained dofs, 0 elsewhere"""
        ub = np.zeros(self.od.n_dofs)
        c = self.od.constrained
        ub[c] = solution(self.dof_coords[c])
        return ub

    def solve(self):
        """CPU Poisson solve: A x = rhs(f, lift) on the oracle's assembled operator, u = u_b + x; returns (u, l2)"""
        ub = self.lift()
        b = self.rhs(None, ub)
        x = spla.spsolve(o.assemble(self.od).tocsc(), b)
        u = ub + x
        return u, self.l2_error(u)[0]


def refined_leaves(leaves, dim, r):
    """every octree leaf (level, cx, cy, cz) split r times: h halves, the hanging structure is kept"""
    out = []
    k = 1 << r
    for lv, cx, cy, cz in np.asarray(leaves, dtype=np.int64):
        for m in range(k if dim == 3 else 1):
            for j in range(k):
                for i in range(k):
                    out.append((lv + r, cx * k + i, cy * k + j, cz * k + m if dim == 3 else 0))
    return np.array(out, dtype=np.uint32)


def family(kind, dim, p, level):
    """the three mesh families of the convergence tests, level = 0, 1, 2 (h halves per level)"""
    if kind == "cube":
        return mf.Mesh.uniform(dim, p, 4 << level)
    if kind == "hanging":
        # the pseudo-adaptive recipe has its first hanging nodes at n_ref = 3 (2D) / 4 (3D)
        leaves = mf.Mesh.adaptive(dim, p, 3 if dim == 2 else 4).cell_levels()
        return mf.Mesh.from_leaves(dim, p, refined_leaves(leaves, dim, level))
    if kind == "ball":
        return mf.Mesh.ball(dim, p, level + 1)
    raise ValueError(kind)


def orders(errors):
    e = np.asarray(errors)
    return np.log2(e[:-1] / e[1:])
