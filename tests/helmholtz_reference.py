"""numpy restatement of the Helmholtz operator A = sum_cells P^T C^T (K_cell + M_cell) C P (checker for the mass term,
mfgpu_desc.mass_coefficient; small meshes only).

  M_cell[i][j] = sum_q phi_i(x_q) phi_j(x_q) c_q JxW_q

Built from oracle.mf_oracle (cell_apply, assemble's element loop, hn_resolve, hn_cell_matrix) and
tests/poisson_reference.Cells, which stay as they are; `c` is always [n_cells, nd] at the quadrature points."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import poisson_reference as pr
from oracle import mf_oracle as o


def phi_table(od: o.Desc):
    """Phi[q, i] = phi_i(x_q), q and i lexicographic (x fastest): as poisson_reference.Cells.Phi"""
    n = od.n
    return pr._kron_tables([od.shape_values.reshape(n, n).astype(np.float64).T] * od.dim)


def _mass_weight(od, c):
    return np.asarray(c, np.float64).reshape(od.n_cells, od.nd) * od.JxW.astype(np.float64)


def assemble(od: o.Desc, c) -> sp.csr_matrix:
    """oracle.mf_oracle.assemble's element loop with K + Phi^T diag(c JxW) Phi"""
    dim, nd = od.dim, od.nd
    Gt, Phi, m = o._dense_grad_tables(od), phi_table(od), _mass_weight(od, c)
    rows, cols, vals = [], [], []
    for cell in range(od.n_cells):
        a = od.coefficient[cell].astype(np.float64) * od.JxW[cell].astype(np.float64)
        if od.uniform_j0:
            j0 = float(od.inv_jac[cell])
            K = sum(Gt[d].T @ (a[:, None] * j0 * j0 * Gt[d]) for d in range(dim))
        else:
            J = od.inv_jac[cell].astype(np.float64)
            P = [sum(J[:, d2, d1][:, None] * Gt[d2] for d2 in range(dim)) for d1 in range(dim)]
            K = sum(P[d].T @ (a[:, None] * P[d]) for d in range(dim))
        K = K + Phi.T @ (m[cell][:, None] * Phi)
        C = o.hn_cell_matrix(od, cell)
        if C is not None:
            K = C.T @ K @ C
        idx = od.loc2glob[cell].astype(np.int64)
        rows.append(np.repeat(idx, nd))
        cols.append(np.tile(idx, nd))
        vals.append(K.reshape(-1))
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(od.n_dofs, od.n_dofs)).tocsr()
    free = np.ones(od.n_dofs)
    free[od.constrained] = 0.0
    D = sp.diags(free)
    return (D @ A @ D + sp.diags(1.0 - free)).tocsr()


def _hn(od, v, transpose):
    """hn_resolve on every masked cell of v [cell, nd] (a copy)"""
    v = np.array(v, dtype=np.float64)
    if od.constraint_mask is not None:
        for cell in np.nonzero(od.constraint_mask)[0]:
            v[cell] = o.hn_resolve(v[cell].reshape((od.n,) * od.dim), int(od.constraint_mask[cell]), od.dim, od.degree,
                                   od.weights, transpose).reshape(-1)
    return v


def mass_cell_apply(od: o.Desc, c, u_loc):
    """sum-factorised C^T S^T (c JxW .* S C u) on gathered local values u_loc [cell, nd]"""
    dim, n = od.dim, od.n
    S = od.shape_values.reshape(n, n).astype(np.float64)  # S[i, q]
    t = _hn(od, u_loc, False).reshape((od.n_cells,) + (n,) * dim)
    for r in range(dim):
        t = o._contract(t, S.T.copy(), r)
    t = t * _mass_weight(od, c).reshape(t.shape)
    for r in range(dim):
        t = o._contract(t, S, r)
    return _hn(od, t.reshape(od.n_cells, od.nd), True)


def vmult_add(od: o.Desc, c, dst, src):
    """o.vmult_add with the mass term in the cell kernel (constrained rows: dst_c += src_c)"""
    dst = np.array(dst, dtype=np.float64)
    s = np.array(src, dtype=np.float64)
    con = od.constrained
    tmp = dst[con] + s[con]
    s[con] = 0
    loc = o.cell_apply(od, s[od.loc2glob]).astype(np.float64) + mass_cell_apply(od, c, s[od.loc2glob])
    np.add.at(dst, od.loc2glob.reshape(-1), loc.reshape(-1))
    dst[con] = tmp
    return dst


def vmult(od: o.Desc, c, src):
    return vmult_add(od, c, np.zeros(od.n_dofs), src)


def local_diagonal(od: o.Desc, c):
    """K_ii + M_ii per cell, M_ii = sum_q c_q JxW_q phi_i(x_q)^2 (dense table)"""
    Phi = phi_table(od)
    return o.local_diagonal(od) + _mass_weight(od, c) @ (Phi * Phi)


def inverse_diagonal(od: o.Desc, c):
    """o.compute_inverse_diagonal with the Helmholtz local diagonal"""
    loc = _hn(od, local_diagonal(od, c), True)
    diag = np.zeros(od.n_dofs)
    np.add.at(diag, od.loc2glob.reshape(-1), loc.reshape(-1))
    diag[od.constrained] = 1.0
    return 1.0 / diag


def rhs(cells: "pr.Cells", c, f_qp=None, u_b=None):
    """poisson_reference.Cells.rhs with the lift - int a grad phi_i . grad u_b - int c phi_i u_b"""
    od = cells.od
    out = cells.rhs(f_qp, u_b)
    if u_b is not None:
        ub = np.asarray(u_b, np.float64)
        uq = _hn(od, ub[od.loc2glob], False) @ cells.Phi.T        # [cell, q]
        loc = _hn(od, (_mass_weight(od, c) * uq) @ cells.Phi, True)
        lift = np.zeros(od.n_dofs)
        np.add.at(lift, od.loc2glob.reshape(-1), loc.reshape(-1))
        lift[od.constrained] = 0.0
        out = out - lift
    return out


def vmult_interface_down(od: o.Desc, c, edge_dofs, src):
    """o.vmult_interface_down on the unconstrained Helmholtz operator"""
    e = np.asarray(edge_dofs, dtype=np.int64)
    s = np.array(src, dtype=np.float64)
    s[od.constrained] = 0.0
    s[e] = 0.0
    tmp = vmult(o._unconstrained(od), c, s)
    dst = np.zeros(od.n_dofs)
    dst[e] = tmp[e]
    return dst


def vmult_interface_up(od: o.Desc, c, edge_dofs, src):
    e = np.asarray(edge_dofs, dtype=np.int64)
    s = np.zeros(od.n_dofs)
    s[e] = np.asarray(src, dtype=np.float64)[e]
    dst = vmult(o._unconstrained(od), c, s)
    dst[od.constrained] = 0.0
    dst[e] = 0.0
    return dst


# ---- the driver's problem: -div(a grad u) + c u = f, c = 1 + |x|^2, u = Solution<dim>


def mass_function(x):
    return 1.0 + np.sum(x * x, axis=-1)


def load(x):
    """f = RightHandSide + c * Solution"""
    return pr.right_hand_side(x) + mass_function(x) * pr.solution(x)


def solve(cells: "pr.Cells"):
    """CPU Helmholtz solve on the assembled operator: (u, l2 error)"""
    c = mass_function(cells.qpts)
    ub = cells.lift()
    b = rhs(cells, c, load(cells.qpts), ub)
    x = spla.spsolve(assemble(cells.od, c).tocsc(), b)
    u = ub + x
    return u, cells.l2_error(u)[0]


def known_answer_vector(dof_coords, constrained):
    """u = prod_d (1 - x_d^2) at the support points, 0 on the constrained dofs: with coefficient = 0 and c = 1 on a mesh
    of [-1,1]^dim, u^T A u = int u^2 = (16/15)^dim (QGauss(p+1) integrates degree 4 per direction exactly for p >= 2)"""
    u = np.prod(1.0 - dof_coords ** 2, axis=1)
    u[np.asarray(constrained, dtype=np.int64)] = 0.0
    return u
