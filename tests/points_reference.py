"""numpy restatement of evaluation and point sources at arbitrary points (checker for mfgpu_locate_points and
mfgpu_points_*; small meshes only), built on poisson_reference.Cells.

With N = p + 1, x_q the quadrature points of a cell (QGauss(N), x fastest) and L_q the tensor Lagrange basis on the 1D
Gauss abscissae:
  mapping    x(xi) = sum_q L_q(xi) x_q
  field      U_q = Phi H_c u[loc2glob[c]] (H_c: the cell's hanging-node resolution), u_h(xi) = sum_q L_q(xi) U_q
  gradient   grad_x u_h = J^-T grad_xi u_h, J = sum_q grad L_q(xi) x_q
Location is brute force over ALL cells (no bin grid): a cell is a candidate when the point lies in the box of the cell's
corners inflated by 1e-10 of its diagonal; Newton from the centre, at most 30 steps, converged at |delta xi|_inf <= 1e-14,
accepted when every xi_d is in [-1e-10, 1 + 1e-10], then clamped; the lowest accepting cell wins.  Everything uses dense 1D
Lagrange tables (oracle.mf_oracle.lagrange_eval); the transpose is the explicit dense matrix E [n_points, n_dofs]."""
import itertools

import numpy as np

import poisson_reference as pr
from oracle import mf_oracle as o

NOT_FOUND = 0xFFFFFFFF
NEWTON_STEPS, NEWTON_TOL, ACCEPT_TOL, BOX_INFLATION = 30, 1e-14, 1e-10, 1e-10


def tables(p, t):
    """(L [k, q], L' [k, q]) of the Lagrange basis on the QGauss(p+1) abscissae at the abscissae t [k]"""
    xq = o.gauss_01(p + 1)[0]
    v, d = o.lagrange_eval(xq, np.asarray(t, np.float64).reshape(-1))
    return v.T, d.T


def tensor_rows(p, xi, deriv=None):
    """[k, q] = prod_d (L or, for d == deriv, L')_{q_d}(xi[k, d]), q with x fastest"""
    xi = np.asarray(xi, np.float64)
    dim = xi.shape[1]
    t = [tables(p, xi[:, d]) for d in range(dim)]
    rows = np.ones((len(xi), 1))
    for d in range(dim):
        f = t[d][1 if d == deriv else 0]
        rows = (f[:, :, None] * rows[:, None, :]).reshape(len(xi), -1)
    return rows


def mapping(p, xq, xi):
    """x [k, dim] and J [k, d, e] = dx_d / dxi_e of the cell with quadrature points xq [q, dim] at xi [k, dim]"""
    dim = xq.shape[1]
    x = tensor_rows(p, xi) @ xq
    J = np.stack([tensor_rows(p, xi, e) @ xq for e in range(dim)], axis=-1)
    return x, J


def newton(p, xq, x):
    """(accepted [k], xi [k, dim]) of the points x [k, dim] in the cell with quadrature points xq"""
    dim = xq.shape[1]
    xi = np.full((len(x), dim), 0.5)
    alive = np.ones(len(x), bool)
    conv = np.zeros(len(x), bool)
    for _ in range(NEWTON_STEPS):
        idx = np.flatnonzero(alive & ~conv)
        if not len(idx):
            break
        # residual on the differences x_q - x (they sum to x(xi) - x because the L_q sum to 1): rounding relative to the cell
        F = np.einsum("kq,kqd->kd", tensor_rows(p, xi[idx]), xq[None, :, :] - x[idx, None, :])
        J = mapping(p, xq, xi[idx])[1]
        with np.errstate(all="ignore"):
            det = np.linalg.det(J)
            ok = np.isfinite(det) & (det != 0)
            delta = np.zeros_like(F)
            delta[ok] = -np.linalg.solve(J[ok], F[ok][:, :, None])[:, :, 0]
        ok &= np.all(np.isfinite(delta), axis=1)
        xi[idx[ok]] += delta[ok]
        ok &= np.all(np.abs(xi[idx] - 0.5) < 1e3, axis=1)
        alive[idx[~ok]] = False
        conv[idx[ok]] = np.max(np.abs(delta[ok]), axis=1) <= NEWTON_TOL
    acc = alive & conv & np.all((xi >= -ACCEPT_TOL) & (xi <= 1 + ACCEPT_TOL), axis=1)
    return acc, np.clip(xi, 0.0, 1.0)


def locate(cells: "pr.Cells", x):
    """(cell [n] uint32, xi [n, dim], n_not_found): brute force over all cells, the lowest accepting cell wins"""
    x = np.asarray(x, np.float64).reshape(-1, cells.dim)
    dim, p = cells.dim, cells.p
    cell = np.full(len(x), NOT_FOUND, np.uint32)
    xi = np.zeros((len(x), dim))
    corners = np.array(list(itertools.product((0.0, 1.0), repeat=dim)))[:, ::-1]
    for c in range(cells.od.n_cells):
        xc = mapping(p, cells.qpts[c], corners)[0]
        lo, hi = xc.min(axis=0), xc.max(axis=0)
        pad = BOX_INFLATION * np.linalg.norm(hi - lo)
        cand = np.flatnonzero((cell == NOT_FOUND) & np.all((x >= lo - pad) & (x <= hi + pad), axis=1))
        if not len(cand):
            continue
        acc, t = newton(p, cells.qpts[c], x[cand])
        cell[cand[acc]] = c
        xi[cand[acc]] = t[acc]
    return cell, xi, int(np.sum(cell == NOT_FOUND))


class PointsRef:
    """evaluation at points given as (cell, xi); cell NOT_FOUND gives 0 and contributes nothing"""

    def __init__(self, cells: "pr.Cells", cell, xi):
        self.cells = cells
        self.cell = np.asarray(cell, np.uint32).reshape(-1)
        self.xi = np.asarray(xi, np.float64).reshape(len(self.cell), cells.dim)
        self._H = {}

    def _nodal_to_gauss(self, c):
        """[q, i]: values at the cell's Gauss points from u[loc2glob[c]] (hanging-node resolution, then Phi)"""
        cells = self.cells
        m = 0 if cells.od.constraint_mask is None else int(cells.od.constraint_mask[c])
        if m not in self._H:
            nd = cells.od.nd
            self._H[m] = np.stack([cells._hn(c, e, False) for e in np.eye(nd)], axis=1) if m else np.eye(nd)
        return cells.Phi @ self._H[m]

    def matrix(self):
        """E [n_points, n_dofs]: values = E u"""
        od = self.cells.od
        E = np.zeros((len(self.cell), od.n_dofs))
        for c in np.unique(self.cell[self.cell != NOT_FOUND]):
            k = np.flatnonzero(self.cell == c)
            np.add.at(E, (k[:, None], od.loc2glob[c][None, :]),
                      tensor_rows(self.cells.p, self.xi[k]) @ self._nodal_to_gauss(c))
        return E

    def evaluate(self, u):
        """(values [n], gradients [n, dim]); u is read on the dofs a cell lists only"""
        cells, od, dim, p = self.cells, self.cells.od, self.cells.dim, self.cells.p
        u = np.asarray(u, np.float64)
        vals, grads = np.zeros(len(self.cell)), np.zeros((len(self.cell), dim))
        for c in np.unique(self.cell[self.cell != NOT_FOUND]):
            k = np.flatnonzero(self.cell == c)
            U = self._nodal_to_gauss(c) @ u[od.loc2glob[c]]
            vals[k] = tensor_rows(p, self.xi[k]) @ U
            g = np.stack([tensor_rows(p, self.xi[k], e) @ U for e in range(dim)], axis=-1)  # [k, e]
            J = mapping(p, cells.qpts[c], self.xi[k])[1]
            grads[k] = np.linalg.solve(np.swapaxes(J, 1, 2), g[:, :, None])[:, :, 0]
        return vals, grads

    def integrate(self, w=None):
        """rhs = E^T w, constrained rows 0"""
        w = np.ones(len(self.cell)) if w is None else np.asarray(w, np.float64)
        rhs = self.matrix().T @ w
        rhs[self.cells.od.constrained] = 0.0
        return rhs


def unread_dofs(mesh):
    """mask of the dofs no cell lists (the hanging dofs)"""
    m = np.ones(mesh.n_dofs, bool)
    m[mesh.arrays()["loc2glob"].reshape(-1)] = False
    return m
