"""numpy reference for mfgpu_integrator_integrate and the quadrature-point operator mfgpu_qop_* (small meshes only), built
on poisson_reference.Cells and nonlinear_reference.evaluate:

  integrate(cells, v, g)            dst_i = sum_q JxW_q (phi_i v_q + grad_x phi_i . g_q), constrained rows 0
  apply(cells, src, ...)            (A u)_i = sum_q JxW_q [grad phi_i . (D grad u + gamma u) + phi_i (beta . grad u + c u)]
                                    with the dense per-cell tables, _hn on both sides, identity rows
  cell_matrix / assemble(cells, ...) the same operator as dense cell matrices C^T K C and as a sparse matrix;
                                    cell_diagonal / diagonal / inverse_diagonal: its diagonal without the matrices
  newton(cells, ...)                Newton for -div((1 + u^2) grad u) = f (nonlinear_reference's problem)

Coefficients are per point: diffusion [cell, q] (scalar a, D = a I) or [cell, q, dim, dim] (any matrix), convection (beta)
and flux (gamma) [cell, q, dim], reaction (c) [cell, q]; None = term absent."""
import numpy as np
import scipy.sparse as sp

import nonlinear_reference as nr
import poisson_reference as pr
from oracle import mf_oracle as o


def grad_tables(cells: "pr.Cells", c):
    """P[k][q, i] = d phi_i / d x_k at x_q of cell c: sum_e J^-1[e][k] Ghat_e"""
    od, dim = cells.od, cells.dim
    if od.uniform_j0:
        return [float(od.inv_jac[c]) * cells.Gt[k] for k in range(dim)]
    J = od.inv_jac[c].astype(np.float64)  # [q, e, k]
    return [sum(J[:, e, k][:, None] * cells.Gt[e] for e in range(dim)) for k in range(dim)]


def hn_matrix(cells: "pr.Cells", c):
    """o.hn_cell_matrix, computed once per constraint mask (it depends on the cell through the mask alone)"""
    od = cells.od
    if od.constraint_mask is None or od.constraint_mask[c] == 0:
        return None
    cache = cells.__dict__.setdefault("_hn_matrices", {})
    mask = int(od.constraint_mask[c])
    if mask not in cache:
        cache[mask] = o.hn_cell_matrix(od, c)
    return cache[mask]


def integrate(cells: "pr.Cells", v=None, g=None):
    od, dim = cells.od, cells.dim
    out = np.zeros(od.n_dofs)
    w = od.JxW.astype(np.float64)
    for c in range(od.n_cells):
        loc = np.zeros(od.nd)
        if v is not None:
            loc += cells.Phi.T @ (w[c] * np.asarray(v, np.float64).reshape(od.n_cells, od.nd)[c])
        if g is not None:
            gc = np.asarray(g, np.float64).reshape(od.n_cells, od.nd, dim)[c]
            P = grad_tables(cells, c)
            loc += sum(P[k].T @ (w[c] * gc[:, k]) for k in range(dim))
        np.add.at(out, od.loc2glob[c], cells._hn(c, loc, True))
    out[od.constrained] = 0.0
    return out


def cell_matrix(cells: "pr.Cells", c, diffusion=None, convection=None, flux=None, reaction=None):
    """dense K[i, j] of cell c, hanging-node resolved (C^T K C)"""
    od, dim = cells.od, cells.dim
    w = od.JxW[c].astype(np.float64)
    P, Phi = grad_tables(cells, c), cells.Phi
    K = np.zeros((od.nd, od.nd))
    if diffusion is not None:
        D = np.asarray(diffusion, np.float64)
        if D.size == od.n_cells * od.nd:
            D = D.reshape(od.n_cells, od.nd)[c][:, None, None] * np.eye(dim)
        else:
            D = D.reshape(od.n_cells, od.nd, dim, dim)[c]
        for k in range(dim):
            for l in range(dim):
                K += P[k].T @ ((w * D[:, k, l])[:, None] * P[l])
    if flux is not None:
        gm = np.asarray(flux, np.float64).reshape(od.n_cells, od.nd, dim)[c]
        K += sum(P[k].T @ ((w * gm[:, k])[:, None] * Phi) for k in range(dim))
    if convection is not None:
        b = np.asarray(convection, np.float64).reshape(od.n_cells, od.nd, dim)[c]
        K += sum(Phi.T @ ((w * b[:, k])[:, None] * P[k]) for k in range(dim))
    if reaction is not None:
        K += Phi.T @ ((w * np.asarray(reaction, np.float64).reshape(od.n_cells, od.nd)[c])[:, None] * Phi)
    C = hn_matrix(cells, c)
    return K if C is None else C.T @ K @ C


def apply(cells: "pr.Cells", src, diffusion=None, convection=None, flux=None, reaction=None, transpose=False):
    """the cell matrices of cell_matrix applied factor by factor (dense tables, no matrix formed): _hn, values and
    gradients at the points, the point-wise terms, integration, transposed _hn.  transpose: D -> D^T, beta <-> gamma
    (test_qop_host checks that this is the transpose of assemble)"""
    od, dim = cells.od, cells.dim
    shape = (od.n_cells, od.nd)
    D = None if diffusion is None else np.asarray(diffusion, np.float64)
    if D is not None:
        D = D.reshape(shape)[..., None, None] * np.eye(dim) if D.size == od.n_cells * od.nd else D.reshape(shape + (dim, dim))
    beta = None if convection is None else np.asarray(convection, np.float64).reshape(shape + (dim,))
    gamma = None if flux is None else np.asarray(flux, np.float64).reshape(shape + (dim,))
    cr = None if reaction is None else np.asarray(reaction, np.float64).reshape(shape)
    if transpose:
        D, beta, gamma = None if D is None else np.swapaxes(D, -1, -2), gamma, beta
    s = np.array(src, dtype=np.float64)
    s[od.constrained] = 0.0
    dst = np.zeros(od.n_dofs)
    w = od.JxW.astype(np.float64)
    for c in range(od.n_cells):
        uc = cells._hn(c, s[od.loc2glob[c]], False)
        P, Phi = grad_tables(cells, c), cells.Phi
        val, grad = Phi @ uc, np.stack([Pk @ uc for Pk in P], axis=-1)  # [q], [q, k]
        fl, vo = np.zeros((od.nd, dim)), np.zeros(od.nd)
        if D is not None:
            fl += np.einsum("qkl,ql->qk", D[c], grad)
        if gamma is not None:
            fl += gamma[c] * val[:, None]
        if beta is not None:
            vo += np.sum(beta[c] * grad, axis=-1)
        if cr is not None:
            vo += cr[c] * val
        loc = Phi.T @ (w[c] * vo) + sum(P[k].T @ (w[c] * fl[:, k]) for k in range(dim))
        np.add.at(dst, od.loc2glob[c], cells._hn(c, loc, True))
    dst[od.constrained] = np.asarray(src, np.float64)[od.constrained]
    return dst


def assemble(cells: "pr.Cells", diffusion=None, convection=None, flux=None, reaction=None) -> sp.csr_matrix:
    od, nd = cells.od, cells.od.nd
    rows, cols, vals = [], [], []
    for c in range(od.n_cells):
        idx = od.loc2glob[c].astype(np.int64)
        rows.append(np.repeat(idx, nd))
        cols.append(np.tile(idx, nd))
        vals.append(cell_matrix(cells, c, diffusion, convection, flux, reaction).reshape(-1))
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(od.n_dofs, od.n_dofs)).tocsr()
    free = np.ones(od.n_dofs)
    free[od.constrained] = 0.0
    Dg = sp.diags(free)
    return (Dg @ A @ Dg + sp.diags(1.0 - free)).tocsr()


def cell_diagonal(cells: "pr.Cells", diffusion=None, convection=None, flux=None, reaction=None):
    """diag(C^T K C) of every cell, [cell, i], without the cell matrices: with A_k = P_k C and B = Phi C,
    sum_q w [sum_kl D_kl A_k[q,i] A_l[q,i] + sum_k (gamma_k + beta_k) A_k[q,i] B[q,i] + c B[q,i]^2].  On uniform-J0 meshes
    the cells of one constraint mask share C, A_k / J0^-1 and B and are done together."""
    od, dim = cells.od, cells.dim
    shape = (od.n_cells, od.nd)
    w = od.JxW.astype(np.float64)
    D = None if diffusion is None else np.asarray(diffusion, np.float64)
    if D is not None:
        D = D.reshape(shape)[..., None, None] * np.eye(dim) if D.size == od.n_cells * od.nd else D.reshape(shape + (dim, dim))
    bg = sum(np.asarray(a, np.float64).reshape(shape + (dim,)) for a in (convection, flux) if a is not None)
    cr = None if reaction is None else np.asarray(reaction, np.float64).reshape(shape)
    masks = np.zeros(od.n_cells, np.int64) if od.constraint_mask is None else od.constraint_mask.astype(np.int64)
    if od.uniform_j0:
        groups = [np.nonzero(masks == m)[0] for m in np.unique(masks)]
        j0 = od.inv_jac.astype(np.float64).reshape(-1, 1)
    else:
        groups = [np.array([c]) for c in range(od.n_cells)]
        j0 = np.ones((od.n_cells, 1))
    out = np.zeros(shape)
    for cs in groups:
        C = hn_matrix(cells, cs[0])
        P = cells.Gt if od.uniform_j0 else grad_tables(cells, cs[0])
        A = [Pk if C is None else Pk @ C for Pk in P]
        B = cells.Phi if C is None else cells.Phi @ C
        if D is not None:
            for k in range(dim):
                for l in range(dim):
                    out[cs] += (w[cs] * D[cs, :, k, l] * j0[cs] ** 2) @ (A[k] * A[l])
        if not np.isscalar(bg):
            for k in range(dim):
                out[cs] += (w[cs] * bg[cs, :, k] * j0[cs]) @ (A[k] * B)
        if cr is not None:
            out[cs] += (w[cs] * cr[cs]) @ (B * B)
    return out


def diagonal(cells: "pr.Cells", **terms):
    """A_ii from cell_diagonal; 1 on constrained dofs (test_qop_host checks it against assemble(...).diagonal())"""
    od = cells.od
    d = np.zeros(od.n_dofs)
    np.add.at(d, od.loc2glob.reshape(-1), cell_diagonal(cells, **terms).reshape(-1))
    d[od.constrained] = 1.0
    return d


def inverse_diagonal(cells: "pr.Cells", **terms):
    """1 / A_ii; 1 on constrained dofs and on dofs no cell references"""
    od = cells.od
    d = diagonal(cells, **terms)
    unref = np.ones(od.n_dofs, bool)
    unref[od.loc2glob.reshape(-1)] = False
    d[unref] = 1.0
    return 1.0 / d


def bicgstab(A, b, dinv, rtol=1e-12, max_it=20000):
    """right-preconditioned BiCGStab, zero start, until |r| <= rtol |b|: the loop of the GPU tests and of the shim's
    SolverBicgstab.  A: callable."""
    x, r = np.zeros_like(b), b.copy()
    r0, tol = r.copy(), rtol * np.linalg.norm(b)
    rho = alpha = omega = 1.0
    v, p = np.zeros_like(b), np.zeros_like(b)
    for it in range(1, max_it + 1):
        rho_new = r0 @ r
        beta = (rho_new / rho) * (alpha / omega)
        rho = rho_new
        p = r + beta * (p - omega * v)
        y = dinv * p
        v = A(y)
        alpha = rho / (r0 @ v)
        s = r - alpha * v
        if np.linalg.norm(s) <= tol:
            return x + alpha * y, it
        z = dinv * s
        t = A(z)
        omega = (t @ s) / (t @ t)
        x = x + alpha * y + omega * z
        r = s - omega * t
        if np.linalg.norm(r) <= tol:
            return x, it
    raise RuntimeError("BiCGStab did not converge")


def newton_terms(cells: "pr.Cells", u):
    """(residual R(u) = integrate(-f, (1 + u^2) grad u), Jacobian terms: diffusion 1 + u^2, flux 2 u grad u)"""
    val, grad = nr.evaluate(cells, u)
    a = nr.coefficient(val)
    R = integrate(cells, -nr.load(cells.qpts), a[..., None] * grad)
    return R, {"diffusion": a, "flux": 2.0 * val[..., None] * grad}


def newton(cells: "pr.Cells", steps=None, tol=1e-10, solve=None, max_steps=50):
    """nonlinear_reference.picard's start (u* on the constrained dofs, 0 elsewhere) and stopping rule
    (|u_{k+1} - u_k| / |u_{k+1}| <= tol), Newton updates J(u_k) d = -R(u_k) by a sparse direct solve (or
    solve(cells, terms, b)).  Returns (u, [relative update norms])"""
    u, hist = cells.lift(), []
    for _ in range(max_steps if steps is None else steps):
        R, terms = newton_terms(cells, u)
        d = nr.direct_solve(assemble(cells, **terms), -R) if solve is None else solve(cells, terms, -R)
        u = u + d
        hist.append(np.linalg.norm(d) / np.linalg.norm(u))
        if steps is None and hist[-1] <= tol:
            break
    return u, hist


def bicgstab_solve(cells, terms, b):
    """the GPU tests' linear solve on the reference operator: BiCGStab with the inverse diagonal to 1e-12 |b|"""
    A = assemble(cells, **terms)
    return bicgstab(lambda x: A @ x, b, inverse_diagonal(cells, **terms))[0]
