"""numpy reference for the vector-valued quadrature-point operator mfgpu_vqop_* (small meshes only), built on
poisson_reference.Cells and qop_reference.grad_tables / hn_matrix.  A field has dim components in blocks,
u[a * n_dofs + i]; a constrained list is in that block numbering (None: the description's list in every component).

  apply(cells, src, ...)         (A u)_(a,i) = sum_q JxW_q [sum_k d_k phi_i sigma_ak + phi_i rho u_a], factor by factor with
                                 the dense per-cell tables, _hn on both sides of every component, identity rows
  cell_matrix / assemble         the same operator as dense cell matrices (local block numbering a * nd + i) and as a
                                 sparse matrix with identity rows
  diagonal / inverse_diagonal    its diagonal without the matrices; 1 on constrained and unreferenced entries
  isotropic_tensor(lam, mu, dim) C = lam d_ak d_bl + mu (d_ab d_kl + d_al d_bk)

Coefficients are per point: lam, mu, mass [cell, q]; tensor [cell, q, dim, dim, dim, dim] indexed (a, k, b, l), any
tensor; None = term absent.  sigma = lam (div u) I + mu (grad u + grad u^T) or sigma_ak = sum_bl C[a][k][b][l] d_l u_b."""
import numpy as np
import scipy.sparse as sp

import poisson_reference as pr
import qop_reference as qr


def isotropic_tensor(lam, mu, dim):
    lam, mu = np.asarray(lam, np.float64), np.asarray(mu, np.float64)
    d = np.eye(dim)
    return (lam[..., None, None, None, None] * np.einsum("ak,bl->akbl", d, d)
            + mu[..., None, None, None, None] * (np.einsum("ab,kl->akbl", d, d) + np.einsum("al,bk->akbl", d, d)))


def _coefs(cells, lam, mu, tensor, mass):
    od, dim = cells.od, cells.dim
    shape = (od.n_cells, od.nd)
    assert (lam is None) == (mu is None) and (lam is None or tensor is None)
    lam = None if lam is None else np.asarray(lam, np.float64).reshape(shape)
    mu = None if mu is None else np.asarray(mu, np.float64).reshape(shape)
    tensor = None if tensor is None else np.asarray(tensor, np.float64).reshape(shape + (dim,) * 4)
    mass = None if mass is None else np.asarray(mass, np.float64).reshape(shape)
    return lam, mu, tensor, mass


def constrained_flags(cells, constrained=None):
    """bool [dim * n_dofs]"""
    od, dim = cells.od, cells.dim
    con = np.zeros(dim * od.n_dofs, bool)
    if constrained is None:
        for a in range(dim):
            con[a * od.n_dofs + np.asarray(od.constrained, np.int64)] = True
    else:
        con[np.asarray(constrained, np.int64)] = True
    return con


def apply(cells: "pr.Cells", src, lam=None, mu=None, tensor=None, mass=None, constrained=None):
    od, dim = cells.od, cells.dim
    lam, mu, tensor, mass = _coefs(cells, lam, mu, tensor, mass)
    con = constrained_flags(cells, constrained)
    src = np.asarray(src, np.float64)
    s = np.where(con, 0.0, src).reshape(dim, od.n_dofs)
    dst = np.zeros((dim, od.n_dofs))
    w = od.JxW.astype(np.float64)
    for c in range(od.n_cells):
        idx = od.loc2glob[c]
        uc = [cells._hn(c, s[a][idx], False) for a in range(dim)]
        P, Phi = qr.grad_tables(cells, c), cells.Phi
        grad = np.stack([np.stack([P[l] @ uc[b] for l in range(dim)], axis=-1) for b in range(dim)], axis=1)  # [q, b, l]
        sigma = np.zeros((od.nd, dim, dim))  # [q, a, k]
        if tensor is not None:
            sigma += np.einsum("qakbl,qbl->qak", tensor[c], grad)
        if lam is not None:
            div = np.trace(grad, axis1=1, axis2=2)
            sigma += lam[c][:, None, None] * div[:, None, None] * np.eye(dim) \
                + mu[c][:, None, None] * (grad + np.swapaxes(grad, 1, 2))
        for a in range(dim):
            loc = sum(P[k].T @ (w[c] * sigma[:, a, k]) for k in range(dim))
            if mass is not None:
                loc = loc + Phi.T @ (w[c] * mass[c] * (Phi @ uc[a]))
            np.add.at(dst[a], idx, cells._hn(c, loc, True))
    dst = dst.reshape(-1)
    dst[con] = src[con]
    return dst


def cell_matrix(cells: "pr.Cells", c, lam=None, mu=None, tensor=None, mass=None):
    """dense K[a * nd + i, b * nd + j] of cell c, hanging-node resolved in every component"""
    od, dim = cells.od, cells.dim
    lam, mu, tensor, mass = _coefs(cells, lam, mu, tensor, mass)
    nd = od.nd
    w = od.JxW[c].astype(np.float64)
    P, Phi = qr.grad_tables(cells, c), cells.Phi
    C4 = tensor[c] if tensor is not None else (isotropic_tensor(lam[c], mu[c], dim) if lam is not None else None)
    K = np.zeros((dim * nd, dim * nd))
    Ch = qr.hn_matrix(cells, c)
    for a in range(dim):
        for b in range(dim):
            blk = np.zeros((nd, nd))
            if C4 is not None:
                for k in range(dim):
                    for l in range(dim):
                        blk += P[k].T @ ((w * C4[:, a, k, b, l])[:, None] * P[l])
            if mass is not None and a == b:
                blk += Phi.T @ ((w * mass[c])[:, None] * Phi)
            K[a * nd:(a + 1) * nd, b * nd:(b + 1) * nd] = blk if Ch is None else Ch.T @ blk @ Ch
    return K


def assemble(cells: "pr.Cells", lam=None, mu=None, tensor=None, mass=None, constrained=None) -> sp.csr_matrix:
    od, dim, nd = cells.od, cells.dim, cells.od.nd
    n = dim * od.n_dofs
    rows, cols, vals = [], [], []
    for c in range(od.n_cells):
        idx = np.concatenate([a * od.n_dofs + od.loc2glob[c].astype(np.int64) for a in range(dim)])
        rows.append(np.repeat(idx, dim * nd))
        cols.append(np.tile(idx, dim * nd))
        vals.append(cell_matrix(cells, c, lam, mu, tensor, mass).reshape(-1))
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    free = 1.0 - constrained_flags(cells, constrained)
    Dg = sp.diags(free)
    return (Dg @ A @ Dg + sp.diags(1.0 - free)).tocsr()


def diagonal(cells: "pr.Cells", lam=None, mu=None, tensor=None, mass=None, constrained=None):
    """A_jj without the cell matrices: with A_k = P_k C and B = Phi C, entry (a, i) of a cell is
    sum_q w [sum_kl C4[a][k][a][l] A_k[q,i] A_l[q,i] + rho B[q,i]^2]; 1 on constrained entries"""
    od, dim = cells.od, cells.dim
    lam, mu, tensor, mass = _coefs(cells, lam, mu, tensor, mass)
    w = od.JxW.astype(np.float64)
    d = np.zeros((dim, od.n_dofs))
    for c in range(od.n_cells):
        Ch = qr.hn_matrix(cells, c)
        P = qr.grad_tables(cells, c)
        A = [Pk if Ch is None else Pk @ Ch for Pk in P]
        B = cells.Phi if Ch is None else cells.Phi @ Ch
        C4 = tensor[c] if tensor is not None else (isotropic_tensor(lam[c], mu[c], dim) if lam is not None else None)
        for a in range(dim):
            loc = np.zeros(od.nd)
            if C4 is not None:
                for k in range(dim):
                    for l in range(dim):
                        loc += (w[c] * C4[:, a, k, a, l]) @ (A[k] * A[l])
            if mass is not None:
                loc += (w[c] * mass[c]) @ (B * B)
            np.add.at(d[a], od.loc2glob[c], loc)
    d = d.reshape(-1)
    d[constrained_flags(cells, constrained)] = 1.0
    return d


def inverse_diagonal(cells: "pr.Cells", lam=None, mu=None, tensor=None, mass=None, constrained=None):
    """1 / A_jj; 1 on constrained entries and on dofs no cell references"""
    od, dim = cells.od, cells.dim
    d = diagonal(cells, lam, mu, tensor, mass, constrained)
    unref = np.ones(od.n_dofs, bool)
    unref[od.loc2glob.reshape(-1)] = False
    d[np.tile(unref, dim)] = 1.0
    return 1.0 / d
