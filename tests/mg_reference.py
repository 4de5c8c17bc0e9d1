"""float64 numpy restatement of ONE local-smoothing V-cycle on the hierarchy of an adaptive stand-in mesh, in the schedule
of tests/test_gpu_mg_adaptive.py::v_step (Janssen & Kanschat, local smoothing with edge matrices):

  level l > 0:  x = Chebyshev(A_l, defect_l) from a zero start                 pre-smoothing
                t = defect_l - A_l x - down_l x                                 residual with the edge rows
                defect_{l-1} += R_l t                                           restrict_and_add
                x_{l-1} = V-cycle(l - 1)
                x += P_l x_{l-1}                                                prolongate
                x = Chebyshev(A_l, defect_l - up_l x) started from x            post-smoothing
  level 0:      x = A_0^-1 defect_0                                             scipy's sparse direct solver

with copy_to_mg / copy_from_mg through the hierarchy's copy pairs around it.  Every matrix is built from the oracle
(oracle/mf_oracle.py): A_l = assemble of the level description with Dirichlet AND refinement-edge dofs constrained, the
interface matrices are blocks of K_l = assemble of the unconstrained description (what vmult_interface_down / _up
compute), P_l is the sparse form of mg_prolongate and R_l of mg_restrict_and_add, D^-1 = compute_inverse_diagonal.
tests/test_mg_reference_host.py checks each of these sparse forms against the oracle's own function on random vectors, and
the V-cycle as a whole by what it must be: a symmetric positive definite preconditioner under which CG converges.

Vectors are [n] or blocks [n, k] (k vectors at once: the host test builds the V-cycle's matrix that way).  Small meshes
only.  The hierarchy is host-only, so nothing here touches a GPU."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import pymfgpu as mf
from oracle import mf_oracle as o
from util import oracle_desc_from_mesh

DEGREE, SMOOTHING_RANGE = 5, 15.0  # of the Chebyshev smoother, as test_gpu_mg_adaptive.py and the poisson-mg drivers


def with_constrained(od: o.Desc, constrained) -> o.Desc:
    """the description with another constrained set (level meshes have no hanging-node masks)"""
    assert od.constraint_mask is None or not od.constraint_mask.any()
    return o.Desc(od.dim, od.degree, od.n_dofs, od.loc2glob, od.JxW, od.inv_jac, od.coefficient,
                  np.asarray(constrained, dtype=np.uint32), None, np.float64, od.shape_values, od.shape_gradients)


def transfer_matrix(dim, p, coarse_cell_dofs, fine_patch_dofs, n_coarse, n_fine, coarse_dirichlet):
    """P [n_fine, n_coarse] with P x = o.mg_prolongate(..., x): per coarse cell the tensor product of the oracle's 1D
    matrix, weighted by the oracle's patch weights, columns of the coarse Dirichlet dofs zero.  restrict_and_add is
    dst + P^T src (the zero columns are the Dirichlet rows it skips)."""
    P1 = o.mg_prolongation_1d(p)
    Pc = np.ones((1, 1))
    for _ in range(dim):  # x fastest: kron(later, earlier)
        Pc = np.kron(P1, Pc)
    w = o._mg_weights(fine_patch_dofs, n_fine)  # [cell, nf^dim]
    nfd, ncd = Pc.shape
    rows = np.repeat(fine_patch_dofs.astype(np.int64), ncd, axis=1).reshape(-1)
    cols = np.tile(coarse_cell_dofs.astype(np.int64), (1, nfd)).reshape(-1)
    vals = (w[:, :, None] * Pc[None, :, :]).reshape(-1)
    P = sp.coo_matrix((vals, (rows, cols)), shape=(n_fine, n_coarse)).tocsr()
    free = np.ones(n_coarse)
    free[np.asarray(coarse_dirichlet, dtype=np.int64)] = 0.0
    return (P @ sp.diags(free)).tocsr()


def lambda_max(A, dinv):
    """1.2 times the largest eigenvalue of D^-1 A (of the similar symmetric D^-1/2 A D^-1/2; deterministic start)"""
    s = sp.diags(np.sqrt(dinv))
    S = (s @ A @ s).tocsc()
    if S.shape[0] <= 64:
        lam = np.linalg.eigvalsh(S.toarray())[-1]
    else:
        lam = spla.eigsh(S, k=1, which="LA", tol=1e-12, v0=np.ones(S.shape[0]))[0][0]
    return 1.2 * float(lam)


class Hierarchy:
    """the product's own hierarchy (mf.Mesh.adaptive_mg + mf.MgHierarchy) with the oracle's matrices of every level"""

    def __init__(self, dim, p, n_ref, number_type=mf.F64, matrices=True):
        self.dim, self.p = dim, p
        self.mesh = mf.Mesh.adaptive_mg(dim, p, n_ref, number_type=number_type)
        self.H = mf.MgHierarchy(self.mesh)
        self.n_levels = self.H.n_levels
        self.meshes = [self.H.level_mesh(l) for l in range(self.n_levels)]
        self.od = [oracle_desc_from_mesh(M, dtype=np.float64) for M in self.meshes]
        self.edge = [self.H.edge_dofs(l) for l in range(self.n_levels)]
        self.odc = [with_constrained(od, np.union1d(od.constrained, E)) for od, E in zip(self.od, self.edge)]
        self.pairs = [self.H.copy_pairs(l) for l in range(self.n_levels)]  # (active dofs, level dofs)
        nd, nfd = (p + 1) ** dim, (2 * p + 1) ** dim
        self.patches = [None] + [self.H.transfer_arrays(l, nd, nfd) for l in range(1, self.n_levels)]
        if matrices:
            self.build_matrices()

    def build_matrices(self):
        self.A, self.down, self.up, self.dinv, self.P, self.lmax = [], [], [], [], [None], []
        for l in range(self.n_levels):
            od, odc, E = self.od[l], self.odc[l], self.edge[l].astype(np.int64)
            n = od.n_dofs
            A = o.assemble(odc)
            K = o.assemble(o._unconstrained(od))
            sel_e, free = np.zeros(n), np.ones(n)
            sel_e[E] = 1.0
            free[odc.constrained] = 0.0
            self.A.append(A)
            self.down.append((sp.diags(sel_e) @ K @ sp.diags(free)).tocsr())  # rows E of K (columns C zeroed)
            self.up.append((sp.diags(free) @ K @ sp.diags(sel_e)).tocsr())    # columns E of K (rows C zeroed)
            self.dinv.append(o.compute_inverse_diagonal(odc))
            self.lmax.append(lambda_max(A, self.dinv[l]))
            if l > 0:
                cd, fd = self.patches[l]
                self.P.append(transfer_matrix(self.dim, self.p, cd, fd, self.od[l - 1].n_dofs, n,
                                              self.od[l - 1].constrained))
        self.coarse_solve = spla.splu(self.A[0].tocsc()).solve

    def chebyshev(self, l, x, b, zero_start):
        """PreconditionChebyshev with D^-1 as inner preconditioner, on [lmax / SMOOTHING_RANGE, lmax]"""
        A, lmax = self.A[l], self.lmax[l]
        dinv = self.dinv[l] if b.ndim == 1 else self.dinv[l][:, None]
        lmin = lmax / SMOOTHING_RANGE
        theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
        sigma = theta / delta
        rho = 1.0 / sigma
        r = b.copy() if zero_start else b - A @ x
        d = (1.0 / theta) * r * dinv
        x = d.copy() if zero_start else x + d
        for _ in range(DEGREE - 1):
            r = r - A @ d
            rho_new = 1.0 / (2.0 * sigma - rho)
            d = (rho_new * rho) * d + (2.0 * rho_new / delta) * r * dinv
            x = x + d
            rho = rho_new
        return x

    def vcycle(self, r):
        """z = M^-1 r on the active mesh's vectors ([N] or [N, k])"""
        r = np.asarray(r, dtype=np.float64)
        defect = []
        for l in range(self.n_levels):  # copy_to_mg
            a, b = self.pairs[l]
            d = np.zeros((self.od[l].n_dofs,) + r.shape[1:])
            d[b] = r[a]
            defect.append(d)
        sol = [None] * self.n_levels  # every level's solution is kept: copy_from_mg reads them all

        def v_step(l):
            if l == 0:
                sol[0] = self.coarse_solve(defect[0])
                return
            x = self.chebyshev(l, None, defect[l], True)
            t = defect[l] - self.A[l] @ x - self.down[l] @ x
            defect[l - 1] = defect[l - 1] + self.P[l].T @ t
            v_step(l - 1)
            x = x + self.P[l] @ sol[l - 1]
            sol[l] = self.chebyshev(l, x, defect[l] - self.up[l] @ x, False)

        v_step(self.n_levels - 1)
        z = np.zeros_like(r)
        for l in range(self.n_levels):
            a, b = self.pairs[l]
            z[a] = sol[l][b]
        return z
