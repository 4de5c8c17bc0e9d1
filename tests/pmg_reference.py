"""float64 numpy restatement of p-multigrid for the tests; host only.

  P1(pc, pf)            the 1D matrix of the p-transfer from the oracle's own tables: the FE_Q(pc) Lagrange basis on its
                        Gauss-Lobatto nodes (oracle gll_01, lagrange_eval) at the FE_Q(pf) nodes, [pf + 1, pc + 1]
  p_transfer_matrix     the sparse P [n_fine, n_coarse] of a mesh pair: per cell the Kronecker product of the 1D matrix,
                        every fine dof written by its OWNER cell only (the first cell that lists it), the columns of the
                        coarse Dirichlet dofs zero.  prolongate is P x, restrict_and_add dst + P^T src.
  level_hierarchy       an mg_reference.Hierarchy (its vcycle and chebyshev run unchanged) over any coarse-to-fine list of
                        conforming stand-in meshes: the h-transfer between meshes of one degree, the p-transfer where the
                        degree rises; matrices from oracle.assemble; lambda_max per level is an INPUT (None: 1.2 x the
                        exact largest eigenvalue of D^-1 A, mg_reference.lambda_max)
  cg_iterations         CG preconditioned by one V-cycle, to a relative residual
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import cg_reference as cgref
import mg_reference as mg
import pymfgpu as mf
from oracle import mf_oracle as o
from util import oracle_desc_from_mesh


def P1(pc, pf):
    """[X, x] = phi_x(xi_X)"""
    return o.lagrange_eval(o.gll_01(pc), o.gll_01(pf))[0].T.copy()


def cell_matrix(dim, p1):
    Pc = np.ones((1, 1))
    for _ in range(dim):  # x fastest: kron(later, earlier)
        Pc = np.kron(p1, Pc)
    return Pc


def owners(fine_cell_dofs, n_fine):
    """[cells, nfd] 1.0 where the cell is the first one that lists the fine dof"""
    flat = np.asarray(fine_cell_dofs, dtype=np.int64).reshape(-1)
    first = np.full(n_fine, flat.size, dtype=np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    return (first[flat] == np.arange(flat.size)).astype(np.float64).reshape(np.shape(fine_cell_dofs))


def p_transfer_matrix(dim, pc, pf, coarse_cell_dofs, fine_cell_dofs, n_coarse, n_fine, coarse_dirichlet, p1=None):
    Pc = cell_matrix(dim, P1(pc, pf) if p1 is None else np.asarray(p1, dtype=np.float64).reshape(pf + 1, pc + 1))
    nfd, ncd = Pc.shape
    cd = np.asarray(coarse_cell_dofs, dtype=np.int64).reshape(-1, ncd)
    fd = np.asarray(fine_cell_dofs, dtype=np.int64).reshape(-1, nfd)
    w = owners(fd, n_fine)
    rows = np.repeat(fd, ncd, axis=1).reshape(-1)
    cols = np.tile(cd, (1, nfd)).reshape(-1)
    vals = (w[:, :, None] * Pc[None, :, :]).reshape(-1)
    P = sp.coo_matrix((vals, (rows, cols)), shape=(n_fine, n_coarse)).tocsr()
    free = np.ones(n_coarse)
    free[np.asarray(coarse_dirichlet, dtype=np.int64)] = 0.0
    return (P @ sp.diags(free)).tocsr()


def mesh_pair_matrix(coarse, fine, p1=None):
    """P of two stand-in meshes: equal degrees = the h-transfer of mg_reference, a rising degree = the p-transfer"""
    dim, pc, pf = int(coarse.desc.dim), int(coarse.desc.degree), int(fine.desc.degree)
    con = coarse.arrays()["constrained_dofs"]
    if pc == pf:
        cd, fd = coarse.transfer_patches(fine)
        return mg.transfer_matrix(dim, pc, cd, fd, coarse.n_dofs, fine.n_dofs, con)
    assert pc < pf and coarse.n_cells == fine.n_cells
    return p_transfer_matrix(dim, pc, pf, coarse.arrays()["loc2glob"], fine.arrays()["loc2glob"], coarse.n_dofs,
                             fine.n_dofs, con, p1)


def level_hierarchy(meshes64, lmax=None):
    """meshes64: the level meshes in double, coarse to fine (cubes or balls, any mix of h- and p-steps)"""
    H = mg.Hierarchy.__new__(mg.Hierarchy)
    H.dim, H.p = int(meshes64[0].desc.dim), int(meshes64[-1].desc.degree)
    H.mesh, H.H = meshes64[-1], None
    H.n_levels = len(meshes64)
    H.meshes = list(meshes64)
    H.od = [oracle_desc_from_mesh(M, dtype=np.float64) for M in meshes64]
    none = np.zeros(0, dtype=np.uint32)
    H.edge = [none for _ in meshes64]
    H.odc = H.od
    ident = np.arange(meshes64[-1].n_dofs, dtype=np.uint32)
    H.pairs = [(none, none) for _ in meshes64[:-1]] + [(ident, ident)]
    H.A = [o.assemble(od).tocsr() for od in H.od]
    H.down = [sp.csr_matrix(A.shape) for A in H.A]  # no refinement edges
    H.up = H.down
    H.dinv = [o.compute_inverse_diagonal(od) for od in H.od]
    H.P = [None] + [mesh_pair_matrix(meshes64[l - 1], meshes64[l]) for l in range(1, H.n_levels)]
    H.lmax = [mg.lambda_max(A, d) for A, d in zip(H.A, H.dinv)] if lmax is None else [float(x) for x in lmax]
    H.coarse_solve = spla.splu(H.A[0].tocsc()).solve
    return H


def with_lambda_max(H, lmax):
    """the same hierarchy (matrices shared, never modified) with other smoother bounds"""
    G = mg.Hierarchy.__new__(mg.Hierarchy)
    G.__dict__.update(H.__dict__)
    G.lmax = [float(x) for x in lmax]
    return G


def meshes_of(dim, spec, number_type=mf.F64, ball=False):
    """spec: (cells per direction, degree) per level for cubes, (n_ref, degree) for balls"""
    if ball:
        return [mf.Mesh.ball(dim, p, r, number_type=number_type) for r, p in spec]
    return [mf.Mesh.uniform(dim, p, n, number_type=number_type) for n, p in spec]


def rhs(H, seed=None):
    """the right-hand side of the poisson-mg / poisson-pmg drivers, b = A x* with x* = sin(0.37 i) + 0.5 cos(0.011 i), zero
    on the Dirichlet dofs (seed None), or a seeded random one, zero on the Dirichlet dofs"""
    if seed is None:
        i = np.arange(H.mesh.n_dofs, dtype=np.float64)
        xs = np.sin(0.37 * i) + 0.5 * np.cos(0.011 * i)
        xs[H.od[-1].constrained] = 0.0
        return H.A[-1] @ xs
    b = np.random.default_rng(seed).standard_normal(H.mesh.n_dofs)
    b[H.od[-1].constrained] = 0.0
    return b


def cg_iterations(H, b, relative=1e-10, max_iterations=100):
    """(iterations, x) of CG on the finest level's matrix with H.vcycle as preconditioner"""
    A = H.A[-1]
    last = None
    for last in cgref.cg(lambda v: A @ v, b, H.vcycle, np.float64, relative * np.linalg.norm(b), max_iterations):
        pass
    it, status, _, x = last
    assert status == 1, (it, status)
    return it, x
