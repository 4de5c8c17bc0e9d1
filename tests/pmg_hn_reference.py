"""float64 numpy restatement of the p-multigrid transfer on meshes with hanging nodes for the
tests; host only.  What pmg_reference.py does for conforming meshes, with the same conventions.

  constrained_positions  the local positions of a cell that hn_resolve with the cell's mask CAN write: found by running
                         the oracle's hn_resolve with a dense weight matrix on a generic input and looking at which
                         entries changed, not taken from the product's geometry
  owners_hn              [cells, nfd] 1.0 where the cell is the first one that lists the fine dof at a position that is
                         not constrained
  p_transfer_matrix_hn   the sparse P [n_fine, n_coarse]: per cell P_loc C_pc(mask), P_loc the Kronecker product of the 1D
                         matrix (pmg_reference.cell_matrix), C_pc the oracle's hn_resolve(NOTRANSPOSE) at the coarse degree
                         with the oracle's weights; every fine dof written by its owner only; the columns of the coarse
                         Dirichlet dofs zero.  prolongate is P x, restrict_and_add dst + P^T src.
  level_hierarchy_hn     pmg_reference.level_hierarchy over the SAME cells at rising degrees, masks allowed
"""
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import mg_reference as mg
import pmg_reference as pr
from oracle import mf_oracle as o
from util import oracle_desc_from_mesh


@functools.lru_cache(maxsize=None)
def constrained_positions(dim, p, mask):
    """bool [(p+1)^dim], lexicographic with x fastest"""
    n = p + 1
    if not mask:
        return np.zeros(n ** dim, dtype=bool)
    rng = np.random.default_rng(12345)
    W = rng.uniform(0.3, 0.7, (n, n))       # dense: no entry is 0 or 1, so every row of a flagged pencil moves
    v = rng.uniform(1.0, 2.0, (n,) * dim)
    return (o.hn_resolve(v, int(mask), dim, p, W, False) != v).reshape(-1)


@functools.lru_cache(maxsize=None)
def _resolve_matrix(dim, p, mask, wkey):
    nd = (p + 1) ** dim
    if not mask:
        return np.eye(nd)
    W = np.frombuffer(wkey, dtype=np.float64)
    C = np.zeros((nd, nd))
    for j in range(nd):
        e = np.zeros(nd)
        e[j] = 1.0
        C[:, j] = o.hn_resolve(e.reshape((p + 1,) * dim), int(mask), dim, p, W, False).reshape(-1)
    return C


def resolve_matrix(dim, p, mask, weights=None):
    """dense C_p(mask) of hn_resolve(NOTRANSPOSE) (oracle.hn_cell_matrix for one mask value); identity for mask 0"""
    W = o.constraint_weights(p) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    return _resolve_matrix(dim, p, int(mask), np.ascontiguousarray(W).tobytes())


def _masks(mask, n_cells):
    return np.zeros(n_cells, dtype=np.int64) if mask is None else np.asarray(mask, dtype=np.int64).reshape(n_cells)


def owners_hn(dim, pf, fine_cell_dofs, mask, n_fine):
    nfd = (pf + 1) ** dim
    fd = np.asarray(fine_cell_dofs, dtype=np.int64).reshape(-1, nfd)
    m = _masks(mask, len(fd))
    free = np.stack([~constrained_positions(dim, pf, int(v)) for v in m]) if len(fd) else np.zeros((0, nfd), dtype=bool)
    flat, where = fd.reshape(-1), np.arange(fd.size)
    first = np.full(n_fine, fd.size, dtype=np.int64)
    sel = free.reshape(-1)
    np.minimum.at(first, flat[sel], where[sel])
    return (first[flat] == where).astype(np.float64).reshape(fd.shape)


def p_transfer_matrix_hn(dim, pc, pf, coarse_mesh_arrays, fine_mesh_arrays, mask, dirichlet, p1=None, weights=None):
    """coarse_mesh_arrays, fine_mesh_arrays: (loc2glob, n_dofs) of the two descriptions; mask: [n_cells] or None; dirichlet:
    the coarse dofs read as 0; p1: [pf + 1, pc + 1] (None: pmg_reference.P1); weights: [(pc+1)^2] (None: the oracle's)"""
    (cd, n_coarse), (fd, n_fine) = coarse_mesh_arrays, fine_mesh_arrays
    Pc = pr.cell_matrix(dim, pr.P1(pc, pf) if p1 is None else np.asarray(p1, dtype=np.float64).reshape(pf + 1, pc + 1))
    nfd, ncd = Pc.shape
    cd = np.asarray(cd, dtype=np.int64).reshape(-1, ncd)
    fd = np.asarray(fd, dtype=np.int64).reshape(-1, nfd)
    m = _masks(mask, len(cd))
    w = owners_hn(dim, pf, fd, m, n_fine)
    rows, cols, vals = [], [], []
    for v in np.unique(m):  # cells grouped by mask value
        sel = m == v
        PC = Pc @ resolve_matrix(dim, pc, int(v), weights)
        rows.append(np.repeat(fd[sel], ncd, axis=1).reshape(-1))
        cols.append(np.tile(cd[sel], (1, nfd)).reshape(-1))
        vals.append((w[sel][:, :, None] * PC[None, :, :]).reshape(-1))
    P = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n_fine, n_coarse)).tocsr()
    free = np.ones(n_coarse)
    free[np.asarray(dirichlet, dtype=np.int64)] = 0.0
    return (P @ sp.diags(free)).tocsr()


def mesh_pair_matrix_hn(coarse, fine, dirichlet=None, p1=None, weights=None):
    """P of two stand-in meshes of the same cells (the coarse mesh's constrained dofs unless `dirichlet` is given)"""
    dim, pc, pf = int(coarse.desc.dim), int(coarse.desc.degree), int(fine.desc.degree)
    ca, fa = coarse.arrays(), fine.arrays()
    mc, mfine = ca["constraint_mask"], fa["constraint_mask"]
    assert pc < pf and coarse.n_cells == fine.n_cells and (mc is None) == (mfine is None)
    assert mc is None or np.array_equal(mc, mfine)
    con = ca["constrained_dofs"] if dirichlet is None else dirichlet
    return p_transfer_matrix_hn(dim, pc, pf, (ca["loc2glob"], coarse.n_dofs), (fa["loc2glob"], fine.n_dofs), mc, con, p1,
                                weights)


def level_hierarchy_hn(meshes64, lmax=None):
    """pmg_reference.level_hierarchy for one set of cells at rising degrees (double meshes, coarse to fine), with or
    without hanging nodes; vcycle, chebyshev and the rest of pmg_reference / mg_reference run on it unchanged"""
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
    H.P = [None] + [mesh_pair_matrix_hn(meshes64[l - 1], meshes64[l]) for l in range(1, H.n_levels)]
    H.lmax = [mg.lambda_max(A, d) for A, d in zip(H.A, H.dinv)] if lmax is None else [float(x) for x in lmax]
    H.coarse_solve = spla.splu(H.A[0].tocsc()).solve
    return H
