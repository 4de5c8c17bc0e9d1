"""float64 numpy restatement of global-coarsening multigrid for the tests; host only.

  coarsen_rule         a pure-Python restatement of one coarsening step of a leaf set: every complete family of sibling
                       leaves becomes its parent; then, until nothing changes, a new parent that a leaf two or more
                       levels finer touches over a face (3D: or an edge) is split again.  Written on sets of tuples and
                       on covering levels, not on the product's tree code
  one_irregular        the check itself, on any leaf set
  gc_transfer_matrix   the sparse P [n_fine, n_coarse] of a mesh pair: per fine cell kron(E(child)) @ resolve_matrix(dim,
                       p, coarse mask of the parent), E the lower / upper half of the oracle's 1D h-matrix per direction
                       (identity for child 0), scattered through owners_hn with the FINE mask; the columns of the coarse
                       Dirichlet dofs zero.  resolve_matrix and owners_hn are pmg_hn_reference's
  coarsening_map       (parent, child) from the two meshes' cell_levels, by coordinates
  level_hierarchy_gc   pmg_hn_reference.level_hierarchy_hn over coarsened meshes followed by one mesh at rising degrees
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import mg_reference as mg
import pmg_hn_reference as hr
from oracle import mf_oracle as o
from util import oracle_desc_from_mesh


# ---- the coarsening rule


def _offsets(dim):
    out = []
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in ((-1, 0, 1) if dim == 3 else (0,)):
                nz = (ox != 0) + (oy != 0) + (oz != 0)
                if nz == 1 or (dim == 3 and nz == 2):
                    out.append((ox, oy, oz))
    return out


def _covering(active, dim, level, c):
    """level of the leaf that is (level, c) or an ancestor of it; -1: (level, c) is refined; -2: outside the root"""
    if any(c[d] < 0 or c[d] >= (1 << level) for d in range(dim)):
        return -2
    c = list(c)
    for ll in range(level, -1, -1):
        if (ll, c[0], c[1], c[2]) in active:
            return ll
        c = [v >> 1 for v in c]
    return -1


def one_irregular(dim, leaves):
    active = {tuple(int(v) for v in l) for l in leaves}
    for (l, cx, cy, cz) in active:
        for o_ in _offsets(dim):
            lv = _covering(active, dim, l, (cx + o_[0], cy + o_[1], cz + o_[2]))
            if 0 <= lv < l - 1:
                return False
    return True


def _touches_two_finer(active, dim, P):
    l, c = P[0], P[1:]
    for o_ in _offsets(dim):
        nb = tuple(c[d] + o_[d] for d in range(3))
        if _covering(active, dim, l, nb) != -1:
            continue
        for k in range(1 << dim):
            b = [(k >> d) & 1 for d in range(dim)] + [0] * (3 - dim)
            if any((o_[d] == 1 and b[d] != 0) or (o_[d] == -1 and b[d] != 1) for d in range(dim)):
                continue  # not at the shared face / edge
            ch = tuple(2 * nb[d] + b[d] if d < dim else 0 for d in range(3))
            if _covering(active, dim, l + 1, ch) == -1:
                return True
    return False


def _children(dim, P):
    l, c = P[0], P[1:]
    return [(l + 1,) + tuple(2 * c[d] + ((k >> d) & 1) if d < dim else 0 for d in range(3)) for k in range(1 << dim)]


def coarsen_rule(dim, leaves):
    """sorted list of (level, cx, cy, cz) after one step"""
    active = {tuple(int(v) for v in l) for l in leaves}
    count = {}
    for (l, cx, cy, cz) in active:
        if l:
            key = (l - 1, cx >> 1, cy >> 1, cz >> 1)
            count[key] = count.get(key, 0) + 1
    parents = [P for P, k in count.items() if k == (1 << dim)]
    for P in parents:
        active -= set(_children(dim, P))
        active.add(P)
    changed = True
    while changed:
        changed = False
        for P in list(parents):
            if _touches_two_finer(active, dim, P):
                active.remove(P)
                active |= set(_children(dim, P))
                parents.remove(P)
                changed = True
    return sorted(active)


def coarsening_counts(dim, leaves):
    """cell counts of the whole sequence down to the root cell"""
    counts = [len(leaves)]
    while counts[-1] > 1:
        leaves = coarsen_rule(dim, leaves)
        counts.append(len(leaves))
    return counts


# ---- the transfer


def coarsening_map(coarse, fine):
    cl, fl = coarse.cell_levels().astype(np.int64), fine.cell_levels().astype(np.int64)
    index = {tuple(l): i for i, l in enumerate(cl)}
    parent, child = np.zeros(len(fl), dtype=np.int64), np.zeros(len(fl), dtype=np.int64)
    for f, (l, cx, cy, cz) in enumerate(fl):
        if (l, cx, cy, cz) in index:
            parent[f] = index[(l, cx, cy, cz)]
        else:
            parent[f] = index[(l - 1, cx >> 1, cy >> 1, cz >> 1)]
            child[f] = 1 + (cx & 1) + 2 * (cy & 1) + 4 * (cz & 1)
    return parent, child


def child_matrix(dim, p, child, p1=None):
    """kron over the directions of the lower / upper half of the 1D matrix [(2p+1), (p+1)]; identity for child 0"""
    nd = (p + 1) ** dim
    if not child:
        return np.eye(nd)
    P1 = o.mg_prolongation_1d(p) if p1 is None else np.asarray(p1, dtype=np.float64).reshape(2 * p + 1, p + 1)
    E = np.ones((1, 1))
    for d in range(dim):  # x fastest: kron(later, earlier)
        half = ((child - 1) >> d) & 1
        E = np.kron(P1[half * p:half * p + p + 1], E)
    return E


def gc_transfer_matrix(dim, p, coarse_arrays, fine_arrays, parent, child, coarse_mask, fine_mask, dirichlet, p1=None,
                       weights=None):
    (cd, n_coarse), (fd, n_fine) = coarse_arrays, fine_arrays
    nd = (p + 1) ** dim
    cd = np.asarray(cd, dtype=np.int64).reshape(-1, nd)
    fd = np.asarray(fd, dtype=np.int64).reshape(-1, nd)
    parent, child = np.asarray(parent, dtype=np.int64), np.asarray(child, dtype=np.int64)
    cm = np.zeros(len(cd), dtype=np.int64) if coarse_mask is None else np.asarray(coarse_mask, dtype=np.int64)
    w = hr.owners_hn(dim, p, fd, fine_mask, n_fine)
    pm = cm[parent]
    rows, cols, vals = [], [], []
    for ch, m in sorted(set(zip(child.tolist(), pm.tolist()))):  # fine cells grouped by (child, parent's mask)
        sel = (child == ch) & (pm == m)
        PC = child_matrix(dim, p, ch, p1) @ hr.resolve_matrix(dim, p, int(m), weights)
        rows.append(np.repeat(fd[sel], nd, axis=1).reshape(-1))
        cols.append(np.tile(cd[parent[sel]], (1, nd)).reshape(-1))
        vals.append((w[sel][:, :, None] * PC[None, :, :]).reshape(-1))
    P = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n_fine, n_coarse)).tocsr()
    free = np.ones(n_coarse)
    free[np.asarray(dirichlet, dtype=np.int64)] = 0.0
    return (P @ sp.diags(free)).tocsr()


def mesh_pair_matrix_gc(coarse, fine, dirichlet=None, p1=None, weights=None):
    """P of two leaf meshes of one degree (the coarse mesh's constrained dofs unless `dirichlet` is given)"""
    dim, p = int(coarse.desc.dim), int(coarse.desc.degree)
    assert p == int(fine.desc.degree)
    ca, fa = coarse.arrays(), fine.arrays()
    parent, child = coarsening_map(coarse, fine)
    con = ca["constrained_dofs"] if dirichlet is None else dirichlet
    return gc_transfer_matrix(dim, p, (ca["loc2glob"], coarse.n_dofs), (fa["loc2glob"], fine.n_dofs), parent, child,
                              ca["constraint_mask"], fa["constraint_mask"], con, p1, weights)


def mesh_pair_matrix(coarse, fine):
    if int(coarse.desc.degree) == int(fine.desc.degree):
        return mesh_pair_matrix_gc(coarse, fine)
    return hr.mesh_pair_matrix_hn(coarse, fine)


def level_hierarchy_gc(meshes64, lmax=None):
    """level_hierarchy_hn for coarsened meshes at one degree followed by the active mesh at rising degrees"""
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
