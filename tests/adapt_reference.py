"""float64 numpy restatement of adaptation in both directions for the tests; host only.  Written
from the definitions in include/mfgpu.h (mfgpu_mesh_adapt_leaves, mfgpu_transfer_interpolate), not from the product code.

  adapt_rule             one step of refinement and coarsening of a leaf set on sets of tuples: (new, mid) in output order
  interpolation_1d       J1[i][j] = phi_j(2 xi_i - b(i)), the child's 1D basis at the coarse nodes
  interpolation_matrix   the sparse J [n_coarse, n_fine] of a mesh pair: row coarse(K, i) of the owner K holds, for an
                         unchanged cell, row i of resolve_matrix(fine mask) on the fine cell's list; for a refined cell,
                         row i of kron(J1) @ resolve_matrix(fine mask of child k(i)) on that child's list.  The rows of
                         coarse Dirichlet dofs and of dofs no coarse cell owns are empty
  mark_refine_coarsen    the ceil(fr n) largest and the floor(fc n) smallest, ties to the lower index, never both
"""
import numpy as np
import scipy.sparse as sp

import amr_reference as ar
import gc_reference as gr
import pmg_hn_reference as hr
from oracle import mf_oracle as o


# ---- the rule


def adapt_rule(dim, leaves, refine, coarsen, balance_vertices=False):
    """(new, mid), lists of (level, cx, cy, cz).  ValueError where the library returns MFGPU_EINVAL"""
    leaves = [tuple(int(v) for v in l) for l in leaves]
    old = set(leaves)
    offsets = ar._offsets(dim, balance_vertices)
    # 1. R
    R = ar.refine_rule(dim, leaves, refine, balance_vertices)
    active = set(R)
    flag = {L: (bool(r), bool(c)) for L, r, c in zip(leaves, refine, coarsen)}
    # 2. the candidate families
    parents = set()
    for L in leaves:
        if L[0] == 0:
            continue
        Q = (L[0] - 1, L[1] >> 1, L[2] >> 1, L[3] >> 1)
        kids = gr._children(dim, Q)
        if all(k in old and flag[k][1] and not flag[k][0] and k in active for k in kids):
            parents.add(Q)
    # 3. replaced by their parents
    for Q in parents:
        active -= set(gr._children(dim, Q))
        active.add(Q)
    # 4. the rollback, in the relation of the closure
    changed = True
    while changed:
        changed = False
        for Q in sorted(parents):
            if ar._touched_by_two_finer(active, dim, Q, offsets):
                active.remove(Q)
                active |= set(gr._children(dim, Q))
                parents.remove(Q)
                changed = True
    new, mid = [], []
    for L in leaves:
        Q = (L[0] - 1, L[1] >> 1, L[2] >> 1, L[3] >> 1) if L[0] else None
        if Q in parents:
            if L == gr._children(dim, Q)[0]:
                new.append(Q)
                mid.append(Q)
            continue
        mid.append(L)
        new += [L] if L in active else gr._children(dim, L)
    assert set(new) == active and len(new) == len(active)
    return new, mid


def mark_refine_coarsen(eta, refine_fraction, coarsen_fraction):
    n = len(eta)
    refine = ar.mark_fixed_number(eta, refine_fraction)
    order = [i for i in sorted(range(n), key=lambda i: (float(eta[i]), i)) if not refine[i]]
    coarsen = np.zeros(n, dtype=np.uint8)
    coarsen[order[:int(np.floor(coarsen_fraction * n))]] = 1
    return refine, coarsen


# ---- the interpolation


def lower_half(p):
    """bool [p + 1]: xi_i <= 1/2"""
    return o.gll_01(p) <= 0.5


def interpolation_1d(p):
    nodes = o.gll_01(p)
    b = (~lower_half(p)).astype(np.float64)
    J1 = o.lagrange_eval(nodes, 2.0 * nodes - b)[0].T.copy()  # [i, j] = phi_j(2 xi_i - b(i))
    J1[np.abs(J1) < 1e-15] = 0.0  # a coarse node that is a node of the child
    J1[np.abs(J1 - 1.0) < 1e-15] = 1.0
    return J1


def child_of_position(dim, p):
    """int [(p+1)^dim], x fastest: k = sum_d b_d 2^d of the local position"""
    n = p + 1
    up = (~lower_half(p)).astype(np.int64)
    idx = np.stack(np.unravel_index(np.arange(n ** dim), (n,) * dim), axis=-1)[:, ::-1]  # [i, (x, y(, z))]
    return sum(up[idx[:, d]] << d for d in range(dim))


def interpolation_matrix(dim, p, coarse_arrays, fine_arrays, parent, child, coarse_mask, fine_mask, dirichlet, j1=None,
                         weights=None):
    (cd, n_coarse), (fd, n_fine) = coarse_arrays, fine_arrays
    nd = (p + 1) ** dim
    cd = np.asarray(cd, dtype=np.int64).reshape(-1, nd)
    fd = np.asarray(fd, dtype=np.int64).reshape(-1, nd)
    parent, child = np.asarray(parent, dtype=np.int64), np.asarray(child, dtype=np.int64)
    fm = np.zeros(len(fd), dtype=np.int64) if fine_mask is None else np.asarray(fine_mask, dtype=np.int64)
    own = hr.owners_hn(dim, p, cd, coarse_mask, n_coarse)  # 1 at the owner's entry
    free = np.ones(n_coarse)
    free[np.asarray(dirichlet, dtype=np.int64)] = 0.0
    own = own * free[cd]
    J1 = interpolation_1d(p) if j1 is None else np.asarray(j1, dtype=np.float64).reshape(p + 1, p + 1)
    JK = np.ones((1, 1))
    for d in range(dim):  # x fastest: kron(later, earlier)
        JK = np.kron(J1, JK)
    block = child_of_position(dim, p)
    rows, cols, vals = [], [], []
    for ch, m in sorted(set(zip(child.tolist(), fm.tolist()))):  # fine cells grouped by (child, own mask)
        sel = (child == ch) & (fm == m)
        C = hr.resolve_matrix(dim, p, int(m), weights)
        M = C if ch == 0 else (block == ch - 1)[:, None] * (JK @ C)
        w = own[parent[sel]]
        rows.append(np.repeat(cd[parent[sel]], nd, axis=1).reshape(-1))
        cols.append(np.tile(fd[sel], (1, nd)).reshape(-1))
        vals.append((w[:, :, None] * M[None, :, :]).reshape(-1))
    J = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n_coarse, n_fine))
    J = J.tocsr()
    J.eliminate_zeros()
    return J


def mesh_pair_interpolation(coarse, fine, dirichlet=None, j1=None, weights=None):
    """J of two leaf meshes of one degree (the coarse mesh's constrained dofs unless `dirichlet` is given)"""
    dim, p = int(coarse.desc.dim), int(coarse.desc.degree)
    assert p == int(fine.desc.degree)
    ca, fa = coarse.arrays(), fine.arrays()
    parent, child = gr.coarsening_map(coarse, fine)
    con = ca["constrained_dofs"] if dirichlet is None else dirichlet
    return interpolation_matrix(dim, p, (ca["loc2glob"], coarse.n_dofs), (fa["loc2glob"], fine.n_dofs), parent, child,
                                ca["constraint_mask"], fa["constraint_mask"], con, j1, weights)


def stored_rows(coarse, dirichlet=None):
    """bool [n_coarse]: the coarse dofs that interpolate stores: owned by a coarse cell and not Dirichlet"""
    ca = coarse.arrays()
    dim, p = int(coarse.desc.dim), int(coarse.desc.degree)
    cd = np.asarray(ca["loc2glob"], dtype=np.int64).reshape(-1, (p + 1) ** dim)
    own = hr.owners_hn(dim, p, cd, ca["constraint_mask"], coarse.n_dofs)
    out = np.zeros(coarse.n_dofs, dtype=bool)
    out[cd[own > 0]] = True
    out[np.asarray(ca["constrained_dofs"] if dirichlet is None else dirichlet, dtype=np.int64)] = False
    return out
