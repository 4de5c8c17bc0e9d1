"""float64 numpy restatement of adaptive refinement for the tests; host only.  Written from the
definition in include/mfgpu.h (mfgpu_integrator_recovery_indicator, mfgpu_mesh_refine_leaves), not from the kernels.

  refine_rule            one refinement step of a leaf set on sets of tuples: split the flagged leaves; then, until nothing
                         changes, split every leaf that a leaf two or more levels finer touches (faces, 3D edges; with
                         balance_vertices also vertices), on an input that is one-irregular in that relation.  Returns
                         the leaves in output order
  constrained_positions  the local positions on a constrained face / edge of a cell, from the mask bits
  recovery_indicator     steps a-c on poisson_reference.Cells (dense tables; small meshes only)
  amr_loop               a CPU model of solve -> estimate -> mark -> refine with a scipy sparse solve on the oracle's matrices
"""
import numpy as np

import gc_reference as gr
import nonlinear_reference as nr
import poisson_reference as pr
import pymfgpu as mf
from oracle import mf_oracle as o


# ---- the refinement rule


def _offsets(dim, vertices):
    out = []
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in ((-1, 0, 1) if dim == 3 else (0,)):
                nz = (ox != 0) + (oy != 0) + (oz != 0)
                if nz == 0 or (nz == dim and not vertices):
                    continue
                out.append((ox, oy, oz))
    return out


def _touched_by_two_finer(active, dim, M, offsets):
    """does a leaf of level >= level(M) + 2 touch the leaf M over one of the offsets?"""
    l, c = M[0], M[1:]
    for o_ in offsets:
        nb = tuple(c[d] + o_[d] for d in range(3))
        if gr._covering(active, dim, l, nb) != -1:
            continue  # outside, or a leaf of M's level or coarser
        for k in range(1 << dim):  # the neighbour's children that touch M: refined themselves?
            b = [(k >> d) & 1 for d in range(dim)] + [0] * (3 - dim)
            if any((o_[d] == 1 and b[d] != 0) or (o_[d] == -1 and b[d] != 1) for d in range(dim)):
                continue
            ch = tuple(2 * nb[d] + b[d] if d < dim else 0 for d in range(3))
            if gr._covering(active, dim, l + 1, ch) == -1:
                return True
    return False


def one_irregular(dim, leaves, vertices=False):
    """no leaf touches a leaf two or more levels coarser over a face, a 3D edge or (with `vertices`) a vertex"""
    active = {tuple(int(v) for v in l) for l in leaves}
    for (l, cx, cy, cz) in active:
        for o_ in _offsets(dim, vertices):
            if 0 <= gr._covering(active, dim, l, (cx + o_[0], cy + o_[1], cz + o_[2])) < l - 1:
                return False
    return True


def refine_rule(dim, leaves, flags, balance_vertices=False):
    """list of (level, cx, cy, cz): the input order, the children of a split leaf in its place in child order.  The input
    must be one-irregular in the relation of the closure (with balance_vertices over vertices too): ValueError otherwise,
    where the library returns MFGPU_EINVAL"""
    leaves = [tuple(int(v) for v in l) for l in leaves]
    active = set(leaves)
    offsets = _offsets(dim, balance_vertices)
    if not one_irregular(dim, leaves, balance_vertices):
        raise ValueError("refine_rule: the input is not one-irregular in the relation of the closure")
    for L, f in zip(leaves, flags):
        if f:
            active.remove(L)
            active |= set(gr._children(dim, L))
    changed = True
    while changed:
        changed = False
        for M in sorted(active):
            if _touched_by_two_finer(active, dim, M, offsets):
                active.remove(M)
                active |= set(gr._children(dim, M))
                changed = True
    out = []
    for L in leaves:
        if L in active:
            out.append(L)
        else:
            kids = gr._children(dim, L)
            assert all(k in active for k in kids), "no leaf splits twice"
            out += kids
    assert len(out) == len(active)
    return out


def mark_fixed_number(eta, fraction):
    """the ceil(fraction n) largest, ties to the lower index"""
    n = len(eta)
    k = min(n, int(np.ceil(fraction * n)))
    order = sorted(range(n), key=lambda i: (-float(eta[i]), i))
    flags = np.zeros(n, dtype=np.uint8)
    flags[order[:k]] = 1
    return flags


# ---- the indicator


def constrained_positions(dim, p, mask):
    """bool [(p+1)^dim], x fastest: on a constrained face or (3D) edge of a cell with this mask"""
    n = p + 1
    idx = np.stack(np.unravel_index(np.arange(n ** dim), (n,) * dim), axis=-1)[:, ::-1]  # [i, (x, y(, z))]
    at = [idx[:, d] == (0 if mask & (1 << d) else p) for d in range(dim)]
    con = np.zeros(n ** dim, dtype=bool)
    for d in range(dim):
        if mask & (1 << (3 + d)):
            con |= at[d]
    if dim == 3:
        for e, bit in enumerate((1 << 7, 1 << 8, 1 << 6)):  # edges along x, y, z
            if mask & bit:
                con |= at[(e + 1) % 3] & at[(e + 2) % 3]
    return con


def recovery_indicator(cells: "pr.Cells", u, weight=None, parts=False):
    """eta_K^2 [n_cells]; with parts also (grad u_h [cell, q, dim], G [n_dofs, dim])"""
    od, dim, p = cells.od, cells.dim, cells.p
    nc, nd = od.n_cells, od.nd
    jxw = od.JxW.astype(np.float64).reshape(nc, nd)
    # a. the cell gradient at the quadrature points and its nodal coefficients
    _, grads = nr.evaluate(cells, u)
    T1 = np.linalg.inv(o.shape_info(p)[0].reshape(p + 1, p + 1).T)  # [i, q], inverse of [q, i] = phi_i(x_q) (pivoted LU)
    T = pr._kron_tables([T1] * dim)
    g = np.einsum("iq,cqk->cik", T, grads)
    # b. the nodal average
    vol = jxw.sum(axis=1)
    num, den = np.zeros((od.n_dofs, dim)), np.zeros(od.n_dofs)
    for c in range(nc):
        mask = 0 if od.constraint_mask is None else int(od.constraint_mask[c])
        free = ~constrained_positions(dim, p, mask)
        np.add.at(num, od.loc2glob[c][free], vol[c] * g[c][free])
        np.add.at(den, od.loc2glob[c][free], vol[c])
    G = np.where(den[:, None] > 0, num / np.where(den > 0, den, 1.0)[:, None], 0.0)
    # c. the cell indicator
    w = jxw if weight is None else jxw * np.asarray(weight, np.float64).reshape(nc, nd)
    eta = np.zeros(nc)
    for c in range(nc):
        Gq = np.stack([cells.Phi @ cells._hn(c, G[od.loc2glob[c], k], False) for k in range(dim)], axis=-1)
        eta[c] = np.sum(np.sum((Gq - grads[c]) ** 2, axis=-1) * w[c])
    return (eta, grads, G) if parts else eta


# ---- the loop on the CPU


def amr_loop(dim, p, start_level, n_cycles, fraction):
    """[(leaves, l2 error, eta)] per cycle: uniform start mesh of `start_level`, the reference's Poisson problem solved
    by a sparse direct solve, the indicator with weight 1, fixed-number marking, refine_rule"""
    leaves = pr.refined_leaves([[0, 0, 0, 0]], dim, start_level)
    out = []
    for _ in range(n_cycles):
        cells = pr.Cells(mf.Mesh.from_leaves(dim, p, leaves))
        leaves = cells.mesh.cell_levels()
        u, l2 = cells.solve()
        eta = recovery_indicator(cells, u)
        out.append((leaves, l2, float(np.sqrt(eta.sum()))))
        leaves = np.array(refine_rule(dim, leaves, mark_fixed_number(eta, fraction)), dtype=np.uint32)
    return out
