"""Description transforms for the tests (pure numpy on oracle.mf_oracle.Desc; never imports the product).

The C-ABI takes ANY cell-to-dof map as loc2glob.  The oracle defines A = sum_c P_c^T K_c P_c for any loc2glob (vmult,
vmult_add, compute_inverse_diagonal and assemble all scatter with np.add.at), so it is the reference for every
description made here; no geometry has to be truly periodic.

Every transform returns Transformed(desc, dof_map, cell_map):
  dof_map[old dof] = new dof  (a permutation for permute_*, many-to-one for periodic and pinch)
  cell_map[new cell] = old cell
pull(t, x_new) is the old-numbering vector that reads the new one through dof_map; push(t, x_old) carries a vector the
other way and exists for injective maps only (the permutations).

The transforms only touch loc2glob, the constrained list, the dof coordinates and the order of the per-cell arrays, so
they compose with util.deform (general geometry) in either order, except that periodic() needs the coordinates that
deform() drops: deform last.
"""
from collections import namedtuple

import numpy as np

from oracle import mf_oracle as o

Transformed = namedtuple("Transformed", "desc dof_map cell_map")


def _rebuild(od, n_dofs, loc2glob, constrained, dof_coords, cells=None):
    sel = slice(None) if cells is None else cells
    return o.Desc(od.dim, od.degree, n_dofs, loc2glob, od.JxW[sel], od.inv_jac[sel], od.coefficient[sel],
                  np.unique(np.asarray(constrained, dtype=np.int64)),
                  None if od.constraint_mask is None else od.constraint_mask[sel], od.dtype,
                  od.shape_values, od.shape_gradients, od.weights, dof_coords)


def _renumber(od, m, n_new, cells=None):
    """the description with dof g renamed m[g] (m need not be injective); coordinates: those of the lowest old dof"""
    m = np.asarray(m, dtype=np.int64)
    coords = None
    if od.dof_coords is not None:
        coords = np.zeros((n_new, od.dim))
        coords[m[::-1]] = od.dof_coords[::-1]
    l2g = m[od.loc2glob.astype(np.int64)]
    return _rebuild(od, n_new, l2g if cells is None else l2g[cells], m[od.constrained.astype(np.int64)], coords, cells)


def _compact(m):
    """m with its image renumbered densely, ascending; returns (m, size of the image)"""
    keep, inv = np.unique(m, return_inverse=True)
    return inv.reshape(-1).astype(np.int64), len(keep)


def pull(t, x_new):
    return np.asarray(x_new)[t.dof_map]


def push(t, x_old):
    x_old = np.asarray(x_old)
    assert len(np.unique(t.dof_map)) == len(t.dof_map) == len(x_old), "push needs an injective dof map"
    out = np.zeros(t.desc.n_dofs, dtype=x_old.dtype)
    out[t.dof_map] = x_old
    return out


def periodic(od, axes, compact=True):
    """Identify each dof on the hi face of every axis in `axes` of an o.uniform_mesh_desc box with its partner on the lo
    face (matched by coordinates; the axes one after the other, so edges and corners collapse transitively).  The
    constrained set becomes exactly the dofs on the faces that remain boundary.  compact=False keeps the dropped ids as
    holes: dofs no cell touches and that are not constrained."""
    X = od.dof_coords
    assert X is not None and od.constraint_mask is None
    N, dim = od.n_dofs, od.dim
    key = np.round((X - X.min(0)) / (X.max(0) - X.min(0)).max() * 2 ** 30).astype(np.int64)  # exact comparisons
    lo, hi = key.min(0), key.max(0)
    m = np.arange(N, dtype=np.int64)
    for a in axes:
        other = [d for d in range(dim) if d != a]

        def face(v):
            idx = np.nonzero(key[:, a] == v)[0]
            return idx[np.lexsort(key[idx][:, other].T)] if other else idx

        f_lo, f_hi = face(lo[a]), face(hi[a])
        assert len(f_lo) == len(f_hi) and np.array_equal(key[f_lo][:, other], key[f_hi][:, other])
        r = np.arange(N, dtype=np.int64)
        r[f_hi] = f_lo
        m = r[m]
    on_boundary = np.zeros(N, dtype=bool)
    for d in range(dim):
        if d not in axes:
            on_boundary |= (key[:, d] == lo[d]) | (key[:, d] == hi[d])
    n_new = N
    if compact:
        m, n_new = _compact(m)
    coords = np.zeros((n_new, dim))
    coords[m[::-1]] = X[::-1]
    nd = _rebuild(od, n_new, m[od.loc2glob.astype(np.int64)], m[np.nonzero(on_boundary)[0]], coords)
    return Transformed(nd, m, np.arange(od.n_cells))


def permute_dofs(od, seed):
    """a random renumbering of the dofs"""
    m = np.random.default_rng(seed).permutation(od.n_dofs).astype(np.int64)
    return Transformed(_renumber(od, m, od.n_dofs), m, np.arange(od.n_cells))


def permute_cells(od, seed):
    """a random reordering of the cells; loc2glob, JxW, inv_jac, coefficient and constraint_mask move with their cell"""
    cells = np.random.default_rng(seed).permutation(od.n_cells)
    m = np.arange(od.n_dofs, dtype=np.int64)
    return Transformed(_renumber(od, m, od.n_dofs, cells), m, cells)


def pinch(od, dofs):
    """identify the listed free dofs into one (a vertex of arbitrary valence); dense renumbering"""
    dofs = np.unique(np.asarray(dofs, dtype=np.int64))
    assert len(dofs) >= 2 and not np.isin(dofs, od.constrained).any()
    m = np.arange(od.n_dofs, dtype=np.int64)
    m[dofs] = dofs[0]
    m, n_new = _compact(m)
    return Transformed(_renumber(od, m, n_new), m, np.arange(od.n_cells))


def interior_vertices(od):
    """the dofs at cell corners in the interior of an o.uniform_mesh_desc box"""
    n, dim = od.n, od.dim
    corners = [sum((n - 1) * ((k >> d) & 1) * n ** d for d in range(dim)) for k in range(1 << dim)]
    v = np.unique(od.loc2glob[:, corners])
    return v[~np.isin(v, od.constrained)]
