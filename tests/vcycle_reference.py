"""tests/mg_reference.py's Hierarchy filled for GLOBALLY refined hierarchies: uniform cubes of n, 2n, 4n ... cells per
direction or balls of successive n_ref.  No refinement edges, the active vector is the finest level's (identity copy pairs
on the top level, none below), transfer patches from Mesh.transfer_patches; the matrices are then those of
Hierarchy.build_matrices(), so Hierarchy.vcycle and Hierarchy.chebyshev run unchanged.  Host only."""
import numpy as np

import mg_reference as mg
import pymfgpu as mf
from util import oracle_desc_from_mesh


def global_hierarchy(meshes64, matrices=True):
    """meshes64: the level meshes in double, coarse to fine"""
    H = mg.Hierarchy.__new__(mg.Hierarchy)
    H.dim, H.p = int(meshes64[0].desc.dim), int(meshes64[0].desc.degree)
    H.mesh, H.H = meshes64[-1], None
    H.n_levels = len(meshes64)
    H.meshes = list(meshes64)
    H.od = [oracle_desc_from_mesh(M, dtype=np.float64) for M in meshes64]
    none = np.zeros(0, dtype=np.uint32)
    H.edge = [none for _ in meshes64]
    H.odc = [mg.with_constrained(od, od.constrained) for od in H.od]
    ident = np.arange(meshes64[-1].n_dofs, dtype=np.uint32)
    H.pairs = [(none, none) for _ in meshes64[:-1]] + [(ident, ident)]
    H.patches = [None] + [meshes64[l - 1].transfer_patches(meshes64[l]) for l in range(1, H.n_levels)]
    if matrices:
        H.build_matrices()
    return H


def cube_meshes(dim, p, cells, number_type=mf.F64):
    return [mf.Mesh.uniform(dim, p, n, number_type=number_type) for n in cells]


def ball_meshes(dim, p, n_refs, number_type=mf.F64):
    return [mf.Mesh.ball(dim, p, r, number_type=number_type) for r in n_refs]
