"""Host-side premise of the mixed-precision multigrid (host/mfgpu_shim_mg.h, MGDoFHandler::distribute_mg_dofs with a
level and an active number type): the mesh generators number a float and a double mesh of the same recipe
identically, so the level hierarchy built from the float active mesh and the double active mesh built again next to
it share every index.  Uniform cubes, balls and the vertex-balanced adaptive recipe at p = 2 and 4 in 2D and 3D; on
the adaptive meshes also the hierarchies' level meshes, refinement-edge dofs, copy pairs and transfer arrays."""
import numpy as np
import pytest

import pymfgpu as mf


def _same_numbering(a: "mf.Mesh", b: "mf.Mesh"):
    assert a.desc.number_type != b.desc.number_type
    assert a.n_dofs == b.n_dofs and a.n_cells == b.n_cells
    A, B = a.arrays(), b.arrays()
    np.testing.assert_array_equal(A["loc2glob"], B["loc2glob"])
    np.testing.assert_array_equal(A["constrained_dofs"], B["constrained_dofs"])
    assert (A["constraint_mask"] is None) == (B["constraint_mask"] is None)
    if A["constraint_mask"] is not None:
        np.testing.assert_array_equal(A["constraint_mask"], B["constraint_mask"])


@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("dim,n", [(2, 8), (3, 4)])
def test_uniform_meshes_number_alike_in_both_types(dim, p, n):
    _same_numbering(mf.Mesh.uniform(dim, p, n, number_type=mf.F32), mf.Mesh.uniform(dim, p, n, number_type=mf.F64))


@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("dim,nref", [(2, 3), (3, 1)])
def test_ball_meshes_number_alike_in_both_types(dim, p, nref):
    _same_numbering(mf.Mesh.ball(dim, p, nref, number_type=mf.F32), mf.Mesh.ball(dim, p, nref, number_type=mf.F64))


@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("dim,nref", [(2, 4), (3, 3)])
def test_adaptive_mg_hierarchies_agree_in_both_types(dim, p, nref):
    m32 = mf.Mesh.adaptive_mg(dim, p, nref, number_type=mf.F32)
    m64 = mf.Mesh.adaptive_mg(dim, p, nref, number_type=mf.F64)
    _same_numbering(m32, m64)
    np.testing.assert_array_equal(m32.cell_levels(), m64.cell_levels())
    H32, H64 = mf.MgHierarchy(m32), mf.MgHierarchy(m64)
    assert H32.n_levels == H64.n_levels >= 2
    nd, nfd = (p + 1) ** dim, (2 * p + 1) ** dim
    for l in range(H32.n_levels):
        L32, L64 = H32.level_mesh(l), H64.level_mesh(l)
        assert L32.desc.number_type == mf.F32 and L64.desc.number_type == mf.F64
        _same_numbering(L32, L64)
        np.testing.assert_array_equal(H32.edge_dofs(l), H64.edge_dofs(l))
        for a, b in zip(H32.copy_pairs(l), H64.copy_pairs(l)):
            np.testing.assert_array_equal(a, b)
        if l > 0:
            for a, b in zip(H32.transfer_arrays(l, nd, nfd), H64.transfer_arrays(l, nd, nfd)):
                np.testing.assert_array_equal(a, b)
