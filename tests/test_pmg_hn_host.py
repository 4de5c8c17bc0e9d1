"""CPU: the owner rule of the p-transfer on meshes with hanging nodes (mfgpu_transfer_p_owner_list, the list
mfgpu_transfer_create_p_hn uploads) against tests/pmg_hn_reference.py, and the reference's own P
against a known answer, on the seven meshes of test_hanging_host.py."""
import numpy as np
import pytest

import pmg_hn_reference as hr
import pmg_reference as pr
import pymfgpu as mf
from test_hanging_host import CASES

PAIRS = [(1, 2), (2, 4), (2, 3)]
BIT31 = np.uint32(0x80000000)


def mesh_of(name, p):
    dim, leaves = CASES[name]
    return dim, mf.Mesh.from_leaves(dim, p, leaves)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("pc,pf", PAIRS)
def test_owner_list_is_the_reference_rule(name, pc, pf):
    dim, fine = mesh_of(name, pf)
    a = fine.arrays()
    fd, mask = a["loc2glob"], a["constraint_mask"]
    assert mask is not None and (mask != 0).any()
    got = mf.p_owner_list(dim, pf, fd, fine.n_dofs, mask)
    np.testing.assert_array_equal(got & ~BIT31, fd)  # the indices themselves are untouched
    owned = (got & BIT31) == 0
    np.testing.assert_array_equal(owned, hr.owners_hn(dim, pf, fd, mask, fine.n_dofs) == 1.0)
    # every listed fine dof has exactly one owner, at a position that is not constrained
    count = np.bincount(fd[owned].astype(np.int64), minlength=fine.n_dofs)
    listed = np.bincount(fd.reshape(-1).astype(np.int64), minlength=fine.n_dofs) > 0
    np.testing.assert_array_equal(count, listed.astype(count.dtype))
    constrained = np.stack([hr.constrained_positions(dim, pf, int(m)) for m in mask])
    assert constrained.any() and not (owned & constrained).any()
    # the dofs without an owner are the ones no cell lists: the hanging dofs, all of them constrained dofs
    con = np.zeros(fine.n_dofs, dtype=bool)
    con[a["constrained_dofs"]] = True
    assert (~listed).any() and con[~listed].all()
    np.testing.assert_array_equal(count == 0, ~listed)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("pc,pf", PAIRS)
def test_reference_p_reproduces_polynomials_of_the_coarse_degree(name, pc, pf):
    dim, coarse = mesh_of(name, pc)
    _, fine = mesh_of(name, pf)
    P = hr.mesh_pair_matrix_hn(coarse, fine, dirichlet=[])
    coef = np.random.default_rng(10 * pc + pf).uniform(0.5, 1.5, (dim, pc + 1))

    def poly(X):  # degree pc per direction
        return np.prod([np.polyval(coef[d], X[:, d]) for d in range(dim)], axis=0)

    fa = fine.arrays()
    owned = (mf.p_owner_list(dim, pf, fa["loc2glob"], fine.n_dofs, fa["constraint_mask"]) & BIT31) == 0
    sel = np.zeros(fine.n_dofs, dtype=bool)
    sel[fa["loc2glob"][owned]] = True
    got, want = P @ poly(coarse.dof_coords()), poly(fine.dof_coords())
    err = np.linalg.norm(got[sel] - want[sel]) / np.linalg.norm(want[sel])
    print(f"{name} ({pc} -> {pf}): rel l2 at the {sel.sum()} owned fine dofs {err:.2e}")
    assert err <= 1e-13
    assert not got[~sel].any()  # rows of the fine dofs no cell lists are empty
    hanging = np.setdiff1d(np.arange(coarse.n_dofs), coarse.arrays()["loc2glob"].reshape(-1))
    assert len(hanging) and P[:, hanging].nnz == 0  # columns of the coarse hanging dofs are exactly zero


@pytest.mark.parametrize("name", ["2d_L", "3d_corner"])
@pytest.mark.parametrize("pf", [2, 3, 4])
def test_without_a_mask_the_first_lister_owns(name, pf):
    dim, fine = mesh_of(name, pf)
    fd = fine.arrays()["loc2glob"]
    want = pr.owners(fd, fine.n_dofs) == 1.0
    for mask in (None, np.zeros(fine.n_cells, dtype=np.uint32)):
        got = mf.p_owner_list(dim, pf, fd, fine.n_dofs, mask)
        np.testing.assert_array_equal((got & BIT31) == 0, want)
        np.testing.assert_array_equal(got & ~BIT31, fd)


def test_owner_list_errors():
    dim, fine = mesh_of("2d_corner", 2)
    a = fine.arrays()
    fd, mask, N = a["loc2glob"], a["constraint_mask"].copy(), fine.n_dofs
    out = np.zeros_like(fd)
    f = mf.lib().mfgpu_transfer_p_owner_list

    def rc(dim=2, pf=2, n=fine.n_cells, fd=fd, mask=mask, N=N, out=out):
        return f(dim, pf, n, None if fd is None else fd.ctypes.data, None if mask is None else mask.ctypes.data, N,
                 None if out is None else out.ctypes.data)

    assert rc() == 0 and rc(mask=None) == 0
    assert rc(fd=None) == mf.EINVAL and rc(out=None) == mf.EINVAL          # null arrays
    assert rc(dim=1) == mf.EINVAL and rc(dim=4) == mf.EINVAL
    assert rc(pf=0) == mf.EINVAL and rc(pf=7) == mf.EINVAL
    assert rc(N=N - 1) == mf.EINVAL and rc(N=1 << 31) == mf.EINVAL         # a dof out of range, dof counts >= 2^31
    bad = mask.copy()
    bad[0] |= 1 << 9
    assert rc(mask=bad) == mf.EINVAL                                       # a bit outside the 9 defined ones
    for bit in (2, 5, 6, 7, 8):                                            # TYPE z, FACE z, the EDGE bits: 3D only
        bad = mask.copy()
        bad[0] |= 1 << bit
        assert rc(mask=bad) == mf.EINVAL, bit
    # two cells that share a face and both flag it: the dofs inside that face are listed but have no owner
    two = mf.Mesh.uniform(2, 2, (2, 1))
    fd2 = two.arrays()["loc2glob"]
    both = np.array([1 << 3, (1 << 3) | 1], dtype=np.uint32)  # FACE x on both; cell 0 at x = p, cell 1 (TYPE x) at x = 0
    out2 = np.zeros_like(fd2)
    assert f(2, 2, 2, fd2.ctypes.data, both.ctypes.data, two.n_dofs, out2.ctypes.data) == mf.EINVAL
    one = np.array([1 << 3, 0], dtype=np.uint32)              # flagged on one side only: the neighbour owns the face
    assert f(2, 2, 2, fd2.ctypes.data, one.ctypes.data, two.n_dofs, out2.ctypes.data) == 0
    face = fd2[0].reshape(3, 3)[:, 2]
    np.testing.assert_array_equal(out2[0].reshape(3, 3)[:, 2], face | BIT31)
    np.testing.assert_array_equal(out2[1].reshape(3, 3)[:, 0], face)
