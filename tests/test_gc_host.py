"""CPU: the host side of global-coarsening multigrid: one coarsening step of a leaf set
(mfgpu_mesh_coarsen_leaves) against the pure-Python rule of tests/gc_reference.py, the map between two leaf meshes
(mfgpu_mesh_coarsening_map), the error cases, and the numpy P of gc_reference.py by what it must do: reproduce polynomials
of degree p per direction at every fine dof that is not hanging."""
import numpy as np
import pytest

import gc_reference as gr
import pymfgpu as mf
from test_hanging_host import CASES, leaves_refine


def as_set(leaves):
    return sorted(tuple(int(v) for v in l) for l in leaves)


def sequence(dim, leaves):
    """every step of the C++ coarsening down to the root cell"""
    out = [np.asarray(leaves, dtype=np.uint32).reshape(-1, 4)]
    while len(out[-1]) > 1:
        out.append(mf.Mesh.coarsen_leaves(dim, out[-1]))
        assert len(out[-1]) < len(out[-2])
    return out


def maximal(dim, fine, coarse):
    """no family that was complete in `fine` and is still there in `coarse` (rolled back) could be coarsened without
    breaking one-irregularity"""
    before, active = set(as_set(fine)), set(as_set(coarse))
    for P in {(l - 1, cx >> 1, cy >> 1, cz >> 1) for (l, cx, cy, cz) in active if l}:
        kids = set(gr._children(dim, P))
        if kids <= active and kids <= before and gr.one_irregular(dim, (active - kids) | {P}):
            return False
    return True


@pytest.mark.parametrize("name", sorted(CASES))
def test_coarsening_equals_the_python_rule_on_the_small_cases(name):
    dim, leaves = CASES[name]
    seq = sequence(dim, leaves)
    for fine, coarse in zip(seq, seq[1:]):
        assert as_set(coarse) == gr.coarsen_rule(dim, fine)
        assert gr.one_irregular(dim, coarse)
        assert maximal(dim, fine, coarse)
        mf.Mesh.from_leaves(dim, 1, coarse)  # accepted
    assert as_set(seq[-1]) == [(0, 0, 0, 0)]


COUNTS_3D = {4: [736, 253, 78, 22, 8, 1], 5: [33797, 7099, 1870, 589, 267, 92, 36, 8, 1]}


@pytest.mark.parametrize("dim,n_ref", [(2, 3), (2, 4), (2, 5), (3, 4), (3, 5)])
def test_coarsening_of_the_adaptive_recipe(dim, n_ref):
    mesh = mf.Mesh.adaptive(dim, 1, n_ref)
    seq = sequence(dim, mesh.cell_levels())
    counts = [len(s) for s in seq]
    print(f"adaptive {dim}D n_ref {n_ref}: cells per step {counts}, sum / finest {sum(counts) / counts[0]:.2f}")
    if dim == 3:
        assert counts == COUNTS_3D[n_ref]
    check_python = dim == 2 or n_ref == 4  # (the Python rule on 33 797 leaves takes a minute)
    if check_python:
        assert counts == gr.coarsening_counts(dim, seq[0])
    for fine, coarse in zip(seq, seq[1:]):
        if check_python:
            assert as_set(coarse) == gr.coarsen_rule(dim, fine)
            assert gr.one_irregular(dim, coarse)
        if len(coarse) <= 2000:
            assert maximal(dim, fine, coarse)
        assert mf.Mesh.from_leaves(dim, 1, coarse).n_cells == len(coarse)  # (from_leaves refuses what is not one-irregular)


def test_coarsening_sequence_of_meshes():
    mesh = mf.Mesh.adaptive(3, 2, 4, number_type=mf.F32)
    seq = mf.Mesh.coarsening_sequence(mesh)
    assert [M.n_cells for M in seq] == COUNTS_3D[4][-2::-1] and seq[-1] is mesh
    assert all(int(M.desc.degree) == 2 and int(M.desc.number_type) == mf.F32 for M in seq)
    seq = mf.Mesh.coarsening_sequence(mesh, degree=1, min_cells=20)
    assert [M.n_cells for M in seq] == [22, 78, 253, 736] and seq[-1] is not mesh
    assert all(int(M.desc.degree) == 1 for M in seq)
    np.testing.assert_array_equal(seq[-1].cell_levels(), mesh.cell_levels())
    with pytest.raises(mf.MfgpuError):
        mf.Mesh.coarsening_sequence(mf.Mesh.uniform(3, 1, 4))


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_map_finds_every_fine_leaf(name):
    dim, leaves = CASES[name]
    fine = mf.Mesh.from_leaves(dim, 1, leaves)
    coarse = mf.Mesh.from_leaves(dim, 1, mf.Mesh.coarsen_leaves(dim, leaves))
    parent, child = mf.coarsening_map(coarse, fine)
    cl, fl = coarse.cell_levels().astype(np.int64), fine.cell_levels().astype(np.int64)
    assert len(parent) == fine.n_cells and parent.max() < coarse.n_cells and child.max() <= 2 ** dim
    same = child == 0
    np.testing.assert_array_equal(cl[parent[same]], fl[same])
    kids = fl[~same]
    np.testing.assert_array_equal(cl[parent[~same]][:, 0] + 1, kids[:, 0])
    np.testing.assert_array_equal(cl[parent[~same]][:, 1:], kids[:, 1:] >> 1)
    k = child[~same].astype(np.int64) - 1
    for d in range(3):  # bit d of k: the upper half in direction d
        np.testing.assert_array_equal((k >> d) & 1, kids[:, 1 + d] & 1)
    want_p, want_c = gr.coarsening_map(coarse, fine)
    np.testing.assert_array_equal(parent, want_p)
    np.testing.assert_array_equal(child, want_c)
    # every refined parent has all its 2^dim children, each once
    refined, n = np.unique(parent[~same], return_counts=True)
    assert (n == 2 ** dim).all() and not np.intersect1d(refined, parent[same]).size
    # a mesh against itself: all the same cell
    parent, child = mf.coarsening_map(fine, fine)
    np.testing.assert_array_equal(parent, np.arange(fine.n_cells))
    assert not child.any()


def test_errors():
    def raises(fn, *args):
        with pytest.raises(mf.MfgpuError) as e:
            fn(*args)
        assert e.value.code == mf.EINVAL, str(e.value)

    raises(mf.Mesh.coarsen_leaves, 2, [[0, 0, 0, 0]])                      # the single root cell
    raises(mf.Mesh.coarsen_leaves, 3, [[0, 0, 0, 0]])
    raises(mf.Mesh.coarsen_leaves, 4, CASES["2d_corner"][1])               # dim
    raises(mf.Mesh.coarsen_leaves, 2, np.zeros((0, 4)))
    ok = leaves_refine(2, 1, [(0, 0)])
    raises(mf.Mesh.coarsen_leaves, 2, ok[:-1])                             # a hole
    raises(mf.Mesh.coarsen_leaves, 2, ok + [ok[0]])                        # a leaf twice
    raises(mf.Mesh.coarsen_leaves, 2, ok + [[1, 0, 0, 0]])                 # a leaf inside another
    raises(mf.Mesh.coarsen_leaves, 2, ok[:-1] + [[1, 2, 1, 0]])            # outside the root cell
    raises(mf.Mesh.coarsen_leaves, 2, ok[:-1] + [[1, 1, 1, 1]])            # a z coordinate in 2D
    # level 1 next to level 3 over a face: a partition that is not one-irregular
    bad = [l for l in leaves_refine(2, 1, [(0, 0)]) if l != [2, 1, 1, 0]] + [[3, 2 + i, 2 + j, 0] for i in (0, 1) for j in (0, 1)]
    assert not gr.one_irregular(2, bad)
    raises(mf.Mesh.coarsen_leaves, 2, bad)
    # 3D: level 1 across an EDGE from level 3 (the faces are fine)
    # of 3d_edge: the level-2 cell (1, 2, 0) has level-2 face neighbours and the level-1 cell (1, 0, 0) across a z-edge
    base = CASES["3d_edge"][1]
    assert [2, 1, 2, 0] in base and [2, 2, 2, 0] in base and [2, 1, 1, 0] in base and [1, 1, 0, 0] in base
    edge = [l for l in base if l != [2, 1, 2, 0]] + [[3, 2 + i, 4 + j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    assert len(edge) == len(base) + 7 and not gr.one_irregular(3, edge)
    raises(mf.Mesh.coarsen_leaves, 3, edge)
    # the map
    c2, f2 = mf.Mesh.from_leaves(2, 1, CASES["2d_corner"][1]), mf.Mesh.from_leaves(2, 1, CASES["2d_L"][1])
    c3 = mf.Mesh.from_leaves(3, 1, CASES["3d_corner"][1])
    raises(mf.coarsening_map, c3, f2)                                      # the meshes differ in dim
    raises(mf.coarsening_map, f2, c2)                                      # a fine leaf that is two levels above a coarse one
    raises(mf.coarsening_map, mf.Mesh.from_leaves(2, 1, [[0, 0, 0, 0]]), f2)  # grandchildren
    raises(mf.coarsening_map, mf.Mesh.uniform(2, 1, 2), c2)                # not a leaf mesh
    mf.coarsening_map(mf.Mesh.from_leaves(2, 1, [[0, 0, 0, 0]]), mf.Mesh.from_leaves(2, 1, leaves_refine(2, 0, [(0, 0)])))


@pytest.mark.parametrize("p", [1, 2, 4])
@pytest.mark.parametrize("name", ["2d_center", "2d_L", "3d_edge", "3d_two"])
def test_the_numpy_P_reproduces_polynomials(name, p):
    dim, leaves = CASES[name]
    fine = mf.Mesh.from_leaves(dim, p, leaves)
    coarse = mf.Mesh.from_leaves(dim, p, mf.Mesh.coarsen_leaves(dim, leaves))
    P = gr.mesh_pair_matrix_gc(coarse, fine, dirichlet=np.zeros(0, dtype=np.int64))
    coef = np.random.default_rng(10 * p + dim).uniform(0.5, 1.5, (dim, p + 1))

    def poly(X):  # degree p per direction
        return np.prod([np.polyval(coef[d], X[:, d]) for d in range(dim)], axis=0)

    listed = np.zeros(fine.n_dofs, dtype=bool)
    listed[fine.arrays()["loc2glob"].reshape(-1)] = True
    got, want = P @ poly(coarse.dof_coords()), poly(fine.dof_coords())
    assert listed.sum() < fine.n_dofs and not got[~listed].any()
    err = np.linalg.norm(got[listed] - want[listed]) / np.linalg.norm(want[listed])
    print(f"{name} p = {p}: {coarse.n_cells} -> {fine.n_cells} cells, rel l2 at the {listed.sum()} dofs that are not hanging {err:.2e}")
    assert err <= 1e-13
