"""The five transfer kinds, the level operator with its interface matrices and the index pairs on vectors inside red
zones (tests/redzone.py; the operator is in test_gpu_redzone.py).  Both vectors of a transfer are zoned -- they have
different lengths -- and every call runs 16-byte aligned and one element off, in double and in float.

References and tolerances are those of the entry points' own test files: the sparse P of mg_reference (from_meshes, the
hierarchy's level pairs), pmg_reference (p_from_meshes), pmg_hn_reference (p_hn_from_meshes) and gc_reference
(h_hn_from_meshes) with TRANSFER_TOL of test_gpu_pmg.py (1e-13 / 1e-5, also test_gpu_transfer.py's); the oracle's level
matrix and interface matrices with TOL of test_gpu.py; numpy indexing, bit for bit, for the pairs.  The matrices are
built once per mesh pair in double and shared by the four variants of a case."""
import functools

import numpy as np
import pytest

import gc_reference as gr
import mg_reference as mg
import pmg_hn_reference as hnr
import pmg_reference as pr
import pymfgpu as mf
from oracle import mf_oracle as o
from redzone import Zoned
from test_gpu import TOL
from test_gpu_pmg import TRANSFER_TOL, mesh_pair, rel
from util import oracle_desc_from_mesh

pytestmark = pytest.mark.gpu

F64, F32 = mf.F64, mf.F32
ALIGN = pytest.mark.parametrize("offset_one", [False, True], ids=["aligned", "offset"])
TYPES = pytest.mark.parametrize("nt", [F64, F32], ids=["f64", "f32"])


def typed(a, nt):
    return np.asarray(a).astype(mf.np_dtype(nt)).astype(np.float64)


def check_transfer(t, P, con, nt, offset_one):
    """prolongate, prolongate_add and restrict_and_add of t against the sparse P [n_fine, n_coarse]"""
    tol = TRANSFER_TOL[nt]
    nf, nc = P.shape
    rng = np.random.default_rng(nf * 1000 + nc)
    x, y, z = (typed(rng.standard_normal(n), nt) for n in (nc, nf, nc))
    src, fine = Zoned(x, nt, offset_one), Zoned(nf, nt, offset_one)
    t.prolongate(fine.vec, src.vec)  # overwrites: the payload starts as NaN
    e_p = rel(fine.result(), P @ x)
    acc = Zoned(y, nt, offset_one)
    t.prolongate_add(acc.vec, src.vec)
    e_a = rel(acc.result(), y + P @ x)
    src.unchanged()
    coarse, fsrc = Zoned(z, nt, offset_one), Zoned(y, nt, offset_one)
    t.restrict_and_add(coarse.vec, fsrc.vec)
    got_r = coarse.result()
    fsrc.unchanged()
    e_r = rel(got_r, z + P.T @ y)
    print(f"prolongate {e_p:.2e} prolongate_add {e_a:.2e} restrict_and_add {e_r:.2e}")
    assert e_p <= tol and e_a <= tol and e_r <= tol, (e_p, e_a, e_r)
    np.testing.assert_array_equal(got_r[con], z[con].astype(got_r.dtype))  # Dirichlet entries: not touched


# ---- from_meshes and one level pair of the hierarchy


@functools.lru_cache(maxsize=None)
def _h_matrix(dim, p, n):
    c, f = mf.Mesh.uniform(dim, p, n), mf.Mesh.uniform(dim, p, 2 * n)
    cd, fd = c.transfer_patches(f)
    con = c.arrays()["constrained_dofs"].astype(np.int64)
    return mg.transfer_matrix(dim, p, cd, fd, c.n_dofs, f.n_dofs, con), con


@ALIGN
@TYPES
@pytest.mark.parametrize("dim,p,n", [(3, 2, 2), (2, 4, 3)])
def test_h_transfer_from_meshes(dim, p, n, nt, offset_one):
    P, con = _h_matrix(dim, p, n)
    c, f = mf.Mesh.uniform(dim, p, n, number_type=nt), mf.Mesh.uniform(dim, p, 2 * n, number_type=nt)
    check_transfer(mf.Transfer.from_meshes(c, f), P, con, nt, offset_one)


@functools.lru_cache(maxsize=None)
def _hierarchy(n_ref=3):
    return mg.Hierarchy(3, 2, n_ref)


@ALIGN
@TYPES
@pytest.mark.parametrize("n_ref", [3, 4])
def test_h_transfer_of_a_hierarchy_level_pair(n_ref, nt, offset_one):
    """the finest level pair of MgHierarchy(adaptive_mg(3, 2, n_ref)).  n_ref = 3 is one cell and its eight children;
    n_ref = 4 is the smallest at which the parents are only a part of the coarser level (21 of its 392 cells)"""
    H = _hierarchy(n_ref)
    l = H.n_levels - 1
    cd, fd = H.patches[l]
    assert (len(cd), H.od[l - 1].n_cells) == {3: (1, 1), 4: (21, 392)}[n_ref]
    con = H.od[l - 1].constrained
    t = mf.Transfer.from_arrays(3, 2, cd, fd, H.od[l - 1].n_dofs, H.od[l].n_dofs, con, nt)
    check_transfer(t, H.P[l], con.astype(np.int64), nt, offset_one)


# ---- the p-transfer


@functools.lru_cache(maxsize=None)
def _p_matrix(dim, pc, pf):
    c, f = mesh_pair("cube", dim, pc, pf, F64)
    con = c.arrays()["constrained_dofs"].astype(np.int64)
    return pr.p_transfer_matrix(dim, pc, pf, c.arrays()["loc2glob"], f.arrays()["loc2glob"], c.n_dofs, f.n_dofs, con), con


@ALIGN
@TYPES
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("pc,pf", [(1, 2), (2, 4), (1, 6), (5, 6)])
def test_p_transfer_from_meshes(pc, pf, dim, nt, offset_one):
    P, con = _p_matrix(dim, pc, pf)
    c, f = mesh_pair("cube", dim, pc, pf, nt)
    check_transfer(mf.Transfer.p_from_meshes(c, f), P, con, nt, offset_one)


@functools.lru_cache(maxsize=None)
def _p_hn_matrix(pc, pf):
    c, f = mf.Mesh.adaptive(3, pc, 4), mf.Mesh.adaptive(3, pf, 4)
    assert (c.arrays()["constraint_mask"] != 0).any()
    return hnr.mesh_pair_matrix_hn(c, f), c.arrays()["constrained_dofs"].astype(np.int64)


@ALIGN
@TYPES
@pytest.mark.parametrize("pc,pf", [(1, 2), (2, 4)])
def test_p_transfer_with_hanging_nodes(pc, pf, nt, offset_one):
    P, con = _p_hn_matrix(pc, pf)
    c, f = mf.Mesh.adaptive(3, pc, 4, number_type=nt), mf.Mesh.adaptive(3, pf, 4, number_type=nt)
    check_transfer(mf.Transfer.p_hn_from_meshes(c, f), P, con, nt, offset_one)


# ---- the global-coarsening h-transfer


def _gc_pair(p, which, nt):
    seq = mf.Mesh.coarsening_sequence(mf.Mesh.adaptive(3, p, 4, number_type=nt))
    assert len(seq) >= 4
    k = len(seq) - 1 if which == "finest" else 2  # (interior: neither the coarsest nor the finest mesh)
    return seq[k - 1], seq[k], seq


@functools.lru_cache(maxsize=None)
def _gc_matrix(p, which):
    c, f, _ = _gc_pair(p, which, F64)
    assert (f.arrays()["constraint_mask"] != 0).any()
    return gr.mesh_pair_matrix_gc(c, f), c.arrays()["constrained_dofs"].astype(np.int64)


@ALIGN
@TYPES
@pytest.mark.parametrize("which", ["finest", "interior"])
@pytest.mark.parametrize("p", [1, 2, 4])
def test_h_transfer_with_hanging_nodes(p, which, nt, offset_one):
    P, con = _gc_matrix(p, which)
    c, f, keep = _gc_pair(p, which, nt)
    check_transfer(mf.Transfer.h_hn_from_meshes(c, f), P, con, nt, offset_one)


# ---- the level operator and its interface matrices


@functools.lru_cache(maxsize=None)
def _level_reference(dim, p, n, nt):
    mesh = mf.Mesh.uniform(dim, p, n, number_type=nt)
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    edge = np.nonzero(np.abs(mesh.dof_coords()[:, 0]) < 1e-12)[0].astype(np.uint32)  # the plane x = 0
    assert 0 < len(edge) < mesh.n_dofs
    odc = mg.with_constrained(od, np.union1d(od.constrained, edge))
    x = typed(np.random.default_rng(dim * 10 + p).standard_normal(mesh.n_dofs), nt)
    want = (o.vmult(odc, x), o.vmult_interface_down(od, edge, x), o.vmult_interface_up(od, edge, x),
            o.compute_inverse_diagonal(odc))
    return mesh, edge, x, want


@ALIGN
@TYPES
@pytest.mark.parametrize("dim,p,n", [(3, 2, 4), (2, 4, 5)])
def test_level_operator_and_interface_matrices(dim, p, n, nt, offset_one):
    mesh, edge, x, want = _level_reference(dim, p, n, nt)
    lev = mf.Level(mesh.desc, edge, mesh)
    N = mesh.n_dofs
    src = Zoned(x, nt, offset_one)
    for fn, ref in zip((lev.vmult, lev.vmult_interface_down, lev.vmult_interface_up), want):
        dst = Zoned(N, nt, offset_one)
        fn(dst.vec, src.vec)
        got = dst.result().astype(np.float64)
        src.unchanged()
        assert np.linalg.norm(got - ref) <= TOL[nt] * np.linalg.norm(ref), fn.__name__
    d = Zoned(N, nt, offset_one)
    lev.compute_inverse_diagonal(d.vec)
    got = d.result().astype(np.float64)
    assert np.linalg.norm(got - want[3]) <= TOL[nt] * np.linalg.norm(want[3])


# ---- index pairs


@ALIGN
@TYPES
def test_index_pairs_copy_and_convert(nt, offset_one):
    """copy_to_mg / copy_from_mg over the copy pairs of every level of adaptive_mg(3, 2, 3): IndexPairs.copy in the
    number type, copy_pairs_convert into the number type from the other one; entries outside the pairs keep their bits"""
    H = _hierarchy()
    other = F32 if nt == F64 else F64
    dt = mf.np_dtype(nt)
    N = H.mesh.n_dofs
    rng = np.random.default_rng(N)
    for l in range(H.n_levels):
        a, b = H.pairs[l]  # (active dofs, level dofs)
        nl = H.od[l].n_dofs
        act, lev0 = rng.standard_normal(N), rng.standard_normal(nl)
        for src_t in (nt, other):
            src, dst = Zoned(act, src_t, offset_one), Zoned(lev0, nt, offset_one)
            pairs = mf.IndexPairs(b, a)
            if src_t == nt:
                pairs.copy(dst.vec, src.vec, nt)
            else:
                mf.copy_pairs_convert(pairs, dst.vec, nt, src.vec, src_t)
            want = lev0.astype(dt)
            want[b] = act.astype(mf.np_dtype(src_t))[a].astype(dt)
            np.testing.assert_array_equal(dst.result(), want)
            src.unchanged()
