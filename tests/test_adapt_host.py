"""CPU: the host side of adaptation in both directions: one step of refinement and coarsening of a
leaf set (mfgpu_mesh_adapt_leaves) against the pure-Python rule of tests/adapt_reference.py -- both sets and their order
-- the properties include/mfgpu.h states, the error cases, and mark_refine_coarsen."""
import numpy as np
import pytest

import adapt_reference as ad
import amr_reference as ar
import gc_reference as gr
import pymfgpu as mf
from test_amr_host import as_list, as_set
from test_hanging_host import CASES, leaves_refine


def flag_pairs(n, seed):
    """(refine, coarsen): none, coarsen all, refine thirds with everything else willing to coarsen, and random pairs that
    overlap (refinement wins)"""
    rng = np.random.default_rng(seed)
    zero, one = np.zeros(n, dtype=np.uint8), np.ones(n, dtype=np.uint8)
    out = [(zero, zero), (zero, one), (one, one)]
    for k in range(3):
        f = np.zeros(n, dtype=np.uint8)
        f[k::3] = 1
        out += [(f, one), (f, 1 - f), (f, zero)]
    for q, r in ((0.1, 0.9), (0.3, 0.6), (0.05, 1.0), (0.5, 0.5)):
        out.append(((rng.uniform(size=n) < q).astype(np.uint8), (rng.uniform(size=n) < r).astype(np.uint8)))
    return out


def check_step(dim, leaves, refine, coarsen, balance_vertices=False):
    """the library against the rule, and every property of the header; returns (new, mid)"""
    leaves = np.asarray(leaves, dtype=np.uint32).reshape(-1, 4)
    new, mid = mf.Mesh.adapt_leaves(dim, leaves, refine, coarsen, balance_vertices)
    want_new, want_mid = ad.adapt_rule(dim, leaves, refine, coarsen, balance_vertices)
    assert as_list(new) == want_new and as_list(mid) == want_mid  # the same leaves in the same order
    for s in (new, mid):  # partitions, one-irregular in the relation of the call
        assert sum(2.0 ** (-dim * int(l[0])) for l in s) == 1.0 and len(set(as_list(s))) == len(s)
        assert gr.one_irregular(dim, s) and ar.one_irregular(dim, s, balance_vertices)
    # refinement wins: a leaf with a refine flag is split
    new_set = set(as_list(new))
    assert all(l not in new_set for l, f in zip(as_list(leaves), refine) if f)
    # both coarsening maps exist: every old and every new leaf is a leaf of mid or the child of one
    m_mid, m_old, m_new = (mf.Mesh.from_leaves(dim, 1, s) for s in (mid, leaves, new))
    for fine in (m_old, m_new):
        parent, child = mf.coarsening_map(m_mid, fine)
        gp, gc = gr.coarsening_map(m_mid, fine)
        assert (parent == gp).all() and (child == gc).all()
    # the same sets for permuted input
    perm = np.random.default_rng(len(new)).permutation(len(leaves))
    pn, pm = mf.Mesh.adapt_leaves(dim, leaves[perm], np.asarray(refine)[perm], np.asarray(coarsen)[perm], balance_vertices)
    assert as_set(pn) == as_set(new) and as_set(pm) == as_set(mid)
    return new, mid


@pytest.mark.parametrize("name", sorted(CASES))
def test_adaptation_equals_the_python_rule_on_the_small_cases(name):
    dim, leaves = CASES[name]
    n = len(leaves)
    for k, (rf, cf) in enumerate(flag_pairs(n, n)):
        for bv in (False, True):
            new, mid = check_step(dim, leaves, rf, cf, bv)
            if k == 0:  # no flags
                assert as_list(new) == as_list(leaves) and as_list(mid) == as_list(leaves)
            if not cf.any():  # refine flags only
                assert as_list(new) == as_list(mf.Mesh.refine_leaves(dim, leaves, rf, bv)) and as_list(mid) == as_list(leaves)
            if k == 1 and not bv:  # all coarsen flags, no refine flags
                coarse = as_set(mf.Mesh.coarsen_leaves(dim, leaves))
                assert as_set(new) == coarse and as_set(mid) == coarse and len(coarse) < n


@pytest.mark.parametrize("balance_vertices", [False, True], ids=["faces_edges", "vertices"])
@pytest.mark.parametrize("dim,n_ref", [(2, 4), (3, 4)])
def test_seeded_random_flags_on_the_adaptive_recipe(dim, n_ref, balance_vertices):
    """several steps, each from the result of the last, so that families made by one step are coarsened by a later one"""
    leaves = (mf.Mesh.adaptive_mg if balance_vertices else mf.Mesh.adaptive)(dim, 1, n_ref).cell_levels()
    rng = np.random.default_rng(10 * dim + n_ref + balance_vertices)
    coarsened = refined = 0
    for q, r in ((0.05, 0.8), (0.2, 0.5), (0.02, 1.0)):
        rf = (rng.uniform(size=len(leaves)) < q).astype(np.uint8)
        cf = (rng.uniform(size=len(leaves)) < r).astype(np.uint8)
        new, mid = check_step(dim, leaves, rf, cf, balance_vertices)
        families = (len(leaves) - len(mid)) // (2 ** dim - 1)
        split = (len(new) - len(mid)) // (2 ** dim - 1)
        print(f"{dim}D n_ref {n_ref}: {len(leaves)} leaves, {int(rf.sum())} refine and {int(cf.sum())} coarsen flags -> "
              f"{len(new)} leaves, {families} families coarsened, {split} leaves split")
        coarsened, refined = coarsened + families, refined + split
        if len(new) < 1500:
            leaves = new
    assert coarsened and refined


def test_2d_a_family_is_rolled_back_next_to_a_refined_leaf():
    """leaves_refine(2, 2, [(1, 1)]): a 4 x 4 grid of level-2 cells with the cell (1, 1) split into four level-3 cells.
    The family of the level-1 cell (1, 0) is complete; as a parent it shares the face x = 2 with the level-3 cells
    (3, 3, 2) and (3, 3, 3), two levels finer, so it is rolled back.  The family of (1, 1) meets them at a vertex only."""
    leaves = leaves_refine(2, 2, [(1, 1)])
    none = np.zeros(len(leaves), dtype=np.uint8)
    willing = np.array([l[0] == 2 and (l[1] >> 1, l[2] >> 1) == (1, 0) for l in leaves], dtype=np.uint8)
    assert willing.sum() == 4
    new, mid = check_step(2, leaves, none, willing)
    assert as_list(new) == as_list(leaves) and as_list(mid) == as_list(leaves)
    # the far corner's family does not touch them: it survives, and stands where its child 0 stood
    far = np.array([l[0] == 2 and (l[1] >> 1, l[2] >> 1) == (1, 1) for l in leaves], dtype=np.uint8)
    new, mid = check_step(2, leaves, none, far)
    at = as_list(leaves).index((2, 2, 2, 0))
    assert as_list(new)[at] == (1, 1, 1, 0) and len(new) == len(leaves) - 3 and as_list(mid) == as_list(new)
    # a refine flag on one of its children: refinement wins, the family stays and the child splits
    rf = np.array([l == [2, 3, 3, 0] for l in leaves], dtype=np.uint8)
    new, mid = check_step(2, leaves, rf, far)
    assert (1, 1, 1, 0) not in as_set(new) and (3, 6, 6, 0) in as_set(new) and as_list(mid) == as_list(leaves)
    # a family whose child the closure splits is no candidate either: refine the level-3 cell (3, 3, 3); it forces
    # (2, 2, 1), a child of (1, 1, 0), over the face x = 2
    rf = np.array([l == [3, 3, 3, 0] for l in leaves], dtype=np.uint8)
    new, mid = check_step(2, leaves, rf, willing)
    assert (2, 2, 1, 0) not in as_set(new) and (1, 1, 0, 0) not in as_set(new) and as_list(mid) == as_list(leaves)


def test_mesh_adapted():
    mesh = mf.Mesh.adaptive(2, 2, 3, number_type=mf.F32)
    rf, cf = np.zeros(mesh.n_cells, dtype=np.uint8), np.ones(mesh.n_cells, dtype=np.uint8)
    rf[::7] = 1
    new, mid = mesh.adapted(rf, cf)
    want_new, want_mid = ad.adapt_rule(2, mesh.cell_levels(), rf, cf)
    assert as_set(new.cell_levels()) == sorted(want_new) and as_set(mid.cell_levels()) == sorted(want_mid)
    assert mid.n_cells < mesh.n_cells and mid.n_cells < new.n_cells
    for m in (new, mid):
        assert int(m.desc.degree) == 2 and int(m.desc.number_type) == mf.F32
    assert int(mesh.adapted(rf, cf, degree=3, number_type=mf.F64)[1].desc.degree) == 3
    with pytest.raises(mf.MfgpuError):
        mf.Mesh.uniform(2, 1, 4).adapted(np.zeros(16), np.zeros(16))


def test_errors_create_nothing():
    def raises(*args):
        with pytest.raises(mf.MfgpuError) as e:
            mf.Mesh.adapt_leaves(*args)
        assert e.value.code == mf.EINVAL, str(e.value)
        return str(e.value)

    ok = leaves_refine(2, 1, [(0, 0)])
    one, zero = np.ones(len(ok)), np.zeros(len(ok))
    raises(4, ok, one, zero)                                                   # dim
    raises(2, np.zeros((0, 4)), np.zeros(0), np.zeros(0))
    raises(2, ok[:-1], one[:-1], zero[:-1])                                    # a hole
    raises(2, ok + [ok[0]], np.ones(len(ok) + 1), np.zeros(len(ok) + 1))       # a leaf twice
    raises(2, ok + [[1, 0, 0, 0]], np.ones(len(ok) + 1), np.zeros(len(ok) + 1))  # a leaf inside another
    raises(2, ok[:-1] + [[1, 2, 1, 0]], one, zero)                             # outside the root cell
    bad = [l for l in ok if l != [2, 1, 1, 0]] + [[3, 2 + i, 2 + j, 0] for i in (0, 1) for j in (0, 1)]
    assert not gr.one_irregular(2, bad)
    raises(2, bad, np.zeros(len(bad)), np.ones(len(bad)))                      # not one-irregular
    # balance_vertices on an input that is not balanced over vertices (tests/test_amr_host.py)
    leaves3 = leaves_refine(3, 1, [(0, 0, 0)])
    fine3 = mf.Mesh.refine_leaves(3, leaves3, [l == [2, 1, 1, 1] for l in leaves3]).tolist()
    assert "one-irregular over vertices" in raises(3, fine3, np.zeros(len(fine3)), np.ones(len(fine3)), True)
    with pytest.raises(ValueError):
        ad.adapt_rule(3, fine3, np.zeros(len(fine3)), np.ones(len(fine3)), True)
    # the capacity: the message names the needed count, and nothing is written
    L = mf.lib()
    lv = np.ascontiguousarray(ok, dtype=np.uint32)
    rf, cf = np.zeros(len(ok), dtype=np.uint8), np.zeros(len(ok), dtype=np.uint8)
    rf[0] = 1
    new, mid = np.full((len(ok) + 3, 4), 77, dtype=np.uint32), np.full((len(ok), 4), 77, dtype=np.uint32)
    n_mid = mf.C.c_uint32(77)

    def call(rfp, cfp, cap):
        return L.mfgpu_mesh_adapt_leaves(2, lv.ctypes.data, len(lv), rfp, cfp, 0, new.ctypes.data, cap, mid.ctypes.data,
                                         mf.C.byref(n_mid))

    assert call(rf.ctypes.data, cf.ctypes.data, len(ok) + 2) == mf.EINVAL
    assert f"{len(ok) + 3} leaves" in L.mfgpu_last_error().decode()
    assert call(None, cf.ctypes.data, len(ok) + 3) == mf.EINVAL and call(rf.ctypes.data, None, len(ok) + 3) == mf.EINVAL
    assert (new == 77).all() and (mid == 77).all() and n_mid.value == 77
    assert call(rf.ctypes.data, cf.ctypes.data, len(ok) + 3) == len(ok) + 3 and n_mid.value == len(ok)


def test_mark_refine_coarsen():
    eta = np.array([3.0, 1.0, 3.0, 0.5, 1.0, 1.0, 2.0, 0.5])
    for fr, fc in ((0.25, 0.25), (0.3, 0.4), (0.5, 0.5), (0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (0.6, 0.6)):
        r, c = mf.mark_refine_coarsen(eta, fr, fc)
        wr, wc = ad.mark_refine_coarsen(eta, fr, fc)
        assert r.dtype == np.uint8 and c.dtype == np.uint8
        assert (r == wr).all() and (c == wc).all() and not (r & c).any()
        assert r.sum() == int(np.ceil(fr * 8)) and c.sum() == min(int(np.floor(fc * 8)), 8 - r.sum())
    # ties go to the lower index: two of the three 1.0 (cells 1, 4) after both 0.5, one of the two 3.0 (cell 0)
    r, c = mf.mark_refine_coarsen(eta, 0.125, 0.5)
    assert r.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and c.tolist() == [0, 1, 0, 1, 1, 0, 0, 1]
    # fractions 0 and 1
    r, c = mf.mark_refine_coarsen(eta, 0.0, 1.0)
    assert not r.any() and c.all()
    r, c = mf.mark_refine_coarsen(eta, 1.0, 1.0)
    assert r.all() and not c.any()
    assert all(not v.any() for v in mf.mark_refine_coarsen(eta, 0.0, 0.0))
    assert all(len(v) == 0 for v in mf.mark_refine_coarsen([], 0.5, 0.5))
    for bad in ((-0.1, 0.5), (0.5, 1.1)):
        with pytest.raises(mf.MfgpuError):
            mf.mark_refine_coarsen(eta, *bad)
