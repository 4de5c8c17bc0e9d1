"""CPU: the host side of adaptive refinement: one refinement step of a leaf set
(mfgpu_mesh_refine_leaves) against the pure-Python rule of tests/amr_reference.py, its properties and error cases,
mark_fixed_number, and the numpy indicator of amr_reference.py by what it must do (vanish on polynomials, localise a
kink, drive the CPU loop to a smaller error) -- the facts the GPU tests of tests/test_gpu_amr.py rely on."""
import numpy as np
import pytest

import amr_reference as ar
import gc_reference as gr
import poisson_reference as pr
import pymfgpu as mf
from test_hanging_host import CASES, leaves_refine


def as_set(leaves):
    return sorted(tuple(int(v) for v in l) for l in leaves)


def as_list(leaves):
    return [tuple(int(v) for v in l) for l in leaves]


def flag_sets(n, seed):
    """none, all, each third of the leaves, and two random selections"""
    rng = np.random.default_rng(seed)
    out = [np.zeros(n, dtype=np.uint8), np.ones(n, dtype=np.uint8)]
    for k in range(3):
        f = np.zeros(n, dtype=np.uint8)
        f[k::3] = 1
        out.append(f)
    out += [(rng.uniform(size=n) < q).astype(np.uint8) for q in (0.15, 0.5)]
    return out


def check_step(dim, leaves, flags, balance_vertices=False):
    leaves = np.asarray(leaves, dtype=np.uint32).reshape(-1, 4)
    new = mf.Mesh.refine_leaves(dim, leaves, flags, balance_vertices)
    assert as_list(new) == ar.refine_rule(dim, leaves, flags, balance_vertices)  # the same leaves in the same order
    # a partition that from_leaves accepts (it refuses what is not one-irregular), one-irregular by the Python check
    assert sum(2.0 ** (-dim * int(l[0])) for l in new) == 1.0 and len(set(as_list(new))) == len(new)
    assert gr.one_irregular(dim, new)
    fine = mf.Mesh.from_leaves(dim, 1, new)
    assert fine.n_cells == len(new)
    # every output leaf is an input leaf or a child of one: the map exists, and flagged leaves are split
    parent, child = mf.coarsening_map(mf.Mesh.from_leaves(dim, 1, leaves), fine)
    old_order = {l: i for i, l in enumerate(as_list(mf.Mesh.from_leaves(dim, 1, leaves).cell_levels()))}
    split = set(parent[child != 0].tolist())
    assert all(old_order[l] in split for l, f in zip(as_list(leaves), flags) if f)
    # the same set for permuted input
    perm = np.random.default_rng(len(new)).permutation(len(leaves))
    assert as_set(mf.Mesh.refine_leaves(dim, leaves[perm], np.asarray(flags)[perm], balance_vertices)) == as_set(new)
    return new


@pytest.mark.parametrize("name", sorted(CASES))
def test_refinement_equals_the_python_rule_on_the_small_cases(name):
    dim, leaves = CASES[name]
    for k, flags in enumerate(flag_sets(len(leaves), len(leaves))):
        for bv in (False, True):
            new = check_step(dim, leaves, flags, bv)
            if k == 0:
                assert as_list(new) == as_list(leaves)  # nothing flagged: unchanged, in order
    # all flagged, then one coarsening step: back to the input
    every = mf.Mesh.refine_leaves(dim, leaves, np.ones(len(leaves)))
    assert len(every) == len(leaves) * 2 ** dim
    assert as_set(mf.Mesh.coarsen_leaves(dim, every)) == as_set(leaves)


def test_2d_one_fine_cell_forces_a_coarse_neighbour():
    leaves = leaves_refine(2, 1, [(0, 0)])  # level-2 cells in the lower left quarter, three level-1 cells
    flags = [l == [2, 1, 0, 0] for l in leaves]  # the fine cell next to the level-1 cell (1, 0) over a face
    new = as_set(check_step(2, leaves, flags))
    assert (1, 1, 0, 0) not in new and (2, 2, 0, 0) in new and (3, 2, 0, 0) in new
    assert (1, 0, 1, 0) in new and (1, 1, 1, 0) in new and len(new) == 7 + 3 + 3
    # the fine cell at the centre touches (1, 1, 1) over a vertex only: it forces it with balance_vertices alone
    flags = [l == [2, 1, 1, 0] for l in leaves]
    plain, balanced = as_set(check_step(2, leaves, flags)), as_set(check_step(2, leaves, flags, True))
    assert (1, 1, 1, 0) in plain and (1, 1, 1, 0) not in balanced
    assert len(plain) == 7 + 3 + 6 and len(balanced) == len(plain) + 3


def test_3d_an_edge_neighbour_alone_forces_the_split():
    dim, leaves = CASES["3d_edge"]
    # (tests/test_gc_host.py) the level-2 cell (1, 2, 0) has level-2 face neighbours and the level-1 cell (1, 0, 0) across
    # a z-edge
    flags = [l == [2, 1, 2, 0] for l in leaves]
    new = as_set(check_step(dim, leaves, flags))
    assert (1, 1, 0, 0) not in new and (2, 2, 0, 0) in new
    for d, nb in enumerate(([2, 0, 2, 0], [2, 1, 3, 0], [2, 1, 2, 1])):  # its face neighbours stay
        assert tuple(nb) in new
    assert len(new) == len(leaves) + 7 + 7


def test_3d_balance_vertices_changes_the_result():
    leaves = leaves_refine(3, 1, [(0, 0, 0)])
    flags = [l == [2, 1, 1, 1] for l in leaves]  # touches the level-1 cell (1, 1, 1) at the centre vertex only
    plain, balanced = as_set(check_step(3, leaves, flags)), as_set(check_step(3, leaves, flags, True))
    assert (1, 1, 1, 1) in plain and (1, 1, 1, 1) not in balanced
    assert len(balanced) == len(plain) + 7


@pytest.mark.parametrize("balance_vertices", [False, True], ids=["faces_edges", "vertices"])
@pytest.mark.parametrize("dim,n_ref", [(2, 4), (3, 4)])
def test_refinement_of_the_adaptive_recipe(dim, n_ref, balance_vertices):
    """Mesh.adaptive is balanced over faces and edges, Mesh.adaptive_mg over vertices too; two steps, so that the second
    starts from a result of the call"""
    leaves = (mf.Mesh.adaptive_mg if balance_vertices else mf.Mesh.adaptive)(dim, 1, n_ref).cell_levels()
    assert ar.one_irregular(dim, leaves, balance_vertices)
    rng = np.random.default_rng(n_ref)
    for q in (0.05, 0.3):
        flags = (rng.uniform(size=len(leaves)) < q).astype(np.uint8)
        new = check_step(dim, leaves, flags, balance_vertices)
        assert ar.one_irregular(dim, new, balance_vertices)
        print(f"adaptive {dim}D n_ref {n_ref}: {len(leaves)} leaves, {int(flags.sum())} flagged -> {len(new)}")
        if len(new) < 4000:
            leaves = new


def test_balance_vertices_refuses_an_input_that_is_not_balanced_over_vertices():
    """one-irregular over faces, but the level-1 leaf (1, 1, 1) meets the level-3 leaf (3, 3, 3) at the centre vertex.
    The closure starts at split leaves only, so with balance_vertices such an input would come back unbalanced (nothing
    flagged) or force a child to split ((3, 3, 3) flagged): it is refused, by the library and by the Python rule."""
    leaves = [[1, 1, 1, 0]] + [[2, 2 + i, j, 0] for j in (0, 1) for i in (0, 1)] + [[2, i, 2 + j, 0] for j in (0, 1) for i in (0, 1)]
    leaves += [[2, 0, 0, 0], [2, 1, 0, 0], [2, 0, 1, 0]] + [[3, 2 + i, 2 + j, 0] for j in (0, 1) for i in (0, 1)]
    assert len(leaves) == 16 and gr.one_irregular(2, leaves) and not ar.one_irregular(2, leaves, True)
    for flags in (np.zeros(16), [l == [3, 3, 3, 0] for l in leaves]):
        with pytest.raises(mf.MfgpuError, match="one-irregular over vertices") as e:
            mf.Mesh.refine_leaves(2, leaves, flags, True)
        assert e.value.code == mf.EINVAL
        with pytest.raises(ValueError):
            ar.refine_rule(2, leaves, flags, True)
        check_step(2, leaves, flags)  # without balance_vertices the input is fine, and the result follows the rule
    # balanced first (split (1, 1, 1) by hand), the same flags go through and the result is balanced over vertices
    balanced = mf.Mesh.refine_leaves(2, leaves, [l == [1, 1, 1, 0] for l in leaves]).tolist()
    assert ar.one_irregular(2, balanced, True)
    new = check_step(2, balanced, [l == [3, 3, 3, 0] for l in balanced], True)
    # (3, 3, 3) splits, and with it its face neighbours (2, 2, 1), (2, 1, 2) and its vertex neighbour (2, 2, 2)
    assert ar.one_irregular(2, new, True) and (2, 2, 2, 0) not in as_set(new) and len(new) == len(balanced) + 3 + 9
    # 3D: the same at the centre of the cube
    leaves3 = leaves_refine(3, 1, [(0, 0, 0)])
    fine3 = mf.Mesh.refine_leaves(3, leaves3, [l == [2, 1, 1, 1] for l in leaves3]).tolist()  # (1, 1, 1, 1) stays: vertex only
    assert [1, 1, 1, 1] in fine3 and gr.one_irregular(3, fine3) and not ar.one_irregular(3, fine3, True)
    with pytest.raises(mf.MfgpuError, match="one-irregular over vertices"):
        mf.Mesh.refine_leaves(3, fine3, np.zeros(len(fine3)), True)
    check_step(3, fine3, np.zeros(len(fine3)))


def test_mesh_refined():
    mesh = mf.Mesh.adaptive(2, 2, 3, number_type=mf.F32)
    flags = np.zeros(mesh.n_cells, dtype=np.uint8)
    flags[::5] = 1
    fine = mesh.refined(flags)
    assert int(fine.desc.degree) == 2 and int(fine.desc.number_type) == mf.F32
    assert as_list(fine.cell_levels()) != [] and fine.n_cells > mesh.n_cells
    assert as_set(fine.cell_levels()) == as_set(ar.refine_rule(2, mesh.cell_levels(), flags))
    assert int(mesh.refined(flags, degree=3, number_type=mf.F64).desc.degree) == 3
    with pytest.raises(mf.MfgpuError):
        mf.Mesh.uniform(2, 1, 4).refined(np.zeros(16))


def test_errors():
    def raises(fn, *args):
        with pytest.raises(mf.MfgpuError) as e:
            fn(*args)
        assert e.value.code == mf.EINVAL, str(e.value)
        return str(e.value)

    ok = leaves_refine(2, 1, [(0, 0)])
    one = np.ones(len(ok))
    raises(mf.Mesh.refine_leaves, 4, ok, one)                                   # dim
    raises(mf.Mesh.refine_leaves, 2, np.zeros((0, 4)), np.zeros(0))
    raises(mf.Mesh.refine_leaves, 2, ok[:-1], one[:-1])                         # a hole
    raises(mf.Mesh.refine_leaves, 2, ok + [ok[0]], np.ones(len(ok) + 1))        # a leaf twice
    raises(mf.Mesh.refine_leaves, 2, ok + [[1, 0, 0, 0]], np.ones(len(ok) + 1))  # a leaf inside another
    raises(mf.Mesh.refine_leaves, 2, ok[:-1] + [[1, 2, 1, 0]], one)             # outside the root cell
    bad = [l for l in ok if l != [2, 1, 1, 0]] + [[3, 2 + i, 2 + j, 0] for i in (0, 1) for j in (0, 1)]
    assert not gr.one_irregular(2, bad)
    raises(mf.Mesh.refine_leaves, 2, bad, np.zeros(len(bad)))                   # not one-irregular
    # the capacity: the message names the needed count
    L = mf.lib()
    lv = np.ascontiguousarray(ok, dtype=np.uint32)
    fl = np.zeros(len(ok), dtype=np.uint8)
    fl[0] = 1
    out = np.zeros((len(ok) + 3, 4), dtype=np.uint32)
    assert L.mfgpu_mesh_refine_leaves(2, lv.ctypes.data, len(lv), fl.ctypes.data, 0, out.ctypes.data, len(ok) + 2) == mf.EINVAL
    assert f"{len(ok) + 3} leaves" in L.mfgpu_last_error().decode()
    assert L.mfgpu_mesh_refine_leaves(2, lv.ctypes.data, len(lv), fl.ctypes.data, 0, out.ctypes.data, len(ok) + 3) == len(ok) + 3
    assert L.mfgpu_mesh_refine_leaves(2, lv.ctypes.data, len(lv), None, 0, out.ctypes.data, len(ok) + 3) == mf.EINVAL
    # a child deeper than level 18: a chain of corner refinements down to level 18, then its finest cell flagged
    deep = [[0, 0, 0, 0]]
    for _ in range(18):
        f = np.zeros(len(deep), dtype=np.uint8)
        f[[i for i, l in enumerate(deep) if list(l[1:]) == [0, 0, 0] and l[0] == max(x[0] for x in deep)][0]] = 1
        deep = mf.Mesh.refine_leaves(2, deep, f).tolist()
    assert max(l[0] for l in deep) == 18
    f = np.zeros(len(deep), dtype=np.uint8)
    f[[i for i, l in enumerate(deep) if l[0] == 18][0]] = 1
    assert "level 18" in raises(mf.Mesh.refine_leaves, 2, deep, f)
    assert len(mf.Mesh.refine_leaves(2, deep, np.zeros(len(deep)))) == len(deep)


def test_mark_fixed_number():
    eta = np.array([3.0, 1.0, 3.0, 0.5, 3.0, 2.0])
    assert not mf.mark_fixed_number(eta, 0.0).any()
    assert mf.mark_fixed_number(eta, 1.0).all()
    np.testing.assert_array_equal(mf.mark_fixed_number(eta, 1 / 3), [1, 0, 1, 0, 0, 0])   # ties: the lower index
    np.testing.assert_array_equal(mf.mark_fixed_number(eta, 0.34), [1, 0, 1, 0, 1, 0])    # ceil(2.04) = 3
    np.testing.assert_array_equal(mf.mark_fixed_number(eta, 0.5), [1, 0, 1, 0, 1, 0])
    np.testing.assert_array_equal(mf.mark_fixed_number(eta, 4 / 6), [1, 0, 1, 0, 1, 1])
    np.testing.assert_array_equal(mf.mark_fixed_number(np.zeros(5), 0.4), [1, 1, 0, 0, 0])
    assert mf.mark_fixed_number(eta, 1e-9).sum() == 1 and mf.mark_fixed_number(np.zeros(0), 0.5).size == 0
    rng = np.random.default_rng(0)
    for n in (1, 7, 64):
        e = rng.integers(0, 4, n).astype(np.float64)
        for fr in (0.0, 0.1, 0.3, 0.99, 1.0):
            np.testing.assert_array_equal(mf.mark_fixed_number(e, fr), ar.mark_fixed_number(e, fr))
    with pytest.raises(mf.MfgpuError):
        mf.mark_fixed_number(eta, 1.5)


# ---- the numpy indicator by what it must do (the GPU tests compare with it)

KNOWN_ANSWER_FACTOR = 1e4  # tests/test_gpu_amr.py: sum eta_K^2 <= (FACTOR * 2.2e-16)^2 * sum int |grad u_h|^2


def polynomial(dim, p, seed):
    coef = np.random.default_rng(seed).uniform(0.5, 1.5, (dim, p + 1))
    return lambda X: np.prod([np.polyval(coef[d], X[:, d]) for d in range(dim)], axis=0)


def known_answer_ratio(cells, eta, grads):
    jxw = cells.od.JxW.astype(np.float64).reshape(cells.od.n_cells, -1)
    return np.sqrt(eta.sum() / np.sum(np.sum(grads ** 2, axis=-1) * jxw))


@pytest.mark.parametrize("kind,dim,p", [("uniform", 2, 6), ("leaves", 2, 6), ("uniform", 3, 6), ("leaves", 3, 6),
                                        ("leaves", 2, 1), ("leaves", 3, 2), ("leaves", 2, 4)])
def test_the_reference_vanishes_on_polynomials_100x_inside_the_gpu_bound(kind, dim, p):
    mesh = small_mesh(kind, dim, p)
    cells = pr.Cells(mesh)
    u = polynomial(dim, p, 7 * p + dim)(mesh.dof_coords())
    eta, grads, G = ar.recovery_indicator(cells, u, parts=True)
    r = known_answer_ratio(cells, eta, grads)
    print(f"{kind} {dim}D p = {p}: sqrt(sum eta^2 / sum int |grad u_h|^2) = {r:.2e}, bound {KNOWN_ANSWER_FACTOR * 2.2e-16:.1e}")
    assert r <= KNOWN_ANSWER_FACTOR * 2.2e-16 / 100


def small_mesh(kind, dim, p):
    if kind == "uniform":
        return mf.Mesh.uniform(dim, p, [3, 2] if dim == 2 else [2, 2, 2])
    if kind == "leaves":  # the root split, one child split again: 7 / 15 leaves
        return mf.Mesh.from_leaves(dim, p, leaves_refine(dim, 1, [(0,) * dim]))
    return mf.Mesh.ball(dim, p, int(kind[-1]))


def test_the_reference_localises_a_kink():
    mesh = mf.Mesh.uniform(2, 2, 8)
    cells = pr.Cells(mesh)
    eta = ar.recovery_indicator(cells, np.abs(mesh.dof_coords()[:, 0] - 0.3))
    col = np.floor((cells.qpts[:, :, 0].mean(axis=1) + 1.0) / 0.25).astype(int)
    kink = int(np.floor(1.3 / 0.25))
    big = eta > 1e-3 * eta.max()
    print("columns of the cells above 1e-3 max:", sorted(set(col[big].tolist())), "kink column", kink,
          "largest outside the three columns / max", eta[np.abs(col - kink) > 1].max() / eta.max())
    assert big[col == kink].all() and (np.abs(col[big] - kink) <= 1).all()


def test_the_cpu_loop_reduces_the_error():
    out = ar.amr_loop(2, 2, 2, 3, 0.3)
    for leaves, l2, eta in out:
        print(f"{len(leaves)} cells: l2 {l2:.3e} eta {eta:.3e}")
    assert [len(l) for l, _, _ in out] == sorted(len(l) for l, _, _ in out) and len(out[0][0]) == 16
    assert out[-1][1] < out[0][1]
