"""Host-side tests of the planner on descriptions no mesh stand-in produces (tests/topology.py): periodic rings and
tori, a cell that lists a dof twice, holes in the numbering, random numberings and cell orders, a pinched vertex of
valence 27 and more.  mfgpu_desc.loc2glob may be any cell-to-dof map, and the oracle defines the operator for all of
them, so every plan is checked for its invariants and, through the numpy emulations of the kernels' data flow, against
o.vmult / o.vmult_add.  No GPU calls.  CASES is also the case table of tests/test_gpu_topology.py."""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import pytest

import pymfgpu as mf
import topology as tp
from oracle import mf_oracle as o
from util import deform, desc_from_oracle, emulate_plan_vmult, emulate_plane_records_vmult, oracle_desc_from_mesh

Case = namedtuple("Case", "name make kw tags")
_keep_alive = []


def _box(dim, p, n):
    return o.uniform_mesh_desc(dim, p, n)


def _ring(dim, p, n, axes, compact=True):
    return tp.periodic(_box(dim, p, n), axes, compact).desc


def _pinched(dim, p, n):
    od = _box(dim, p, n)
    return tp.pinch(od, tp.interior_vertices(od)).desc


def _shuffled(od, dofs, cells, seed):
    if dofs:
        od = tp.permute_dofs(od, seed).desc
    if cells:
        od = tp.permute_cells(od, seed + 1).desc
    return od


def _adaptive():
    mesh = mf.Mesh.adaptive(3, 2, 4)
    _keep_alive.append(mesh)
    return oracle_desc_from_mesh(mesh)


def _cases():
    c = []

    def add(name, make, tags="", **kw):
        c.append(Case(name, functools.lru_cache(maxsize=None)(make), kw, frozenset(tags.split())))

    for p in (3, 4, 5, 6):
        add(f"ring2-p{p}", lambda p=p: _ring(3, p, (2, 2, 2), [0]), "ring wraps")
    add("ring4-p4", lambda: _ring(3, 4, (4, 2, 2), [0]), "ring wraps")  # (the 6x2x1 and 4x3x1 shapes wrap)
    for p in (2, 4):
        add(f"ring1-p{p}", lambda p=p: _ring(3, p, (1, 3, 3), [0]), "ring repeated" + (" wraps" if p >= 3 else ""))
    add("torus-p4", lambda: _ring(3, 4, (3, 3, 3), [0, 1, 2]), "torus wraps")
    for p in (1, 2):
        # (two cells share BOTH faces of an axis; p = 1: 8 dofs, every cell lists them all, k = 8 everywhere)
        add(f"torus2-p{p}", lambda p=p: _ring(3, p, (2, 2, 2), [0, 1, 2]), "torus" + (" all8" if p == 1 else ""))
    for p in (3, 4, 5, 6):
        add(f"ring2holes-p{p}", lambda p=p: _ring(3, p, (2, 2, 2), [0], compact=False), "ring wraps holes")
    for p, n in ((4, (3, 4, 4)), (2, (5, 5, 5))):
        for dofs, cells in ((1, 0), (0, 1), (1, 1)):
            add(f"shuffled-p{p}-{'dofs' * dofs}{'cells' * cells}",
                lambda p=p, n=n, dofs=dofs, cells=cells: _shuffled(_box(3, p, n), dofs, cells, 10 * p), "shuffled")
    add("shuffled-adaptive-p2", lambda: _shuffled(_adaptive(), 1, 1, 3), "shuffled")
    for p in (2, 4):
        add(f"pinch27-p{p}-onecell", lambda p=p: _pinched(3, p, (3, 3, 3)), "pinch repeated k27", max_cells_per_batch=1)
        add(f"pinch27-p{p}", lambda p=p: _pinched(3, p, (3, 3, 3)), "pinch repeated")
    add("2d-ring2-p2", lambda: _ring(2, 2, (2, 5), [0]), "ring")
    add("2d-torus-p4", lambda: _ring(2, 4, (3, 3), [0, 1]), "torus")
    add("2d-ring1-p3", lambda: _ring(2, 3, (1, 4), [0]), "ring repeated")
    add("2d-pinch-p3", lambda: _pinched(2, 3, (6, 6)), "pinch")
    for p in (2, 4):
        add(f"general-ring2-p{p}", lambda p=p: deform(_ring(3, p, (2, 2, 2), [0]), seed=p), "ring general")
    add("general-2d-torus-p4", lambda: deform(_ring(2, 4, (3, 3), [0, 1]), seed=7), "torus general")
    return c


CASES = _cases()
CASE = {c.name: c for c in CASES}
KERNELS = [mf.KERNEL_AUTO, mf.KERNEL_PENCILS_X, mf.KERNEL_PLANES, mf.KERNEL_PLANES_2W]
REFUSED_FAMILY = "this kernel family does not cover the description"
REFUSED_MASS = "no mass-term instantiation"


def _plane_kernel_exists(planes4, n, nt, hn, mass):
    """kernel_exists of mfgpu_internal.h for the plane families, without the shared form"""
    if not planes4:
        return 3 <= n <= 5
    return (n <= 7 and not hn and not mass) if n >= 6 else (n >= 3 and not (mass and n == 5 and nt == mf.F64))


def expected_kernel(od, kernel, colored, nt=mf.F64, mass=False):
    """What include/mfgpu.h documents for mfgpu_desc.kernel: ("ran", kernel_name) or ("refused", part of the message).
    A forced family is refused where it does not cover the description (the plane kernels and apply_batches_x: 3D,
    uniform Jacobian, two-pass; the plane kernels p >= 2) or lacks the instantiation; AUTO never refuses."""
    p, dim, general, hn = od.degree, od.dim, not od.uniform_j0, od.constraint_mask is not None
    pk_ok = dim == 3 and not general and not colored and p >= 2
    xk_ok = dim == 3 and not general and not colored
    want_planes = kernel in (mf.KERNEL_PLANES, mf.KERNEL_PLANES_2W)
    if (want_planes and not pk_ok) or (kernel == mf.KERNEL_PENCILS_X and not xk_ok):
        return "refused", REFUSED_FAMILY
    planes4 = kernel == mf.KERNEL_PLANES_2W or p >= 5 or (kernel == mf.KERNEL_AUTO and p == 3 and nt == mf.F64)
    no_mass_planes = mass and pk_ok and not _plane_kernel_exists(planes4, p + 1, nt, False, True)
    if no_mass_planes and want_planes:
        return "refused", REFUSED_MASS
    if pk_ok and not no_mass_planes and (want_planes or (kernel == mf.KERNEL_AUTO and
                                                         (p >= 4 or (p == 3 and (hn or nt == mf.F64))))):
        name = "apply_planes4" if planes4 else "apply_planes3"
        masked_in_pencils = hn and not _plane_kernel_exists(planes4, p + 1, nt, True, mass)
        return "ran", name + ("+apply_batches_x" if masked_in_pencils else "")
    if xk_ok:
        return "ran", "apply_batches_x"
    return "ran", ("apply_batches_g2" if dim == 2 else "apply_batches_g") if general else "apply_batches"


def suggest_renumbering(desc):
    out = np.zeros(desc.n_dofs, dtype=np.uint32)
    mf._check(mf.lib().mfgpu_suggest_renumbering(ctypes.byref(desc), out.ctypes.data))
    return out


def pass2_classes(plan):
    """the numbers of partial sums k of the plan's pass-2 groups"""
    return sorted(set((plan.chunks[:, 1] >> 16).tolist()))


def _check_plan(od, plan, colored):
    nd = od.nd
    order, bco, bdo, bdofs, lmap = plan.cell_order, plan.batch_cell_off, plan.batch_dof_off, plan.bdofs, plan.lmap
    np.testing.assert_array_equal(np.sort(order), np.arange(od.n_cells))
    assert bco[0] == 0 and bco[-1] == od.n_cells and bdo[0] == 0 and bdo[-1] == len(bdofs) and lmap.shape == (od.n_cells, nd)
    for b in range(len(bco) - 1):
        cells = np.arange(bco[b], bco[b + 1])
        assert len(cells) >= 1 and (lmap[cells] < bdo[b + 1] - bdo[b]).all()
        np.testing.assert_array_equal(bdofs[bdo[b]:bdo[b + 1]][lmap[cells]], od.loc2glob[order[cells]])
    cbo = plan.color_batch_off
    assert cbo[0] == 0 and cbo[-1] == len(bco) - 1
    if colored:
        for c in range(len(cbo) - 1):
            g = bdofs[bdo[cbo[c]]:bdo[cbo[c + 1]]]  # (a batch lists a dof once: checked above through lmap and below)
            per_batch = [np.unique(bdofs[bdo[b]:bdo[b + 1]]) for b in range(cbo[c], cbo[c + 1])]
            assert sum(len(u) for u in per_batch) == len(np.unique(g)), f"colour {c} is not conflict-free"


@pytest.mark.parametrize("kernel", KERNELS, ids=["auto", "pencils_x", "planes", "planes_2w"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_plans_of_transformed_descriptions(case, kernel):
    od = case.make()
    rng = np.random.default_rng(5)
    x, y0 = rng.standard_normal(od.n_dofs), rng.standard_normal(od.n_dofs)
    ref, ref_add = o.vmult(od, x), o.vmult_add(od, y0, x)
    atol = 1e-12 * np.abs(ref).max()
    if "holes" in case.tags:
        holes = np.setdiff1d(np.arange(od.n_dofs), np.union1d(od.loc2glob.reshape(-1), od.constrained))
        assert len(holes) > 0 and (ref[holes] == 0).all() and (ref_add[holes] == y0[holes]).all()
    if "repeated" in case.tags:
        assert any(len(np.unique(row)) < od.nd for row in od.loc2glob)
    if "all8" in case.tags:
        assert od.n_dofs == 8 and all(sorted(row) == list(range(8)) for row in od.loc2glob.tolist())
    for colored in (False, True):
        what, detail = expected_kernel(od, kernel, colored)
        desc, keep = desc_from_oracle(od, colored=colored, kernel=kernel, **case.kw)
        if what == "refused":
            assert kernel != mf.KERNEL_AUTO
            with pytest.raises(mf.MfgpuError, match=detail):
                mf.Plan(desc, keep)
            continue
        plan = mf.Plan(desc, keep)
        _check_plan(od, plan, colored)
        new_index = suggest_renumbering(desc)
        np.testing.assert_array_equal(np.sort(new_index), np.arange(od.n_dofs))
        plane_plan = len(plan.pr_dofs) > 0
        assert plane_plan == detail.startswith("apply_planes"), (detail, len(plan.pr_dofs))
        if "wraps" in case.tags and kernel == mf.KERNEL_AUTO and not colored:
            assert plane_plan  # (else the box seeding, whose walk wraps around the ring, is not exercised)
        for twopass in ([False] if colored else [True] if plane_plan else [True, False]):
            got = emulate_plan_vmult(od, plan, x, twopass=twopass)
            np.testing.assert_allclose(got, ref, rtol=0, atol=atol)
            got = emulate_plan_vmult(od, plan, x, y0, twopass=twopass)
            np.testing.assert_allclose(got, ref_add, rtol=0, atol=atol)
        if plane_plan and od.n <= 5:  # (the record layout the emulation knows: apply_planes3 / apply_planes4, p <= 4)
            np.testing.assert_allclose(emulate_plane_records_vmult(od, plan, x), ref, rtol=0, atol=atol)
            np.testing.assert_allclose(emulate_plane_records_vmult(od, plan, x, y0), ref_add, rtol=0, atol=atol)
        if "pinch" in case.tags and od.dim == 3 and not colored and ("k27" in case.tags or not plane_plan):
            # 27 one-cell batches (forced, or the pencil kernels' default on a mesh this small) all touch the pinched
            # vertex: a pass-2 class outside the unrolled {1, 2, 3, 4, 8} and beyond the 12 partial sums a shared
            # pass-2 record holds (kP2MaxK).  (The plane kernels' default batches hold 12 cells: 3 batches, k = 3.)
            ks = pass2_classes(plan)
            assert 27 in ks and any(k not in (1, 2, 3, 4, 8) for k in ks) and max(ks) > 12, ks
        if "all8" in case.tags and not colored:
            assert pass2_classes(plan) == [8]


def test_pinched_vertex_classes_in_2d():
    """36 one-cell batches (the default on a small 2D mesh) around one vertex: k = 36"""
    od = CASE["2d-pinch-p3"].make()
    desc, keep = desc_from_oracle(od)
    ks = pass2_classes(mf.Plan(desc, keep))
    assert max(ks) == 36 and max(ks) > 12, ks


def test_more_than_64_batch_colours_is_refused_loudly():
    """the documented limit of mfgpu_desc.loc2glob: a dof that more than 64 batches touch (here the pinched vertex of
    125 one-cell batches) needs more batch colours than the planner has -- an error, in either scatter mode"""
    od = _pinched(3, 2, (5, 5, 5))
    for colored in (False, True):
        desc, keep = desc_from_oracle(od, max_cells_per_batch=1, colored=colored)
        with pytest.raises(mf.MfgpuError, match="more than 64 batch colours needed") as e:
            mf.Plan(desc, keep)
        assert e.value.code == mf.EUNSUPPORTED


# ---- the helper against the oracle alone


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_assembled_matrix_of_every_case_is_symmetric(case):
    A = o.assemble(case.make())
    assert abs(A - A.T).max() <= 1e-13 * abs(A).max()


@pytest.mark.parametrize("name", ["torus-p4", "torus2-p1", "torus2-p2", "2d-torus-p4", "general-2d-torus-p4"])
def test_constants_are_in_the_null_space_on_a_torus(name):
    od = CASE[name].make()
    assert len(od.constrained) == 0
    A = o.assemble(od)
    assert np.abs(A @ np.ones(od.n_dofs)).max() <= 1e-13 * abs(A).sum(axis=1).max()


def test_periodic_identifies_faces_edges_and_corners():
    od = _box(3, 2, (2, 3, 2))
    t = tp.periodic(od, [0, 2])
    nd = t.desc
    assert nd.n_dofs == 4 * 7 * 4 and len(np.unique(t.dof_map)) == nd.n_dofs
    X = od.dof_coords
    for g in range(od.n_dofs):  # partners differ by whole periods in x and z only
        d = X[g] - nd.dof_coords[t.dof_map[g]]
        assert d[1] == 0 and all(abs(d[k]) < 1e-12 or abs(abs(d[k]) - np.ptp(X[:, k])) < 1e-12 for k in (0, 2))
    on_y = np.isclose(nd.dof_coords[:, 1], X[:, 1].min()) | np.isclose(nd.dof_coords[:, 1], X[:, 1].max())
    np.testing.assert_array_equal(nd.constrained, np.nonzero(on_y)[0])
    th = tp.periodic(od, [0, 2], compact=False)
    assert th.desc.n_dofs == od.n_dofs
    np.testing.assert_array_equal(tp.pull(th, np.arange(od.n_dofs)), th.dof_map)


def test_permutations_carry_the_operator():
    od = _box(2, 3, (3, 4))
    x = np.random.default_rng(0).standard_normal(od.n_dofs)
    ref = o.vmult(od, x)
    t1 = tp.permute_dofs(od, 1)
    assert not np.array_equal(t1.dof_map, np.arange(od.n_dofs))
    np.testing.assert_array_equal(t1.desc.constrained, np.sort(t1.dof_map[od.constrained]))
    np.testing.assert_allclose(tp.pull(t1, o.vmult(t1.desc, tp.push(t1, x))), ref, rtol=0, atol=1e-13 * np.abs(ref).max())
    t2 = tp.permute_cells(od, 2)
    np.testing.assert_array_equal(t2.desc.loc2glob, od.loc2glob[t2.cell_map])
    np.testing.assert_array_equal(t2.desc.coefficient, od.coefficient[t2.cell_map])
    np.testing.assert_array_equal(t2.desc.JxW, od.JxW[t2.cell_map])
    np.testing.assert_array_equal(t2.desc.inv_jac, od.inv_jac[t2.cell_map])
    np.testing.assert_allclose(o.vmult(t2.desc, x), ref, rtol=0, atol=1e-13 * np.abs(ref).max())
