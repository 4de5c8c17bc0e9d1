"""The integrator, the slab exchange, the vector operations of csrc/mfgpu_aux.hip and the solver objects (CG, VCycle) on
vectors inside red zones (tests/redzone.py; the operator is in test_gpu_redzone.py, the transfers and the level operator
in test_gpu_redzone_transfer.py).  Every caller-owned device array of a call is a payload between two zones of 4096 NaN
elements -- outputs, inputs, f / u_b / exact arrays, coefficient arrays, the inverse diagonal a CG borrows -- once 16-byte
aligned and once one element off.

References and tolerances are those of the entry points' own test files: poisson_reference / nonlinear_reference /
helmholtz_reference with 1e-12 relative to the largest entry (test_gpu_poisson.py, test_gpu_evaluate.py), the
single-domain oracle with TOL of test_gpu.py for the slabs, numpy with the bounds of
test_gpu_aux.py::test_vector_operations_match_numpy, cg_reference with the bounds of
test_gpu_cg.py::test_solve_to_convergence, mg_reference / gc_reference with VCYCLE_TOL of test_gpu_vcycle.py, and a fresh
V-cycle with REFRESH_TOL of test_gpu_refresh.py.  The integrator is double only."""
import copy
import functools

import numpy as np
import pytest

import gc_reference as gr
import helmholtz_reference as hr
import mg_reference as mg
import nonlinear_reference as nr
import pmg_reference as pmr
import poisson_reference as pr
import pymfgpu as mf
from oracle import mf_oracle as o
from redzone import Zoned
from test_gpu import TOL, rel
from test_gpu_cg import DEGREE, KIND, NT, RANGE, problem
from test_gpu_evaluate import integrator
from test_gpu_poisson import close, small_mesh
from test_gpu_refresh import REFRESH_TOL, apply_all, defects, field
from test_gpu_update_coefficients import positive, with_coefficient
from test_gpu_vcycle import VCYCLE_TOL
from util import oracle_desc_from_mesh

pytestmark = pytest.mark.gpu

F64, F32 = mf.F64, mf.F32
ALIGN = pytest.mark.parametrize("offset_one", [False, True], ids=["aligned", "offset"])
TYPES = pytest.mark.parametrize("nt", [F64, F32], ids=["f64", "f32"])


def typed(a, nt):
    return np.asarray(a).astype(mf.np_dtype(nt)).astype(np.float64)


# ---- the integrator (double)


@functools.lru_cache(maxsize=None)
def _integrator_reference(kind, dim, p):
    mesh = small_mesh(kind, dim, p)
    cells = pr.Cells(mesh)
    od = cells.od
    rng = np.random.default_rng(dim * 10 + p)
    ub = cells.lift()
    f = rng.standard_normal((od.n_cells, od.nd))
    u = rng.standard_normal(mesh.n_dofs)
    unread = np.ones(mesh.n_dofs, bool)
    unread[od.loc2glob.reshape(-1)] = False
    assert (kind == "hanging") == bool(unread.any())
    vals, grads = nr.evaluate(cells, np.where(unread, 0.0, u))
    u[unread] = np.nan  # the dofs no cell references are not read
    ui = cells.interpolant()
    exact = pr.solution(cells.xe) * (1.0 + 0.1 * rng.standard_normal(cells.xe.shape[:2]))  # (not the built-in function)
    l2, per_cell = cells.l2_error(ui, exact)
    a1, c0, c1 = positive(od, F64, 2), positive(od, F64, 3), positive(od, F64, 4)
    cells1 = copy.copy(cells)
    cells1.od = with_coefficient(od, a1)
    return dict(mesh=mesh, ub=ub, f=f, u=u, ui=ui, exact=exact, c0=c0, a1=a1, c1=c1, rhs=cells.rhs(f, ub), vals=vals,
                grads=grads, l2=l2, per_cell=per_cell, rhs_updated=hr.rhs(cells1, c1, f, ub))


@ALIGN
@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 2), ("hanging", 2, 2), ("cube", 3, 4), ("hanging", 3, 2), ("ball", 3, 2)])
def test_integrator_entry_points(kind, dim, p, offset_one):
    R = _integrator_reference(kind, dim, p)
    mesh = R["mesh"]
    N, nc, npts = mesh.n_dofs, mesh.n_cells, mesh.n_cells * mesh.nd
    Z = lambda a: Zoned(a, F64, offset_one)  # noqa: E731
    it = integrator(mesh)  # (MFGPU_UPDATABLE_COEFFICIENTS: evaluate's gradients need it)
    # rhs(dst, f, u_b)
    dst, f, ub = Z(N), Z(R["f"]), Z(R["ub"])
    it.rhs(dst.vec, f.vec, ub.vec)
    close(dst.result(), R["rhs"], 1e-12)
    f.unchanged()
    ub.unchanged()
    # l2_error(u, exact, per_cell)
    u, exact, per = Z(R["ui"]), Z(R["exact"]), Z(nc)
    l2 = it.l2_error(u.vec, exact.vec, per.vec)
    assert abs(l2 - R["l2"]) <= 1e-12 * R["l2"]
    close(per.result(), R["per_cell"], 1e-12)
    u.unchanged()
    exact.unchanged()
    # evaluate(u, values, gradients)
    u, vals, grads = Z(R["u"]), Z(npts), Z(npts * dim)
    it.evaluate(u.vec, vals.vec, grads.vec)
    close(vals.result(), R["vals"].reshape(-1), 1e-12)
    close(grads.result(), R["grads"].reshape(-1), 1e-12)
    u.unchanged()
    # update_coefficients(a, c) from zoned device arrays on an integrator with a mass term, then the lift
    mesh.set_mass_coefficient(R["c0"])
    try:
        it2 = integrator(mesh)
        a1, c1 = Z(R["a1"]), Z(R["c1"])
        it2.update_coefficients(a1.vec, c1.vec)
        a1.unchanged()
        c1.unchanged()
        dst = Z(N)
        it2.rhs(dst.vec, f.vec, ub.vec)
        close(dst.result(), R["rhs_updated"], 1e-12)
        f.unchanged()
        ub.unchanged()
        del it2
    finally:
        mesh.set_mass_coefficient(None)  # (the mesh is shared by the two variants of the case)


# ---- the slab exchange: in-process slabs against the single-domain oracle


@functools.lru_cache(maxsize=None)
def _slab_reference(p, n, world):
    """(x, A x, per slab the indices of its dofs in the whole mesh); x is what a float holds"""
    from pymfgpu.parallel import slab_ranges
    full = mf.Mesh.uniform(3, p, n)
    od = oracle_desc_from_mesh(full, dtype=np.float64)
    fx = full.dof_coords()
    axes = [np.unique(np.round(fx[:, d], 9)) for d in range(3)]
    mids = [0.5 * (a[:-1] + a[1:]) for a in axes]

    def where(c):  # per direction the index of the nearest grid coordinate
        idx = tuple(np.searchsorted(mids[d], c[:, d]) for d in range(3))
        assert all(np.abs(axes[d][idx[d]] - c[:, d]).max() < 1e-9 for d in range(3))
        return idx

    table = np.full([len(a) for a in axes], -1, dtype=np.int64)
    table[where(fx)] = np.arange(len(fx))
    ranges = list(slab_ranges(n, world))
    gi = []
    for r in ranges:
        slab = mf.Mesh.uniform(3, p, n, slab=r)  # (dof_coords is a view into the mesh: keep it while it is read)
        gi.append(table[where(slab.dof_coords())])
    assert all((g >= 0).all() and len(np.unique(g)) == len(g) for g in gi)
    x = typed(np.sin(3 * fx[:, 0]) + fx[:, 1] ** 2 - np.cos(2 * fx[:, 2]) * fx[:, 0], F32)
    return x, o.vmult(od, x), ranges, gi


@ALIGN
@TYPES
@pytest.mark.parametrize("p,n,world,first", [(4, 12, 2, "interface_first"), (4, 6, 2, None), (4, 6, 2, "round2"),
                                             (4, 24, 3, "hole")],
                         ids=["interface_first", "n6", "n6_round2", "hole"])
def test_slab_exchange(p, n, world, first, nt, offset_one):
    """One vmult_begin on all slabs, then vmult_end on all.  The slabs of uniform(3, 4, 6) are three cells thick: 6 of a
    slab's 9 or 10 batches are interior, so the library still runs them interface first ("n6", the schedule is printed
    and not asserted); with cell_loop_segments = 2 the same slabs take the round-2 schedule (csrc/mfgpu_dist.hip)."""
    x, ref, ranges, gis = _slab_reference(p, n, world)
    slabs = []
    for r, (rng_z, gi) in enumerate(zip(ranges, gis)):
        mesh = mf.Mesh.uniform(3, p, n, slab=rng_z, number_type=nt)
        if first == "round2":
            mesh.desc.cell_loop_segments = 2
        op, dist = mf.Operator(mesh.desc, mesh), mf.Dist(mesh, r, world)
        dist.attach(op)
        slabs.append(dict(mesh=mesh, op=op, dist=dist, gi=gi, a=Zoned(x[gi], nt, offset_one),
                          b=Zoned(mesh.n_dofs, nt, offset_one)))
    for lo, up in zip(slabs, slabs[1:]):
        lo["dist"].connect_local(up["dist"])
    for r, s in enumerate(slabs):
        ifirst, r1, r2, nb = s["dist"].schedule()
        print(f"slab {r}: interface_first {ifirst}, interior batches [{r1}, {r2}) of {nb}")
        if first == "round2":
            assert not ifirst
        elif first is not None:
            assert ifirst and 0 <= r1 < r2 <= nb and (r1 == 0) == (r == 0) and (r2 == nb) == (r == world - 1)
        if first == "hole" and r == 1:  # the middle slab's two interface ranges: one launch with a hole
            assert 0 < r1 < r2 < nb
    for s in slabs:
        s["dist"].vmult_begin(s["op"], s["b"].vec, s["a"].vec)
    for s in slabs:
        s["dist"].vmult_end(s["op"], s["b"].vec)
    for s in slabs:
        e = rel(s["b"].result(), ref[s["gi"]])
        s["a"].unchanged()
        assert e <= TOL[nt], e


# ---- the vector operations of mfgpu_aux.hip


@ALIGN
@TYPES
@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 3])
def test_vector_operations(n, nt, offset_one):
    """test_gpu_aux.py::test_vector_operations_match_numpy with every vector in zones; a reduction that reads one
    element too far returns NaN"""
    rng = np.random.default_rng(n)
    t = mf.np_dtype(nt)
    a, b, c = (rng.standard_normal(n).astype(t) for _ in range(3))
    b[np.abs(b) < 0.1] = 0.5  # divisor / inverted vector away from 0
    tol = 1e-13 if nt == F64 else 1e-6
    Z = lambda v: Zoned(v, nt, offset_one)  # noqa: E731
    za, zb, zc, zf = Z(a), Z(b), Z(c), Z(n)
    va, vb, vc = za.vec, zb.vec, zc.vec
    zf.vec.fill(2.5)
    np.testing.assert_array_equal(zf.result(), np.full(n, 2.5, dtype=t))
    va.sadd(0.5, -2.0, vb)
    ref = (t(0.5) * a + t(-2.0) * b).astype(t)
    np.testing.assert_allclose(za.result(), ref, rtol=tol, atol=tol)
    va.equ(3.0, vc)
    np.testing.assert_array_equal(za.result(), t(3.0) * c)
    va.scale(vb)
    ref = (t(3.0) * c) * b
    np.testing.assert_allclose(za.result(), ref, rtol=tol)
    va.divide(vb)
    ref = ref / b
    np.testing.assert_allclose(za.result(), ref, rtol=tol)
    zb.unchanged()
    zc.unchanged()
    vb.invert()
    np.testing.assert_allclose(zb.result(), t(1.0) / b, rtol=tol)
    va.mul(-0.25)
    ref = t(-0.25) * ref
    np.testing.assert_allclose(za.result(), ref, rtol=tol)
    # reductions
    x, y = za.result().astype(np.float64), c.astype(np.float64)
    rtol = 1e-12 if nt == F64 else 1e-6
    d1 = va.dot(vc)
    assert d1 == va.dot(vc)
    assert abs(d1 - x @ y) <= rtol * np.linalg.norm(x) * np.linalg.norm(y)
    assert abs(va.l2_norm() - np.linalg.norm(x)) <= rtol * np.linalg.norm(x)
    r = va.add_and_dot(0.5, vc, vb)  # va += 0.5 vc ; va . vb
    x2 = za.result().astype(np.float64)
    np.testing.assert_allclose(x2, (x.astype(t) + t(0.5) * c).astype(np.float64), rtol=tol, atol=tol)
    z = zb.result().astype(np.float64)
    assert abs(r - x2 @ z) <= rtol * np.linalg.norm(x2) * np.linalg.norm(z)
    assert not va.all_zero()
    va.mul(0.0)
    assert va.all_zero()
    za.result()
    zc.unchanged()


# ---- CG.solve


@ALIGN
@pytest.mark.parametrize("dt,tol,bound", [(np.float64, 1e-10, 2e-10), (np.float32, 1e-4, 2e-4)], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["jacobi", "chebyshev"])
def test_cg_solve(kind, dt, tol, bound, offset_one):
    """test_gpu_cg.py::test_solve_to_convergence on uniform(3, 2, 4) with x, b and the borrowed inverse diagonal zoned"""
    P = problem(3, 2, 4)
    nt = NT[dt]
    b = P.rhs(1)
    tolerance = tol * np.linalg.norm(b)
    hist = list(P.reference(kind, dt, b, tolerance, 10000))
    ref_it, ref_status, ref_res, _ = hist[-1]
    assert ref_status == 1 and ref_res <= tolerance < hist[-2][2]
    dinv, zb, zx = Zoned(P.dinv, nt, offset_one), Zoned(b, nt, offset_one), Zoned(P.N, nt, offset_one)
    cg = mf.CG(P.op(dt), KIND[kind], dinv.vec, DEGREE, P.lambda_max, RANGE)
    info = cg.solve(zx.vec, zb.vec, tolerance, 10000, check_every=5)  # (begin writes every entry of x)
    x = zx.result()
    zb.unchanged()
    dinv.unchanged()
    true = np.linalg.norm(b - P.A @ x.astype(np.float64)) / np.linalg.norm(b)
    print(f"iterations {info.iterations} (reference {ref_it}), true residual {true:.3e} (bound {bound:.0e})")
    assert info.status == 1 and abs(int(info.iterations) - ref_it) <= 1
    assert info.residual <= tolerance and true <= bound


# ---- the V-cycle objects: active vectors z, r in zones (double), levels in double and in float


@functools.lru_cache(maxsize=None)
def _hierarchy_reference(n_ref):
    ref = mg.Hierarchy(3, 2, n_ref)
    R = defects(ref.mesh, 320 + n_ref)
    return ref, R, ref.vcycle(R)


def _apply_zoned(V, R, offset_one):
    out = []
    for k in range(R.shape[1]):
        z, r = Zoned(R.shape[0], F64, offset_one), Zoned(R[:, k], F64, offset_one)  # z starts as NaN
        V.apply(z.vec, r.vec)
        out.append(z.result())
        r.unchanged()
        assert np.isfinite(out[-1]).all()
    return np.stack(out, axis=1)


# n_ref = 3 is the root cell and its eight children: two levels, no refinement edge, no hanging node.  n_ref = 4 is the
# smallest at which the hierarchy has refinement edges and the mesh hanging nodes (test_gpu_vcycle.py, test_gpu_gc.py).
N_REF = pytest.mark.parametrize("n_ref", [3, 4], ids=["r3", "r4"])


@ALIGN
@N_REF
@pytest.mark.parametrize("nt", [F64, F32], ids=["double_levels", "float_levels"])
def test_vcycle_from_hierarchy(nt, n_ref, offset_one):
    ref, R, Z = _hierarchy_reference(n_ref)
    V = mf.VCycle.from_hierarchy(mf.Mesh.adaptive_mg(3, 2, n_ref, number_type=nt), nt, F64, lambda_max=ref.lmax)
    assert V.n_levels == ref.n_levels and any(len(E) for E in ref.edge) == (n_ref == 4)
    got = _apply_zoned(V, R, offset_one)
    errs = [rel(got[:, k], Z[:, k]) for k in range(R.shape[1])]
    print("V-cycle from_hierarchy, rel l2 from the numpy reference:", errs)
    assert max(errs) <= VCYCLE_TOL[nt], errs


@functools.lru_cache(maxsize=None)
def _gc_reference(n_ref):
    mesh = mf.Mesh.adaptive(3, 2, n_ref)
    meshes = mf.Mesh.coarsening_sequence(mesh, 1) + [mesh]
    return gr.level_hierarchy_gc(meshes), defects(mesh, 120 + n_ref)


@ALIGN
@N_REF
@pytest.mark.parametrize("nt", [F64, F32], ids=["double_levels", "float_levels"])
def test_vcycle_from_global_coarsening(nt, n_ref, offset_one):
    model, R = _gc_reference(n_ref)
    V = mf.VCycle.from_global_coarsening(mf.Mesh.adaptive(3, 2, n_ref, number_type=nt), (1, 2), F64)
    ref = pmr.with_lambda_max(model, V.lambda_max())  # estimated lambda_max
    assert V.n_levels == ref.n_levels and [int(M.desc.degree) for M in ref.meshes][-2:] == [1, 2]
    assert [M.n_cells for M in ref.meshes] == {3: [8, 8], 4: [8, 22, 78, 253, 736, 736]}[n_ref]
    got = _apply_zoned(V, R, offset_one)
    want = ref.vcycle(R)
    errs = [rel(got[:, k], want[:, k]) for k in range(R.shape[1])]
    print("V-cycle from_global_coarsening, rel l2 from the numpy model:", errs)
    assert max(errs) <= VCYCLE_TOL[nt], errs


@ALIGN
@pytest.mark.parametrize("nt", [F64, F32], ids=["double_levels", "float_levels"])
def test_vcycle_refresh_then_apply(nt, offset_one):
    """test_gpu_refresh.py::test_refreshed_is_fresh on adaptive_mg(3, 2, 3): the new coefficient comes from zoned device
    arrays, the refreshed object is applied to zoned vectors and compared with a fresh object"""
    mesh = mf.Mesh.adaptive_mg(3, 2, 3, number_type=nt)
    levels, keep = mf.VCycle.hierarchy_levels(mesh, flags=mf.UPDATABLE_COEFFICIENTS)
    meshes, N = keep[2], mesh.n_dofs
    V = mf.VCycle(levels, F64, N, coarse=mf.VCYCLE_COARSE_DENSE, keep=keep)
    R = defects(mesh, 7)
    coefs = []
    for lev, M in zip(levels, meshes):
        c = Zoned(field(1)(M.arrays()["quadrature_points"].astype(np.float64)), nt, offset_one)
        lev["op"].update_coefficients(c.vec, None)
        coefs.append(c)
    for c in coefs:
        c.unchanged()
    stale = apply_all(V, R)
    V.refresh(eig_steps=200)
    info = V.refresh_status()
    assert info.coarse_status == 0 and info.eig_status_max == 1 and 15 <= info.eig_steps_max <= 200
    W = mf.VCycle(levels, F64, N, coarse=mf.VCYCLE_COARSE_DENSE, keep=keep)
    want, got = apply_all(W, R), _apply_zoned(V, R, offset_one)
    err = max(rel(got[:, j], want[:, j]) for j in range(3))
    moved = min(rel(stale[:, j], want[:, j]) for j in range(3))
    print(f"refreshed against fresh: {err:.3e}; before the refresh {moved:.3e}")
    assert moved > 100 * REFRESH_TOL[nt]  # otherwise the coefficient change proves nothing
    assert err <= REFRESH_TOL[nt]
