"""Every entry point with the library's OWN device arrays guarded and poisoned (mfgpu_debug_guard_*, include/mfgpu.h).

tests/redzone.py puts the caller's vectors between red zones; here the arrays a handle allocates itself -- halo, batch
arrays, workspaces, the solvers' vectors -- sit between two guards of GUARD bytes of 0xFF, and every payload the library
allocates without filling it (DESIGN.md section 8 lists them) is 0xFF too: a NaN as double and as float.  GUARD is the
zone of tests/redzone.py in bytes, 4096 * 8: a condition taken from there, not a measurement -- more than the longest
per-batch dof list any kernel walks (p_kgu(7) * 64 slots).

A scenario is a function that creates its handles, runs every call twice and compares each result with the reference
and at the tolerance of the entry point's own test file (a NaN fails every comparison).  guarded() runs it once with
the mode off and once inside the mode, and then
  - compares the second call with the first bit for bit wherever the header declares the call bitwise repeatable,
  - compares the guarded results with the unguarded ones, bit for bit where repeatable and at the tolerance elsewhere
    (the payload alignment is the same, so is the arithmetic),
  - asks guard_check(), which raises with the report if any guard byte changed,
  - destroys the handles and asserts that the number of registered arrays is back where it was.
The first test shows that the detector detects: the library's self-test plants one damage behind and one in front of a
payload, inside its own allocation.  The module captures no graphs (an allocation in guard mode fills on the null stream)."""
import contextlib
import functools
import gc
import re
import types

import numpy as np
import pytest

import amr_reference as ar
import gc_reference as gr
import mg_reference as mg
import nonlinear_reference as nr
import pmg_reference as pmr
import points_reference as ptr
import poisson_reference as pr
import pymfgpu as mf
from oracle import mf_oracle as o
from test_gpu import KERNELS, TOL, rel
from test_gpu_adapt import reference as interp_reference
from test_gpu_aux import TOL as DIAG_TOL
from test_gpu_cg import DEGREE, ITERATE_TOL, KIND, NT, RANGE, problem
from test_gpu_evaluate import integrator
from test_gpu_gc import pair as gc_pair
from test_gpu_level import _edge_of_box
from test_gpu_locate import XI_TOL, device_locate
from test_gpu_multi import TOL as MULTI_TOL, run_multi, vectors
from test_gpu_pmg import TRANSFER_TOL, dev, hybrid_defects, hybrid_meshes, mesh_pair, model as pmg_model, rel as rel0
from test_gpu_poisson import small_mesh
from test_gpu_redzone import (_adaptive, _ball, _deformed_adaptive, _mesh_row, _oracle_row, _reference, _uniform, _vectors,
                              typed)
from test_gpu_redzone_solvers import _gc_reference
from test_gpu_redzone_transfer import _gc_matrix, _gc_pair, _p_hn_matrix, _p_matrix
from test_gpu_refresh import REFRESH_TOL, apply_all, defects, field
from test_gpu_update_coefficients import positive, with_coefficient
from test_gpu_vcycle import VCYCLE_TOL, make_vcycle, vcycle_reference
from test_points_host import one_refined
from util import deform, deformed_oracle_desc, desc_from_oracle, oracle_desc_from_mesh

pytestmark = pytest.mark.gpu

F64, F32 = mf.F64, mf.F32
GUARD = 4096 * 8
TYPES = pytest.mark.parametrize("nt", [F64, F32], ids=["f64", "f32"])


@pytest.fixture(scope="module", autouse=True)
def guard_mode():
    with mf.guards(GUARD):
        yield


@contextlib.contextmanager
def mode_off():
    mf.lib().mfgpu_debug_guard_end()
    try:
        yield
    finally:
        assert mf.lib().mfgpu_debug_guard_begin(GUARD) == 0


# ---- error measures: each returns a number that is NaN (and fails) when a NaN got in


def max_rel(got, want):
    """largest difference relative to the largest reference entry (close() of tests/test_gpu_poisson.py)"""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def elementwise(got, want):
    """largest elementwise relative difference (assert_allclose(rtol) of tests/test_gpu_aux.py)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / np.abs(want)).max())


def max_abs(got, want):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    return float(d.max()) if d.size else 0.0


def unequal(got, want):
    """0 if every entry equals the reference's, converted to the result's type; else 1"""
    return 0.0 if np.array_equal(got, np.asarray(want).astype(got.dtype)) else 1.0


def rows_rel(got, want):
    return max(rel(g, w) for g, w in zip(got, want))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Run:
    """what one execution of a scenario leaves: its results by name and the handles it created"""

    def __init__(self):
        self.results, self.notes, self.handles = {}, {}, []

    def own(self, *handles):
        self.handles.extend(handles)
        return handles[0] if len(handles) == 1 else handles

    def twice(self, name, call, want, tol, err=rel, exact=False):
        """call() runs the entry point on fresh outputs and returns the result on the host.  exact: the header declares
        the call bitwise repeatable"""
        first, second = call(), call()
        for k, got in enumerate((first, second)):
            e = err(got, want)
            assert e <= tol, (name, "call", k, e, tol, int(np.isnan(np.asarray(got, np.float64)).sum()))
        if exact:
            assert same_bits(first, second), (name, "the second call differs from the first")
        assert name not in self.results
        self.results[name] = (first, err, tol, exact)

    def note(self, name, value):
        self.notes[name] = value

    def close(self):
        for h in reversed(self.handles):
            getattr(h, "destroy", None) and h.destroy()
            getattr(h, "clear", None) and h.clear()
            h.__del__()
        self.handles.clear()
        gc.collect()


def guarded(scenario, *args):
    gc.collect()
    live0 = mf.guard_check()
    with mode_off():
        plain = Run()
        scenario(plain, *args)
        assert mf.guard_check() == live0  # arrays allocated outside the mode are not registered
        plain.close()
    run = Run()
    scenario(run, *args)
    live = mf.guard_check()  # raises with the report when a guard byte changed
    assert live > live0, "the scenario allocated nothing inside the mode"
    assert run.notes == plain.notes
    assert list(run.results) == list(plain.results) and run.results
    for name, (got, err, tol, exact) in run.results.items():
        ref = plain.results[name][0]
        if exact:
            assert same_bits(got, ref), (name, "differs from the run outside the mode")
        else:
            e = err(got, ref)
            assert e <= tol, (name, "against the run outside the mode", e, tol)
    run.close()
    assert mf.guard_check() == live0, "arrays are still registered after their handles were destroyed"


# ---- the detector detects


def test_selftest_reports_exactly_the_two_planted_damages():
    gc.collect()
    live0 = mf.guard_check()
    n_damaged, report, poisoned_ok, zeroed_ok = mf.guard_selftest()
    print(report)
    assert poisoned_ok, "an unfilled payload of doubles did not read back as 0xFF bytes"
    assert zeroed_ok, "a zero-filled payload did not read back as zeros"
    lines = report.splitlines()
    assert n_damaged == 2 and len(lines) == 2, report
    front = re.fullmatch(r"array #(\d+) \(296 payload bytes\): front guard, offset -1: 0x5a", lines[0])
    back = re.fullmatch(r"array #(\d+) \(296 payload bytes\): back guard, offset \+0: 0x5a", lines[1])
    assert front and back and front.group(1) == back.group(1), report
    assert mf.guard_check() == live0  # the self-test freed its arrays, and nothing else is damaged


def test_arrays_from_before_the_mode_are_not_registered_and_later_ones_stay():
    gc.collect()
    live0 = mf.guard_check()
    with mode_off():
        mesh = mf.Mesh.uniform(3, 2, 3)
        before = mf.Operator(mesh.desc, mesh)
        assert mf.guard_check() == live0
    inside = mf.Operator(mesh.desc, mesh)
    live = mf.guard_check()
    assert live > live0
    assert inside.memory_consumption() == before.memory_consumption()  # payload bytes only
    with mode_off():
        assert mf.guard_check() == live  # still registered, and checked, after the mode was switched off
        inside.clear()
        assert mf.guard_check() == live0
    before.clear()
    assert mf.guard_check() == live0


# ---- the operator: vmult, vmult_add, compute_inverse_diagonal, set_constrained_values, update_coefficients


def _flagged(make_mesh, flags):
    def make(nt):
        mesh = make_mesh(nt)
        mesh.desc.flags |= flags
        return mesh
    return make


def _kernel_knobs(p):
    """(tag, knobs) of every cell-loop kernel family and scatter mode that serves a 3D conforming mesh at degree p:
    KERNELS and the coloured mode of tests/test_gpu.py (the plane kernels exist at p = 2..4 and p = 2..6)"""
    out = [("auto", {})]
    for kern, name in KERNELS:
        if (name == "apply_planes3" and not 2 <= p <= 4) or (name == "apply_planes4" and p < 2):
            continue
        out.append((name, dict(kernel=kern)))
    return out + [("colored", dict(colored=True))]


def _operator_rows():
    rows = []
    for p in (1, 2, 4, 6):  # 2D, n = 5: 25 cells
        rows += [(f"cube2d_p{p}_n5", _mesh_row(_uniform(2, p, 5)), "L"),
                 (f"cube2d_p{p}_n5_colored", _mesh_row(_uniform(2, p, 5), colored=True), "L")]
    for p, n in [(p, 3) for p in range(1, 7)] + [(4, 7)]:
        for tag, knobs in _kernel_knobs(p):
            rows.append((f"cube_p{p}_n{n}_{tag}", _mesh_row(_uniform(3, p, n), **knobs), "L"))
    # the record forms of tests/test_gpu_shared_records.py and the segmented cell loop of tests/test_gpu_segments.py
    rows += [("cube_p4_n12_shared", _mesh_row(_uniform(3, 4, 12)), "L"),
             ("cube_p4_n12_expanded", _mesh_row(_flagged(_uniform(3, 4, 12), mf.NO_SHARED_RECORDS)), "L"),
             ("cube_p4_n12_shared_wgs3", _mesh_row(_uniform(3, 4, 12), max_workgroups=3), "L"),
             ("cube_p4_n7_segments2", _mesh_row(_uniform(3, 4, 7), cell_loop_segments=2), "L"),
             ("cube_p4_n7_segments3_wgs3", _mesh_row(_uniform(3, 4, 7), cell_loop_segments=3, max_workgroups=3), "L")]
    # batches of several chunks of cells: the limits of test_gpu.py::test_pencil_kernels_multi_chunk_batches
    for p, n, cells in [(1, 12, 256), (2, 10, 256), (3, 8, 256), (4, 6, 27), (5, 4, 256), (6, 3, 256)]:
        for kern, name in KERNELS[:2]:
            rows.append((f"chunks_p{p}_n{n}_{name}", _mesh_row(_uniform(3, p, n), kernel=kern, max_cells_per_batch=cells), "L"))
    for p in (2, 4, 5):  # hanging-node batches
        rows += [(f"adaptive_p{p}_r4", _mesh_row(_adaptive(3, p, 4)), "LM" if p == 4 else "LA" if p == 2 else "L"),
                 (f"adaptive_p{p}_r4_pencils", _mesh_row(_adaptive(3, p, 4), kernel=mf.KERNEL_PENCILS), "L"),
                 (f"adaptive_p{p}_r4_colored", _mesh_row(_adaptive(3, p, 4), colored=True), "L")]
    rows.append(("adaptive2d_p4_r4", _mesh_row(_adaptive(2, 4, 4)), "L"))
    for p, n in [(2, 4), (4, 2), (5, 2)]:  # general geometry
        rows.append((f"deformed_p{p}_n{n}", _oracle_row(lambda p=p, n=n: deformed_oracle_desc(p, n, seed=10 * p + n)),
                     "LMU" if p == 2 else "L"))
    rows += [("deformed2d_p4_n6", _oracle_row(lambda: deform(o.uniform_mesh_desc(2, 4, 6), eps=0.15, seed=46)), "LM"),
             ("deformed_adaptive_p2_r4", _oracle_row(_deformed_adaptive(3, 2, 4)), "L")]
    for dim in (2, 3):
        for p in (2, 4):
            rows.append((f"ball{dim}d_p{p}_r1", _mesh_row(_ball(dim, p, 1)), "LMA" if (dim, p) == (3, 2) else "L"))
    rows.append(("cube_p2_n5", _mesh_row(_uniform(3, 2, 5)), "MU"))
    rows.append(("cube_p4_n7", _mesh_row(_uniform(3, 4, 7)), "M"))
    return rows


# L: the Laplacian; M: with a mass term; U: a and c replaced through update_coefficients; A: a replaced (no mass term)
MODES = {"L": ("laplace", False, False), "M": ("mass", True, False), "U": ("updated", True, True),
         "A": ("updated_a", False, True)}
OPERATOR_ROWS = _operator_rows()
OPERATOR_CASES = [pytest.param(i, m, id=f"{row[0]}-{MODES[m][0]}") for i, row in enumerate(OPERATOR_ROWS) for m in row[2]]
assert len({row[0] for row in OPERATOR_ROWS}) == len(OPERATOR_ROWS)


def operator_scenario(run, i, m, nt):
    name, build, _ = OPERATOR_ROWS[i]
    _, mass, updated = MODES[m]
    op, od, c = build(nt, mass, updated)
    run.own(op)
    n = od.n_dofs
    assert op.n() == n
    run.note("kernel", op.kernel_name())
    run.note("plan", str(op.plan_stats()))
    if updated:
        a1 = positive(od, nt, 21)
        c1 = positive(od, nt, 22) if mass else None
        da, dc = dev(a1.reshape(-1), nt), (dev(c1.reshape(-1), nt) if mass else None)
        op.update_coefficients(da, dc)
        mf.synchronize()  # (the device arrays are read when the stream gets there)
        od, c = with_coefficient(od, a1), c1
    x, y0 = _vectors(n, nt)
    want_y, want_add, want_diag = _reference(("guards", name, m, nt), od, c, x, y0)
    src = dev(x, nt)

    def vmult():
        dst = mf.DeviceVector(n, nt)
        dst.fill(7.0)  # vmult overwrites
        op.vmult(dst, src)
        mf.synchronize()
        return dst.to_host()

    def vmult_add():
        dst = dev(y0, nt)
        op.vmult_add(dst, src)
        mf.synchronize()
        return dst.to_host()

    def diagonal():
        d = mf.DeviceVector(n, nt)
        d.fill(np.nan)  # every entry is written
        op.compute_inverse_diagonal(d)
        mf.synchronize()
        return d.to_host()

    def constrained():
        v = dev(x, nt)
        op.set_constrained_values(v, -3.5)
        mf.synchronize()
        return v.to_host()

    run.twice("vmult", vmult, want_y, TOL[nt])
    run.twice("vmult_add", vmult_add, want_add, TOL[nt])
    assert np.isfinite(want_diag).all()
    run.twice("compute_inverse_diagonal", diagonal, want_diag, DIAG_TOL[nt], err=elementwise)
    want_c = x.copy()
    want_c[od.constrained] = -3.5
    run.twice("set_constrained_values", constrained, want_c, 0.0, err=unequal)
    np.testing.assert_array_equal(src.to_host(), x.astype(mf.np_dtype(nt)))  # src untouched
    run.note("memory_consumption", op.memory_consumption())  # (after the first diagonal: its tables count)


@TYPES
@pytest.mark.parametrize("i,m", OPERATOR_CASES)
def test_operator(i, m, nt):
    guarded(operator_scenario, i, m, nt)


# ---- vmult_multi: 5 vectors in fused groups of 3 + 2


def multi_scenario(run, p, nt):
    mesh = mf.Mesh.ball(3, p, 1, number_type=nt)
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    op = run.own(mf.Operator(mesh.desc, mesh))
    assert op.kernel_name() == "apply_batches_g" and mf.multi_groups(5, [3, 2]) == [3, 2]
    X, Y0 = vectors(mesh.n_dofs, nt, 5 + p, 5), vectors(mesh.n_dofs, nt, 50 + p, 5)
    key = ("multi", p, nt)
    if key not in _multi_cache:
        _multi_cache[key] = (np.stack([o.vmult(od, v) for v in X]), np.stack([o.vmult_add(od, w, v) for v, w in zip(X, Y0)]))
    want, want_add = _multi_cache[key]
    run.twice("vmult_multi", lambda: run_multi(op, X, nt, stride=mesh.n_dofs + 5, mode=mf.MULTI_FUSED), want, MULTI_TOL[nt],
              err=rows_rel)
    run.twice("vmult_multi_add", lambda: run_multi(op, X, nt, mode=mf.MULTI_FUSED, Y0=Y0), want_add, MULTI_TOL[nt],
              err=rows_rel)
    assert op.multi_width() == 3
    run.note("memory_consumption", op.memory_consumption())  # (with the halo buffers of the fused groups)


_multi_cache = {}


@TYPES
@pytest.mark.parametrize("p", [2, 4])
def test_vmult_multi_fused(p, nt):
    guarded(multi_scenario, p, nt)


# ---- the level operator with refinement edges, and its coefficient update


@functools.lru_cache(maxsize=None)
def _level_reference(dim, p, n, touch_boundary, nt):
    mesh = mf.Mesh.uniform(dim, p, n, number_type=nt)
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    h = 2.0 / n
    edge = _edge_of_box(mesh, -1.0 + (0.0 if touch_boundary else h), -1.0 + h * (n // 2 + 1))
    assert 0 < len(edge) < mesh.n_dofs and bool(len(np.intersect1d(edge, od.constrained))) == touch_boundary
    x = typed(np.random.default_rng(dim * 10 + p).standard_normal(mesh.n_dofs), nt)
    coefs = positive(od, nt, 1), positive(od, nt, 2)
    wants = []
    for a in coefs:
        oda = with_coefficient(od, a)
        odc = mg.with_constrained(oda, np.union1d(od.constrained, edge))
        wants.append((o.vmult(odc, x), o.vmult_interface_down(oda, edge, x), o.vmult_interface_up(oda, edge, x),
                      o.compute_inverse_diagonal(odc)))
    return mesh, od, edge, x, coefs, wants


def level_scenario(run, dim, p, n, touch_boundary, nt):
    mesh, od, edge, x, coefs, wants = _level_reference(dim, p, n, touch_boundary, nt)
    desc, keep = desc_from_oracle(with_coefficient(od, coefs[0]), number_type=nt)
    desc.flags |= mf.UPDATABLE_COEFFICIENTS
    lev = run.own(mf.Level(desc, edge, keep))
    N, src = od.n_dofs, dev(x, nt)

    def call(fn, fill):
        def go():
            dst = mf.DeviceVector(N, nt)
            dst.fill(fill)
            fn(dst, src) if fn != lev.compute_inverse_diagonal else fn(dst)
            mf.synchronize()
            return dst.to_host()
        return go

    for step, want in enumerate(wants):
        if step:
            lev.update_coefficients(dev(coefs[1].reshape(-1), nt), None)
            mf.synchronize()
        for fn, ref in zip((lev.vmult, lev.vmult_interface_down, lev.vmult_interface_up, lev.compute_inverse_diagonal), want):
            run.twice(f"{fn.__name__}{'_updated' if step else ''}", call(fn, 5.0), ref, TOL[nt])


@TYPES
@pytest.mark.parametrize("touch_boundary", [False, True])
@pytest.mark.parametrize("dim,p,n", [(2, 2, 8), (3, 4, 4)])
def test_level_operator(dim, p, n, touch_boundary, nt):
    guarded(level_scenario, dim, p, n, touch_boundary, nt)


# ---- the five transfer kinds


@functools.lru_cache(maxsize=None)
def _h_matrix(p):
    c, f = mf.Mesh.uniform(3, p, 2), mf.Mesh.uniform(3, p, 4)
    cd, fd = c.transfer_patches(f)
    con = c.arrays()["constrained_dofs"].astype(np.int64)
    return mg.transfer_matrix(3, p, cd, fd, c.n_dofs, f.n_dofs, con), con


@functools.lru_cache(maxsize=None)
def _interp_pair_matrix(p):
    _, c, f = gc_pair("2d_center", p)
    return gr.mesh_pair_matrix_gc(c, f), c.arrays()["constrained_dofs"].astype(np.int64)


def _transfer(kind, p, nt):
    """(transfer, P, coarse Dirichlet dofs, J or None) of the smallest pair the kind's own test file uses"""
    if kind == "h":
        c, f = mf.Mesh.uniform(3, p, 2, number_type=nt), mf.Mesh.uniform(3, p, 4, number_type=nt)
        return (mf.Transfer.from_meshes(c, f),) + _h_matrix(p) + (None,)
    if kind == "p":
        pc, pf = (1, 2) if p == 1 else (4, 5)
        c, f = mesh_pair("cube", 3, pc, pf, nt)
        return (mf.Transfer.p_from_meshes(c, f),) + _p_matrix(3, pc, pf) + (None,)
    if kind == "p_hn":
        pc, pf = (1, 2) if p == 1 else (2, 4)
        c, f = mf.Mesh.adaptive(3, pc, 4, number_type=nt), mf.Mesh.adaptive(3, pf, 4, number_type=nt)
        return (mf.Transfer.p_hn_from_meshes(c, f),) + _p_hn_matrix(pc, pf) + (None,)
    if kind == "h_hn":
        c, f, _ = _gc_pair(p, "finest", nt)
        return (mf.Transfer.h_hn_from_meshes(c, f),) + _gc_matrix(p, "finest") + (None,)
    _, c, f = gc_pair("2d_center", p, nt)
    return (mf.Transfer.h_hn_interp_from_meshes(c, f),) + _interp_pair_matrix(p) + (interp_reference("2d_center", p, True)[0],)


def transfer_scenario(run, kind, p, nt):
    t, P, con, J = _transfer(kind, p, nt)
    run.own(t)
    tol = TRANSFER_TOL[nt]
    nf, nc = P.shape
    rng = np.random.default_rng(nf * 1000 + nc)
    x, y, z = (typed(rng.standard_normal(n), nt) for n in (nc, nf, nc))
    src, fsrc = dev(x, nt), dev(y, nt)

    def prolongate():
        fine = mf.DeviceVector(nf, nt)
        fine.fill(3.0)  # overwritten
        t.prolongate(fine, src)
        mf.synchronize()
        return fine.to_host()

    def prolongate_add():
        acc = dev(y, nt)
        t.prolongate_add(acc, src)
        mf.synchronize()
        return acc.to_host()

    def restrict_and_add():
        coarse = dev(z, nt)
        t.restrict_and_add(coarse, fsrc)
        mf.synchronize()
        got = coarse.to_host()
        np.testing.assert_array_equal(got[con], z[con].astype(got.dtype))  # Dirichlet entries: not touched
        return got

    def interpolate():
        dst = mf.DeviceVector(nc, nt)
        dst.fill(3.0)
        t.interpolate(dst, fsrc)
        mf.synchronize()
        return dst.to_host()

    run.twice("prolongate", prolongate, P @ x, tol, err=rel0)
    run.twice("prolongate_add", prolongate_add, y + P @ x, tol, err=rel0, exact=True)  # "no atomics: deterministic"
    run.twice("restrict_and_add", restrict_and_add, z + P.T @ y, tol, err=rel0)  # floating-point atomics
    if J is not None:
        run.twice("interpolate", interpolate, J @ y, tol, err=rel0, exact=True)  # "the same bits on two calls"
    np.testing.assert_array_equal(src.to_host(), x.astype(mf.np_dtype(nt)))
    np.testing.assert_array_equal(fsrc.to_host(), y.astype(mf.np_dtype(nt)))
    run.note("memory_consumption", t.memory_consumption())


@TYPES
@pytest.mark.parametrize("p", [1, 4])
@pytest.mark.parametrize("kind", ["h", "p", "p_hn", "h_hn", "h_hn_interp"])
def test_transfer(kind, p, nt):
    guarded(transfer_scenario, kind, p, nt)


# ---- the integrator (double): rhs, the error integrals, evaluate with gradients, the recovery indicator


def _integrator_mesh(kind, dim, p):
    if kind == "hanging":  # 2^dim cells, the first one refined once: 7 / 15 leaves
        return mf.Mesh.from_leaves(dim, p, one_refined(dim))
    return small_mesh(kind, dim, p)


@functools.lru_cache(maxsize=None)
def _integrator_reference(kind, dim, p):
    mesh = _integrator_mesh(kind, dim, p)
    cells = pr.Cells(mesh)
    od = cells.od
    rng = np.random.default_rng(dim * 10 + p + len(kind))
    ub = cells.lift()
    f = rng.standard_normal((od.n_cells, od.nd))
    u = rng.standard_normal(mesh.n_dofs)
    unread = ptr.unread_dofs(mesh)
    assert (kind == "hanging") == bool(unread.any())
    u0 = np.where(unread, 0.0, u)
    vals, grads = nr.evaluate(cells, u0)
    weight = rng.uniform(0.5, 2.0, (od.n_cells, od.nd))
    eta, eta_w = ar.recovery_indicator(cells, u0), ar.recovery_indicator(cells, u0, weight)
    u[unread] = np.nan  # the dofs no cell references are not read
    ui = cells.interpolant()
    exact = pr.solution(cells.xe) * (1.0 + 0.1 * rng.standard_normal(cells.xe.shape[:2]))
    l2, per_cell = cells.l2_error(ui, exact)
    return dict(mesh=mesh, ub=ub, f=f, u=u, ui=ui, exact=exact, weight=weight, rhs=cells.rhs(f, ub), vals=vals, grads=grads,
                l2=l2, per_cell=per_cell, eta=eta, eta_w=eta_w)


def integrator_scenario(run, kind, dim, p):
    R = _integrator_reference(kind, dim, p)
    mesh = R["mesh"]
    N, nc, npts = mesh.n_dofs, mesh.n_cells, mesh.n_cells * mesh.nd
    it = run.own(integrator(mesh))  # (MFGPU_UPDATABLE_COEFFICIENTS: the gradients need it)
    f, ub, u, ui, exact, weight = (dev(np.asarray(R[k]).reshape(-1)) for k in ("f", "ub", "u", "ui", "exact", "weight"))

    def out(n):
        v = mf.DeviceVector(n)
        v.fill(np.nan)  # every entry is written
        return v

    def rhs():
        dst = out(N)
        it.rhs(dst, f, ub)
        mf.synchronize()
        return dst.to_host()

    def l2_error():
        per = out(nc)
        l2 = it.l2_error(ui, exact, per)
        return np.concatenate([[l2], per.to_host()])

    def evaluate(which):
        def go():
            v, g = out(npts), out(npts * dim)
            it.evaluate(u, v, g)
            mf.synchronize()
            return (v, g)[which].to_host()
        return go

    def indicator(w):
        def go():
            per = out(nc)
            it.recovery_indicator(u, per, w)
            mf.synchronize()
            return per.to_host()
        return go

    run.twice("rhs", rhs, R["rhs"], 1e-12, err=max_rel, exact=True)
    run.twice("l2_error", l2_error, np.concatenate([[R["l2"]], R["per_cell"]]), 1e-12, err=_l2_err, exact=True)
    run.twice("evaluate_values", evaluate(0), R["vals"], 1e-12, err=max_rel, exact=True)
    run.twice("evaluate_gradients", evaluate(1), R["grads"], 1e-12, err=max_rel, exact=True)
    run.twice("recovery_indicator", indicator(None), R["eta"], 1e-12, err=max_rel, exact=True)
    run.twice("recovery_indicator_weighted", indicator(weight), R["eta_w"], 1e-12, err=max_rel, exact=True)


def _l2_err(got, want):
    """the norm relative to itself, the per-cell squares relative to the largest (tests/test_gpu_redzone_solvers.py)"""
    return max(abs(got[0] - want[0]) / want[0], max_rel(got[1:], want[1:]))


@pytest.mark.parametrize("dim,p", [(2, 2), (3, 4)])
@pytest.mark.parametrize("kind", ["cube", "hanging", "ball"])
def test_integrator(kind, dim, p):
    guarded(integrator_scenario, kind, dim, p)


# ---- Points: 1, 65 and 513 points in ONE cell with a hanging-node mask (513: two work items, the second with one point)


@functools.lru_cache(maxsize=None)
def _points_reference(n_points):
    mesh = mf.Mesh.from_leaves(3, 4, one_refined(3))
    cells = pr.Cells(mesh)
    masked = np.flatnonzero(mesh.arrays()["constraint_mask"])
    assert len(masked)
    rng = np.random.default_rng(n_points)
    cell = np.full(n_points, masked[0], dtype=np.uint32)
    xi = rng.random((n_points, 3))
    unread = ptr.unread_dofs(mesh)
    u = rng.standard_normal(mesh.n_dofs)
    ref = ptr.PointsRef(cells, cell, xi)
    w = rng.standard_normal(n_points)
    vals, grads = ref.evaluate(np.where(unread, 0.0, u))
    u[unread] = np.nan
    return mesh, cell, xi, u, w, vals, grads, ref.integrate(w), ref.integrate()


def points_scenario(run, n_points):
    mesh, cell, xi, u, w, vals, grads, rhs_w, rhs_1 = _points_reference(n_points)
    it = integrator(mesh)
    pts = mf.Points.in_cells(it, cell, xi)
    run.own(it, pts)
    assert pts.n_not_found == 0
    du, dw = dev(u), dev(w)

    def out(n):
        v = mf.DeviceVector(n)
        v.fill(np.nan)
        return v

    def evaluate(which):
        def go():
            v, g = out(n_points), out(n_points * 3)
            pts.evaluate(du, v, g)
            mf.synchronize()
            return (v, g)[which].to_host()
        return go

    def integrate(weights):
        def go():
            r = out(mesh.n_dofs)
            pts.integrate(r, weights)
            mf.synchronize()
            return r.to_host()
        return go

    run.twice("evaluate_values", evaluate(0), vals, 1e-12, err=max_rel, exact=True)
    run.twice("evaluate_gradients", evaluate(1), grads, 1e-12, err=max_rel, exact=True)
    run.twice("integrate", integrate(dw), rhs_w, 1e-12, err=max_rel, exact=True)
    run.twice("integrate_unweighted", integrate(None), rhs_1, 1e-12, err=max_rel, exact=True)
    run.note("memory_consumption", pts.memory_consumption())


@pytest.mark.parametrize("n_points", [1, 65, 513])
def test_points(n_points):
    guarded(points_scenario, n_points)


# ---- Locator.locate: 65 points (one full wave and one lane), with and without hints


@functools.lru_cache(maxsize=None)
def _locate_reference(kind):
    mesh = mf.Mesh.from_leaves(3, 2, one_refined(3)) if kind == "hanging" else mf.Mesh.ball(3, 2, 1)
    cells = pr.Cells(mesh)
    rng = np.random.default_rng(65)
    cell = rng.integers(0, mesh.n_cells, 63)
    x = np.concatenate([ptr.mapping(2, cells.qpts[c], rng.random((1, 3)))[0] for c in cell] + [[[2.0] * 3, [np.nan] * 3]])
    assert len(x) == 65
    return mesh, x, mf.locate_points(mesh.desc, x)


def locate_scenario(run, kind):
    mesh, x, (hcell, hxi, hmissing) = _locate_reference(kind)
    assert hmissing == 2
    it = integrator(mesh)
    s = types.SimpleNamespace(loc=mf.Locator(it, mesh.desc), dim=3)
    run.own(it, s.loc)
    hints = np.where(hcell == mf.POINT_NOT_FOUND, 0, hcell).astype(np.uint32)

    def locate(hint, which):
        def go():
            cell, xi, missing = device_locate(s, x, hint=hint)
            assert missing == hmissing and np.all((xi >= 0.0) & (xi <= 1.0))
            return (cell, xi)[which]
        return go

    for tag, hint in (("", None), ("_hinted", hints)):
        run.twice("cell" + tag, locate(hint, 0), hcell, 0.0, err=unequal, exact=True)
        run.twice("xi" + tag, locate(hint, 1), hxi, XI_TOL, err=max_abs, exact=True)
    assert same_bits(run.results["xi"][0], run.results["xi_hinted"][0])  # "the hinted result equals the unhinted one"
    run.note("memory_consumption", s.loc.memory_consumption())


@pytest.mark.parametrize("kind", ["hanging", "ball"])
def test_locator(kind):
    guarded(locate_scenario, kind)


# ---- CG: six iterates against the numpy recurrence, then a solve to convergence


def cg_scenario(run, kind, dt):
    P = problem(3, 2, 4)
    nt = NT[dt]
    mesh = P.mesh[dt]
    op = mf.Operator(mesh.desc, mesh)
    dinv = dev(P.dinv, nt)
    cg = mf.CG(op, KIND[kind], None if kind == "none" else dinv, DEGREE, P.lambda_max, RANGE)
    run.own(op, cg)
    b = P.rhs(0)
    db = dev(b, nt)
    want6 = [h for _, h in zip(range(7), P.reference(kind, np.float64, b, 0.0, 1000))][6]
    assert want6[0] == 6

    def six_iterates():
        x = mf.DeviceVector(P.N, nt)
        x.fill(np.nan)  # begin writes every entry
        cg.begin(x, db, 0.0, 1000)
        cg.iterate(6)
        info = cg.status()
        assert (info.iterations, info.status) == (6, 0)
        return x.to_host()

    run.twice("six_iterates", six_iterates, want6[3], ITERATE_TOL[dt])
    tol, bound = (1e-10, 2e-10) if dt == np.float64 else (1e-4, 2e-4)
    b1 = P.rhs(1)
    tolerance = tol * np.linalg.norm(b1)
    ref_it, ref_status, ref_res, _ = list(P.reference(kind, dt, b1, tolerance, 10000))[-1]
    assert ref_status == 1 and ref_res <= tolerance
    db1 = dev(b1, nt)

    def solve():
        x = mf.DeviceVector(P.N, nt)
        x.fill(np.nan)
        info = cg.solve(x, db1, tolerance, 10000, check_every=5)
        got = x.to_host()
        assert info.status == 1 and abs(int(info.iterations) - ref_it) <= 1 and info.residual <= tolerance
        run.note("iterations", int(info.iterations))
        return np.concatenate([[float(info.iterations)], got.astype(np.float64)])

    def true_residual(got, want):
        """the solve's own bound (tests/test_gpu_cg.py): |b - A x| / |b|; `want` is not used, b and A are the reference"""
        return float(np.linalg.norm(b1 - P.A @ got[1:]) / np.linalg.norm(b1))

    run.twice("solve", solve, None, bound, err=true_residual)
    run.note("memory_consumption", cg.memory_consumption())


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["none", "jacobi", "chebyshev"])
def test_cg(kind, dt):
    guarded(cg_scenario, kind, dt)


# ---- VCycle.apply: local smoothing, p-levels, global coarsening; double and float levels


def _apply_twice(run, V, R, want, nt):
    def go():
        return apply_all(V, R)  # (z starts as NaN, the result is asserted finite)
    run.twice("apply", go, want, VCYCLE_TOL[nt], err=lambda got, ref: max(rel(got[:, k], ref[:, k]) for k in range(R.shape[1])))
    run.note("memory_consumption", V.memory_consumption())


def vcycle_scenario(run, kind, nt):
    if kind == "local_smoothing":  # adaptive_mg(3, 2, 4): refinement edges
        ref, R, want = vcycle_reference("adaptive_3d_p2_r4")
        V = run.own(make_vcycle("adaptive_3d_p2_r4", nt, F64, lambda_max=ref.lmax, coarse=mf.VCYCLE_COARSE_DENSE))
        assert V.n_levels == ref.n_levels and any(len(E) for E in ref.edge)
    elif kind == "p_levels":  # h-levels at degree 1, then degree 1 -> 2 -> 4 (tests/test_gpu_pmg.py)
        V = run.own(mf.VCycle.from_level_meshes(hybrid_meshes("3d", nt), F64))  # estimated lambda_max
        R = hybrid_defects("3d")
        want = pmr.with_lambda_max(pmg_model("3d"), V.lambda_max()).vcycle(R)
    else:  # adaptive(3, 2, 4) coarsened globally, hanging nodes on the levels (tests/test_gpu_redzone_solvers.py)
        model, R = _gc_reference(4)
        V = run.own(mf.VCycle.from_global_coarsening(mf.Mesh.adaptive(3, 2, 4, number_type=nt), (1, 2), F64))
        want = pmr.with_lambda_max(model, V.lambda_max()).vcycle(R)
    _apply_twice(run, V, R, want, nt)


@pytest.mark.parametrize("nt", [F64, F32], ids=["double_levels", "float_levels"])
@pytest.mark.parametrize("kind", ["local_smoothing", "p_levels", "global_coarsening"])
def test_vcycle_apply(kind, nt):
    guarded(vcycle_scenario, kind, nt)


def refresh_scenario(run, nt):
    """tests/test_gpu_refresh.py::test_refreshed_is_fresh on adaptive_mg(3, 2, 3): new coefficients on every level, the
    refreshed object against a fresh one"""
    mesh = mf.Mesh.adaptive_mg(3, 2, 3, number_type=nt)
    levels, keep = mf.VCycle.hierarchy_levels(mesh, flags=mf.UPDATABLE_COEFFICIENTS)
    meshes, N = keep[2], mesh.n_dofs
    V = run.own(mf.VCycle(levels, F64, N, coarse=mf.VCYCLE_COARSE_DENSE, keep=keep))
    R = defects(mesh, 7)
    for lev, M in zip(levels, meshes):
        lev["op"].update_coefficients(dev(field(1)(M.arrays()["quadrature_points"].astype(np.float64)).reshape(-1), nt), None)
    mf.synchronize()
    stale = apply_all(V, R)

    def refresh_and_apply():
        V.refresh(eig_steps=200)
        info = V.refresh_status()
        assert info.coarse_status == 0 and info.eig_status_max == 1 and 15 <= info.eig_steps_max <= 200
        return apply_all(V, R)

    W = run.own(mf.VCycle(levels, F64, N, coarse=mf.VCYCLE_COARSE_DENSE, keep=keep))
    want = apply_all(W, R)
    cols = lambda got, ref: max(rel(got[:, j], ref[:, j]) for j in range(3))  # noqa: E731
    assert cols(stale, want) > 100 * REFRESH_TOL[nt]  # otherwise the coefficient change proves nothing
    run.twice("refresh_then_apply", refresh_and_apply, want, REFRESH_TOL[nt], err=cols)
    del levels, keep


@pytest.mark.parametrize("nt", [F64, F32], ids=["double_levels", "float_levels"])
def test_vcycle_refresh_after_a_coefficient_update(nt):
    guarded(refresh_scenario, nt)


# ---- the slab exchange, in process: three chained distributed applies


@functools.lru_cache(maxsize=None)
def _slab_reference(p, n, world):
    from pymfgpu.parallel import slab_ranges
    full = mf.Mesh.uniform(3, p, n)
    od = oracle_desc_from_mesh(full, dtype=np.float64)
    fx = full.dof_coords()
    key = {tuple(np.round(c, 9)): i for i, c in enumerate(fx)}
    ranges = list(slab_ranges(n, world))
    gi = []
    for r in ranges:
        slab = mf.Mesh.uniform(3, p, n, slab=r)
        gi.append(np.array([key[tuple(np.round(c, 9))] for c in slab.dof_coords()]))
    x = typed(np.sin(3 * fx[:, 0]) + fx[:, 1] ** 2 - np.cos(2 * fx[:, 2]) * fx[:, 0], F32)
    refs = [x]
    for _ in range(3):
        refs.append(o.vmult(od, refs[-1]))
    return ranges, gi, refs


def slab_scenario(run, p, n, world, nt):
    ranges, gis, refs = _slab_reference(p, n, world)
    slabs = []
    for r, (rng_z, gi) in enumerate(zip(ranges, gis)):
        mesh = mf.Mesh.uniform(3, p, n, slab=rng_z, number_type=nt)
        op, dist = mf.Operator(mesh.desc, mesh), mf.Dist(mesh, r, world)
        dist.attach(op)
        run.own(op, dist)
        slabs.append(dict(op=op, dist=dist, gi=gi, n=mesh.n_dofs))
    for lo, up in zip(slabs, slabs[1:]):
        lo["dist"].connect_local(up["dist"])
    run.note("schedule", [s["dist"].schedule() for s in slabs])

    def chained():
        for s in slabs:
            s["a"], s["b"] = dev(refs[0][s["gi"]], nt), mf.DeviceVector(s["n"], nt)
            s["b"].fill(np.nan)
        out = []
        for it in range(3):
            for s in slabs:
                s["dist"].vmult_begin(s["op"], s["b"], s["a"])
            for s in slabs:
                s["dist"].vmult_end(s["op"], s["b"])
            mf.synchronize()
            out.append(np.concatenate([s["b"].to_host() for s in slabs]))
            for s in slabs:
                s["a"], s["b"] = s["b"], s["a"]
        return np.stack(out)

    def chained_err(got, want):
        """per apply, relative to the bound of test_gpu.py::test_cxx_slab_exchange_in_process: TOL * 100^it"""
        return max(rel(got[it], want[it]) / 100 ** it for it in range(3))

    want = np.stack([np.concatenate([refs[it + 1][s["gi"]] for s in slabs]) for it in range(3)])
    run.twice("three_chained_applies", chained, want, TOL[nt], err=chained_err)
    for s in slabs:
        s.pop("a"), s.pop("b")


@TYPES
@pytest.mark.parametrize("p,n,world", [(4, 6, 2), (2, 8, 4)])
def test_slab_exchange(p, n, world, nt):
    guarded(slab_scenario, p, n, world, nt)
