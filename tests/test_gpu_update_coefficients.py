"""mfgpu_update_coefficients (MFGPU_UPDATABLE_COEFFICIENTS): an operator whose coefficients were replaced from device
arrays is the operator created from those values -- vmult, vmult_add and the inverse diagonal of the updated handle H1
against a fresh handle H2 and against the oracle (oracle.mf_oracle / tests/helmholtz_reference.py), through every
cell-loop kernel family; the level operator with its interface matrices and the integrator's lift likewise.

Cases are the smallest at which the plan's cell order is not the identity, batches hold several cells and the last
batch is partial.  Tolerances are the project's parity tolerances, relative l2 <= 1e-12 in double and 1e-5 in float.
H1 against H2 is bit for bit wherever two vmults of one handle are (test_gpu_helmholtz.py REPEAT): the plane kernels,
every MASS instantiation, one-cell batches.  The inverse diagonal adds its cell contributions with atomics, so H1 and
H2 are held to the tolerance there."""
import copy

import numpy as np
import pytest

import helmholtz_reference as hr
import poisson_reference as pr
import pymfgpu as mf
from oracle import mf_oracle as o
from test_gpu import TOL, gpu_vmult, rel
from test_gpu_level import _edge_of_box
from util import deform, deformed_oracle_desc, desc_from_oracle, oracle_desc_from_mesh

pytestmark = pytest.mark.gpu


def positive(od, nt, seed):
    """seeded random values in [0.5, 1.5] per quadrature point, rounded to the number type"""
    c = np.random.default_rng(seed).uniform(0.5, 1.5, (od.n_cells, od.nd))
    return c.astype(mf.np_dtype(nt)).astype(np.float64)


def with_coefficient(od, coef):
    od = copy.copy(od)
    od.coefficient = np.ascontiguousarray(coef, dtype=np.float64).reshape(od.n_cells, od.nd)
    return od


def make_op(od, nt, coef, mass, updatable, **knobs):
    desc, keep = desc_from_oracle(with_coefficient(od, coef), number_type=nt, mass_coefficient=mass, **knobs)
    if updatable:
        desc.flags |= mf.UPDATABLE_COEFFICIENTS
    return mf.Operator(desc, keep)


def dvec(a, nt=mf.F64):
    v = mf.DeviceVector(np.asarray(a).size, nt)
    v.from_host(np.asarray(a).reshape(-1))
    return v


def update(obj, coef, mass, nt=mf.F64):
    dc, dm = (None if a is None else dvec(a, nt) for a in (coef, mass))
    obj.update_coefficients(dc, dm)
    mf.synchronize()  # (the device arrays are read when the stream gets there: keep them until then)


def inv_diag(op, n, nt):
    d = mf.DeviceVector(n, nt)
    op.compute_inverse_diagonal(d)
    mf.synchronize()
    return d.to_host().astype(np.float64)


def reproducible(op, mass):
    """the configurations in which two vmults of one handle give the same bits"""
    return mass or op.kernel_name() in ("apply_planes3", "apply_planes4") or op.plan_stats()["max_batch_cells"] == 1


def mesh_od(mesh):
    """oracle description of a stand-in mesh; its arrays are views into the mesh, which it keeps alive"""
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    od.mesh = mesh
    return od


def _mesh_od(make):
    return lambda nt: mesh_od(make(nt))


CASES = [
    ("cube_p4_n5", _mesh_od(lambda nt: mf.Mesh.uniform(3, 4, 5, number_type=nt)), dict(), [mf.F64, mf.F32]),
    ("cube_p4_n6_shared", _mesh_od(lambda nt: mf.Mesh.uniform(3, 4, 6, number_type=nt)), dict(), [mf.F64]),
    ("cube_p3_n6_2w", _mesh_od(lambda nt: mf.Mesh.uniform(3, 3, 6, number_type=nt)), dict(kernel=mf.KERNEL_PLANES_2W), [mf.F64]),
    ("cube_p2_n9", _mesh_od(lambda nt: mf.Mesh.uniform(3, 2, 9, number_type=nt)), dict(), [mf.F64]),
    ("cube_p5_n4", _mesh_od(lambda nt: mf.Mesh.uniform(3, 5, 4, number_type=nt)), dict(), [mf.F64]),
    ("cube_p6_n2", _mesh_od(lambda nt: mf.Mesh.uniform(3, 6, 2, number_type=nt)), dict(), [mf.F64]),
    ("pencils_x_p4_n6", _mesh_od(lambda nt: mf.Mesh.uniform(3, 4, 6, number_type=nt)),
     dict(kernel=mf.KERNEL_PENCILS_X, max_cells_per_batch=27), [mf.F64]),
    ("cube_2d_p3_n8", _mesh_od(lambda nt: mf.Mesh.uniform(2, 3, 8, number_type=nt)), dict(), [mf.F64]),
    ("cube_2d_p2_n9_colored", _mesh_od(lambda nt: mf.Mesh.uniform(2, 2, 9, number_type=nt)), dict(colored=True), [mf.F64]),
    ("adaptive_p4", _mesh_od(lambda nt: mf.Mesh.adaptive(3, 4, 4, number_type=nt)), dict(), [mf.F64, mf.F32]),
    ("adaptive_p2", _mesh_od(lambda nt: mf.Mesh.adaptive(3, 2, 4, number_type=nt)), dict(), [mf.F64]),
    ("deformed_3d_p2_n3", lambda nt: deformed_oracle_desc(2, 3, seed=3), dict(), [mf.F64]),
    ("deformed_2d_p3_n7", lambda nt: deform(o.uniform_mesh_desc(2, 3, 7), eps=0.15, seed=7), dict(max_cells_per_batch=9), [mf.F64]),
    ("deformed_3d_p2_n4_cells16", lambda nt: deformed_oracle_desc(2, 4, seed=4), dict(max_cells_per_batch=16), [mf.F64]),
    ("cube_2d_p3_n8_cells9", _mesh_od(lambda nt: mf.Mesh.uniform(2, 3, 8, number_type=nt)), dict(max_cells_per_batch=9), [mf.F64]),
    ("ball_3d_p2", _mesh_od(lambda nt: mf.Mesh.ball(3, 2, 1, number_type=nt)), dict(), [mf.F64, mf.F32]),
    ("ball_2d_p2", _mesh_od(lambda nt: mf.Mesh.ball(2, 2, 2, number_type=nt)), dict(), [mf.F64]),
]
PARAMS = [pytest.param(make, knobs, nt, mass, id=f"{name}-{'f64' if nt == mf.F64 else 'f32'}-{'mass' if mass else 'laplace'}")
          for name, make, knobs, nts in CASES for nt in nts for mass in (False, True)]


@pytest.mark.parametrize("make,knobs,nt,mass", PARAMS)
def test_updated_operator_is_the_fresh_operator(make, knobs, nt, mass):
    od = make(nt)
    c0, c1 = positive(od, nt, 1), positive(od, nt, 2)
    m0, m1 = (positive(od, nt, 3), positive(od, nt, 4)) if mass else (None, None)
    h1 = make_op(od, nt, c0, m0, True, **knobs)
    update(h1, c1, m1, nt)
    h2 = make_op(od, nt, c1, m1, False, **knobs)
    assert h1.kernel_name() == h2.kernel_name() and h1.plan_stats() == h2.plan_stats()
    st = h1.plan_stats()
    print(h1.kernel_name(), st["n_batches"], st["max_batch_cells"], st["index_records"])
    rng = np.random.default_rng(11)
    x, y0 = (rng.standard_normal(od.n_dofs).astype(mf.np_dtype(nt)).astype(np.float64) for _ in range(2))
    od1 = with_coefficient(od, c1)
    ref = (hr.vmult(od1, m1, x), hr.vmult_add(od1, m1, y0, x), hr.inverse_diagonal(od1, m1)) if mass else \
          (o.vmult(od1, x), o.vmult_add(od1, y0, x), o.compute_inverse_diagonal(od1))
    got = [(gpu_vmult(h, x, nt), gpu_vmult(h, x, nt, y0=y0), inv_diag(h, od.n_dofs, nt)) for h in (h1, h2)]
    for k, what in enumerate(("vmult", "vmult_add", "inverse diagonal")):
        e1, e2, e12 = rel(got[0][k], ref[k]), rel(got[1][k], ref[k]), rel(got[0][k], got[1][k])
        print(f"{what}: updated vs oracle {e1:.3e}, fresh vs oracle {e2:.3e}, updated vs fresh {e12:.3e}")
        assert e1 <= TOL[nt] and e2 <= TOL[nt] and e12 <= TOL[nt], (what, e1, e2, e12)
    if reproducible(h1, mass):
        np.testing.assert_array_equal(got[0][0], got[1][0])
        np.testing.assert_array_equal(got[0][1], got[1][1])


BITWISE = [("cube_p4_n5", lambda: mesh_od(mf.Mesh.uniform(3, 4, 5)), dict()),
           ("cube_p2_n9", lambda: mesh_od(mf.Mesh.uniform(3, 2, 9)), dict()),
           ("adaptive_p4", lambda: mesh_od(mf.Mesh.adaptive(3, 4, 4)), dict()),
           ("ball_3d_p2", lambda: mesh_od(mf.Mesh.ball(3, 2, 1)), dict())]


@pytest.mark.parametrize("name,make,knobs", BITWISE, ids=[b[0] for b in BITWISE])
def test_one_term_updates_and_repeated_updates(name, make, knobs):
    """with a mass term every family is bit-reproducible: the comparisons against fresh handles are exact"""
    od = make()
    c0, c1, m0, m1 = (positive(od, mf.F64, s) for s in (1, 2, 3, 4))
    x = np.random.default_rng(5).standard_normal(od.n_dofs)

    def fresh(c, m):
        return gpu_vmult(make_op(od, mf.F64, c, m, False, **knobs), x)

    h = make_op(od, mf.F64, c0, m0, True, **knobs)
    np.testing.assert_array_equal(gpu_vmult(h, x), fresh(c0, m0))  # the flag alone changes no output bit
    update(h, c1, None)  # only the coefficient: the mass term is unchanged
    np.testing.assert_array_equal(gpu_vmult(h, x), fresh(c1, m0))
    update(h, None, m1)  # only the mass
    np.testing.assert_array_equal(gpu_vmult(h, x), fresh(c1, m1))
    update(h, c0, m0)    # two updates in a row equal the last one
    update(h, c1, m0)
    np.testing.assert_array_equal(gpu_vmult(h, x), fresh(c1, m0))
    assert rel(inv_diag(h, od.n_dofs, mf.F64), hr.inverse_diagonal(with_coefficient(od, c1), m0)) <= 1e-12


@pytest.mark.parametrize("name,make,knobs", BITWISE[:1] + BITWISE[3:], ids=["cube_p4_n5", "ball_3d_p2"])
def test_flag_alone_changes_no_output_bit_without_mass(name, make, knobs):
    od = make()
    c0 = positive(od, mf.F64, 1)
    x = np.random.default_rng(5).standard_normal(od.n_dofs)
    plain, flagged = (make_op(od, mf.F64, c0, None, f, **knobs) for f in (False, True))
    assert plain.kernel_name() == flagged.kernel_name() and plain.plan_stats() == flagged.plan_stats()
    assert reproducible(plain, False)
    np.testing.assert_array_equal(gpu_vmult(plain, x), gpu_vmult(flagged, x))


@pytest.mark.parametrize("name,make,nt,plane", [
    ("cube_p4_n5", lambda nt: mesh_od(mf.Mesh.uniform(3, 4, 5, number_type=nt)), mf.F64, True),
    ("adaptive_p4", lambda nt: mesh_od(mf.Mesh.adaptive(3, 4, 4, number_type=nt)), mf.F64, True),
    ("deformed_3d_p2_n3", lambda nt: deformed_oracle_desc(2, 3, seed=3), mf.F64, False),
    ("ball_3d_p2_f32", lambda nt: mesh_od(mf.Mesh.ball(3, 2, 1, number_type=nt)), mf.F32, False),
    ("cube_2d_p3_n8", lambda nt: mesh_od(mf.Mesh.uniform(2, 3, 8, number_type=nt)), mf.F64, False),
], ids=["cube_p4_n5", "adaptive_p4", "deformed_3d_p2_n3", "ball_3d_p2_f32", "cube_2d_p3_n8"])
def test_memory_grows_by_the_kept_arrays(name, make, nt, plane):
    """JxW + inv_jac in the number type, the cell order, and on plane plans the two relayout tables (include/mfgpu.h):
    80 B per quadrature point with the full J^-1 in 3D in double"""
    od = make(nt)
    c0, m0 = positive(od, nt, 1), positive(od, nt, 3)
    es, nc, npts = (8 if nt == mf.F64 else 4), od.n_cells, od.n_cells * od.nd
    for mass in (None, m0):
        plain, flagged = (make_op(od, nt, c0, mass, f) for f in (False, True))
        assert (plain.kernel_name() == "apply_planes3") == plane  # (every cell in a plane batch, or none)
        jinv = nc if od.uniform_j0 else npts * od.dim * od.dim
        want = (npts + jinv) * es + 4 * nc + (8 * nc if plane else 0)
        assert flagged.memory_consumption() - plain.memory_consumption() == want
        if not od.uniform_j0 and od.dim == 3 and nt == mf.F64:
            assert want == 80 * npts + 4 * nc


def test_refused_updates_leave_the_operator_as_it_was():
    od = mesh_od(mf.Mesh.uniform(3, 4, 5))
    c0, c1, m1 = (positive(od, mf.F64, s) for s in (1, 2, 4))
    x = np.random.default_rng(5).standard_normal(od.n_dofs)
    dc, dm = dvec(c1), dvec(m1)
    plain = make_op(od, mf.F64, c0, None, False)
    y = gpu_vmult(plain, x)
    with pytest.raises(mf.MfgpuError, match="error -1.*MFGPU_UPDATABLE_COEFFICIENTS"):
        plain.update_coefficients(dc)
    np.testing.assert_array_equal(gpu_vmult(plain, x), y)
    flagged = make_op(od, mf.F64, c0, None, True)
    with pytest.raises(mf.MfgpuError, match="error -1.*both NULL"):
        flagged.update_coefficients()
    with pytest.raises(mf.MfgpuError, match="error -1.*without a mass term"):
        flagged.update_coefficients(dc, dm)  # (nothing is written: the coefficient stays too)
    with pytest.raises(mf.MfgpuError, match="error -1.*without a mass term"):
        flagged.update_coefficients(None, dm)
    np.testing.assert_array_equal(gpu_vmult(flagged, x), y)
    flagged.update_coefficients(dc)  # ... and usable
    mf.synchronize()
    assert rel(gpu_vmult(flagged, x), o.vmult(with_coefficient(od, c1), x)) <= 1e-12


@pytest.mark.parametrize("mass", [False, True], ids=["laplace", "mass"])
@pytest.mark.parametrize("touch_boundary", [False, True])
def test_level_update(mass, touch_boundary):
    dim, p, n = 3, 2, 4
    mesh = mf.Mesh.uniform(dim, p, n)
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    h = 2.0 / n
    edge = _edge_of_box(mesh, -1.0 + (0.0 if touch_boundary else h), -1.0 + h * (n // 2 + 1))
    assert 0 < len(edge) < mesh.n_dofs
    c0, c1 = positive(od, mf.F64, 1), positive(od, mf.F64, 2)
    m0, m1 = (positive(od, mf.F64, 3), positive(od, mf.F64, 4)) if mass else (None, None)
    desc, keep = desc_from_oracle(with_coefficient(od, c0), mass_coefficient=m0)
    desc.flags |= mf.UPDATABLE_COEFFICIENTS
    lev = mf.Level(desc, edge, keep)
    update(lev, c1, m1)
    od1 = with_coefficient(od, c1)
    odc = o.Desc(dim, p, od.n_dofs, od.loc2glob, od.JxW, od.inv_jac, c1,
                 np.union1d(od.constrained, edge).astype(np.uint32), None, np.float64, od.shape_values, od.shape_gradients)
    x = np.random.default_rng(13).standard_normal(mesh.n_dofs)
    a, b = dvec(x), mf.DeviceVector(mesh.n_dofs)
    want = [hr.vmult(odc, m1, x), hr.vmult_interface_down(od1, m1, edge, x), hr.vmult_interface_up(od1, m1, edge, x)] if mass \
        else [o.vmult(odc, x), o.vmult_interface_down(od1, edge, x), o.vmult_interface_up(od1, edge, x)]
    for fn, ref in zip((lev.vmult, lev.vmult_interface_down, lev.vmult_interface_up), want):
        b.fill(5.0)
        fn(b, a)
        mf.synchronize()
        assert np.linalg.norm(b.to_host() - ref) <= 1e-12 * np.linalg.norm(ref)
    d = mf.DeviceVector(mesh.n_dofs)
    lev.compute_inverse_diagonal(d)
    mf.synchronize()
    assert rel(d.to_host(), hr.inverse_diagonal(odc, m1) if mass else o.compute_inverse_diagonal(odc)) <= 1e-12
    # a level without the flag refuses
    plain = mf.Level(desc_from_oracle(with_coefficient(od, c0), mass_coefficient=m0)[0], edge, keep)
    with pytest.raises(mf.MfgpuError, match="error -1.*MFGPU_UPDATABLE_COEFFICIENTS"):
        plain.update_coefficients(dvec(c1))


@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 2), ("hanging", 3, 2), ("ball", 3, 2)])
@pytest.mark.parametrize("mass", [False, True], ids=["laplace", "mass"])
def test_integrator_lift_after_update(kind, dim, p, mass):
    from test_gpu_poisson import close, small_mesh
    mesh = small_mesh(kind, dim, p)
    cells = pr.Cells(mesh)
    od = cells.od
    c0, c1 = positive(od, mf.F64, 1), positive(od, mf.F64, 2)
    m0, m1 = (positive(od, mf.F64, 3), positive(od, mf.F64, 4)) if mass else (None, None)
    mesh.desc.coefficient = c0.ctypes.data
    mesh.set_mass_coefficient(m0)
    mesh.desc.flags |= mf.UPDATABLE_COEFFICIENTS
    it = mf.Integrator(mesh.desc, mesh)
    update(it, c1, m1)
    ub = np.random.default_rng(7).standard_normal(mesh.n_dofs)
    f = np.random.default_rng(8).standard_normal((od.n_cells, od.nd))
    dst = mf.DeviceVector(mesh.n_dofs)
    dst.fill(np.nan)
    it.rhs(dst, dvec(f), dvec(ub))
    c1cells = copy.copy(cells)
    c1cells.od = with_coefficient(od, c1)
    close(dst.to_host(), hr.rhs(c1cells, m1, f, ub) if mass else c1cells.rhs(f, ub), 1e-12)
    # refusals: nothing to update, a mass term the integrator does not have, no flag
    with pytest.raises(mf.MfgpuError, match="error -1.*both NULL"):
        it.update_coefficients()
    if not mass:
        with pytest.raises(mf.MfgpuError, match="error -1.*without a mass term"):
            it.update_coefficients(None, dvec(c1))
    mesh.desc.flags &= ~mf.UPDATABLE_COEFFICIENTS
    with pytest.raises(mf.MfgpuError, match="error -1.*MFGPU_UPDATABLE_COEFFICIENTS"):
        mf.Integrator(mesh.desc, mesh).update_coefficients(dvec(c1))
