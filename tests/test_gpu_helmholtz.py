"""The mass term on the GPU (mfgpu_desc.mass_coefficient: A = sum_cells P^T C^T (K_cell + M_cell) C P) against the numpy
restatement in tests/helmholtz_reference.py: vmult / vmult_add through every cell-loop kernel family, the inverse
diagonal, the integrator's lift, the level operator with its interface matrices, two slabs on one GPU, and a
reaction-diffusion solve whose L2 error falls at order p + 1.

Unless a test says otherwise c is a seeded random value in [0.5, 1.5] per quadrature point, so that a wrong layout of the
folded mass weights cannot pass.  Tolerances are the project's: relative l2 <= 1e-12 in double, 1e-5 in float."""
import os
import subprocess

import numpy as np
import pytest

import helmholtz_reference as hr
import poisson_reference as pr
import pymfgpu as mf
from oracle import mf_oracle as o
from test_gpu import CASES, KERNELS, TOL, gpu_vmult, rel
from test_gpu_aux import TOL as DIAG_TOL
from test_gpu_poisson import close, dv
from util import deform, deformed_oracle_desc, desc_from_oracle, oracle_desc_from_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Orders of the numpy reference (helmholtz_reference.solve) on the ball, p = 2, n_ref 1..3, measured on the CPU:
#   2D: L2 errors 0.12815, 0.014600, 0.0019886, orders 3.13, 2.88
#   3D: L2 errors 0.099717, 0.013946, 0.0020138, orders 2.84, 2.79
HELMHOLTZ_BALL_ORDER_2D_P2 = 2.88
HELMHOLTZ_BALL_ORDER_3D_P2 = 2.79


def random_c(n_cells, nd, nt=mf.F64, seed=0):
    """c in [0.5, 1.5], rounded to the number type (the reference computes in double on the rounded values)"""
    c = np.random.default_rng(seed).uniform(0.5, 1.5, (n_cells, nd))
    return c.astype(mf.np_dtype(nt)).astype(np.float64)


def mass_mesh(mesh, nt=mf.F64, seed=0):
    """(oracle description, c) of a stand-in mesh whose description now carries c"""
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    c = random_c(od.n_cells, od.nd, nt, seed)
    mesh.set_mass_coefficient(c)
    return od, c


def check_vmult_and_add(op, od, c, nt=mf.F64, seed=17, tol=None):
    tol = TOL[nt] if tol is None else tol
    rng = np.random.default_rng(seed)
    x, y0 = (rng.standard_normal(od.n_dofs).astype(mf.np_dtype(nt)).astype(np.float64) for _ in range(2))
    y = gpu_vmult(op, x, nt)  # (checks that src is untouched)
    ey = rel(y, hr.vmult(od, c, x))
    ez = rel(gpu_vmult(op, x, nt, y0=y0), hr.vmult_add(od, c, y0, x))
    print(f"vmult {ey:.3e} vmult_add {ez:.3e}")
    assert ey <= tol and ez <= tol, (ey, ez)
    np.testing.assert_array_equal(gpu_vmult(op, x, nt), y)  # two calls on the same inputs: bitwise equal
    return x, y


# ---- 1. vmult / vmult_add


@pytest.mark.parametrize("dim,p,n", CASES)
@pytest.mark.parametrize("nt", [mf.F64, mf.F32])
@pytest.mark.parametrize("colored", [False, True])
def test_vmult_matches_reference(dim, p, n, nt, colored):
    mesh = mf.Mesh.uniform(dim, p, n, number_type=nt)
    od, c = mass_mesh(mesh, nt, seed=dim * 100 + p * 10 + n)
    if colored:
        mesh.desc.flags |= mf.COLORED_SCATTER
    op = mf.Operator(mesh.desc, mesh)
    if dim == 3 and p == 4 and not colored:
        assert op.kernel_name() == "apply_planes3"  # p = 4 stays in the plane kernel
    if dim == 3 and p >= 5 and not colored:
        assert op.kernel_name() == "apply_batches_x"  # no mass instantiation of apply_planes4w
    check_vmult_and_add(op, od, c, nt)


@pytest.mark.parametrize("kern,name", KERNELS, ids=[k[1] for k in KERNELS])
@pytest.mark.parametrize("p,n", [(4, 7), (2, 9), (3, 6)])
@pytest.mark.parametrize("nt", [mf.F64, mf.F32])
def test_kernel_families_match_reference(kern, name, p, n, nt):
    mesh = mf.Mesh.uniform(3, p, n, number_type=nt)
    od, c = mass_mesh(mesh, nt, seed=p)
    mesh.desc.kernel = kern
    if kern == mf.KERNEL_PLANES_2W and p == 4 and nt == mf.F64:  # apply_planes4<5, double> would spill with the term
        with pytest.raises(mf.MfgpuError, match="error -4.*mass"):
            mf.Operator(mesh.desc, mesh)
        return
    op = mf.Operator(mesh.desc, mesh)
    assert op.kernel_name() == name
    check_vmult_and_add(op, od, c, nt)


@pytest.mark.parametrize("p", [5, 6])
@pytest.mark.parametrize("kern", [mf.KERNEL_PLANES, mf.KERNEL_PLANES_2W])
def test_forced_family_without_mass_instantiation_is_refused(p, kern):
    mesh = mf.Mesh.uniform(3, p, 3)
    mesh.desc.kernel = kern
    assert mf.Operator(mesh.desc, mesh).kernel_name() == "apply_planes4"  # (without a mass term: served)
    mass_mesh(mesh)
    with pytest.raises(mf.MfgpuError, match="error -4.*mass"):
        mf.Operator(mesh.desc, mesh)
    mesh.desc.kernel = mf.KERNEL_PENCILS_X
    assert mf.Operator(mesh.desc, mesh).kernel_name() == "apply_batches_x"


@pytest.mark.parametrize("p,n,cells", [(1, 12, 256), (2, 10, 256), (3, 8, 256), (4, 6, 27), (5, 4, 256), (6, 3, 256)])
@pytest.mark.parametrize("kern", [mf.KERNEL_PENCILS, mf.KERNEL_PENCILS_X], ids=["apply_batches", "apply_batches_x"])
@pytest.mark.parametrize("nt", [mf.F64, mf.F32])
def test_pencil_kernels_multi_chunk_batches(p, n, cells, kern, nt):
    mesh = mf.Mesh.uniform(3, p, n, number_type=nt)
    od, c = mass_mesh(mesh, nt, seed=p * 31 + n)
    mesh.desc.kernel = kern
    mesh.desc.max_cells_per_batch = cells
    op = mf.Operator(mesh.desc, mesh)
    st = op.plan_stats()
    assert st["n_batches"] >= 2 and st["max_batch_cells"] > 256 // (p + 1) ** 2, st
    check_vmult_and_add(op, od, c, nt)


@pytest.mark.parametrize("p,n,cells", [(2, 9, 0), (4, 9, 0), (3, 12, 40), (6, 5, 9)])
def test_2d_multi_cell_batches(p, n, cells):
    mesh = mf.Mesh.uniform(2, p, n)
    od, c = mass_mesh(mesh, seed=p)
    mesh.desc.max_cells_per_batch = cells
    for colored in (False, True):
        mesh.desc.flags = (mesh.desc.flags & ~mf.COLORED_SCATTER) | (mf.COLORED_SCATTER if colored else 0)
        check_vmult_and_add(mf.Operator(mesh.desc, mesh), od, c)


@pytest.mark.parametrize("dim,p,nref", [(2, 2, 4), (2, 4, 5), (3, 1, 4), (3, 2, 4), (3, 4, 4), (3, 4, 5), (3, 3, 5)])
@pytest.mark.parametrize("colored", [False, True])
def test_adaptive_mesh_with_hanging_nodes(dim, p, nref, colored):
    mesh = mf.Mesh.adaptive(dim, p, nref)
    od, c = mass_mesh(mesh, seed=nref)
    assert od.constraint_mask is not None and od.constraint_mask.any()
    if colored:
        mesh.desc.flags |= mf.COLORED_SCATTER
    op = mf.Operator(mesh.desc, mesh)
    if dim == 3 and p == 4 and not colored:
        assert op.kernel_name() == "apply_planes3"  # masked cells too (apply_planes3<HN>)
    check_vmult_and_add(op, od, c)


@pytest.mark.parametrize("p,nref,kern,nt", [(4, 4, mf.KERNEL_PENCILS_X, mf.F64), (2, 4, mf.KERNEL_PENCILS_X, mf.F64),
                                            (3, 5, mf.KERNEL_PENCILS_X, mf.F64), (4, 4, mf.KERNEL_PLANES_2W, mf.F32),
                                            (3, 4, mf.KERNEL_PLANES_2W, mf.F64),
                                            (3, 5, mf.KERNEL_PLANES, mf.F64), (2, 4, mf.KERNEL_PENCILS, mf.F64),
                                            (5, 4, mf.KERNEL_AUTO, mf.F64), (6, 4, mf.KERNEL_AUTO, mf.F64),
                                            (5, 4, mf.KERNEL_AUTO, mf.F32), (4, 4, mf.KERNEL_AUTO, mf.F32),
                                            (3, 4, mf.KERNEL_AUTO, mf.F32)])
def test_adaptive_mesh_kernel_families(p, nref, kern, nt):
    mesh = mf.Mesh.adaptive(3, p, nref, number_type=nt)
    od, c = mass_mesh(mesh, nt, seed=p)
    mesh.desc.kernel = kern
    op = mf.Operator(mesh.desc, mesh)
    if p == 4 and kern == mf.KERNEL_AUTO:
        assert op.kernel_name() == "apply_planes3"
    check_vmult_and_add(op, od, c, nt)


def _rounded(od, nt):
    """the description a float operator sees, as doubles"""
    if nt == mf.F64:
        return od
    f = np.float32
    return o.Desc(od.dim, od.degree, od.n_dofs, od.loc2glob, od.JxW.astype(f), od.inv_jac.astype(f),
                  od.coefficient.astype(f), od.constrained, od.constraint_mask, np.float64, od.shape_values.astype(f),
                  od.shape_gradients.astype(f), od.weights)


@pytest.mark.parametrize("nt,tol", [(mf.F64, 1e-12), (mf.F32, 1e-5)])
@pytest.mark.parametrize("p,n", [(1, 5), (2, 4), (3, 3), (4, 2), (4, 5), (5, 2), (6, 2), (2, 9)])
def test_general_jacobian_3d(p, n, nt, tol):
    od = deformed_oracle_desc(p, n, seed=p * 10 + n)
    c = random_c(od.n_cells, od.nd, nt, seed=p)
    desc, keep = desc_from_oracle(od, number_type=nt, mass_coefficient=c)
    op = mf.Operator(desc, keep)
    assert op.kernel_name() == "apply_batches_g"
    check_vmult_and_add(op, _rounded(od, nt), c, nt, tol=tol)


@pytest.mark.parametrize("p,n,cells", [(2, 8, 64), (4, 6, 27), (3, 6, 40)])
def test_general_jacobian_3d_multi_cell_batches(p, n, cells):
    od = deformed_oracle_desc(p, n, seed=p)
    c = random_c(od.n_cells, od.nd, seed=n)
    desc, keep = desc_from_oracle(od, max_cells_per_batch=cells, mass_coefficient=c)
    op = mf.Operator(desc, keep)
    st = op.plan_stats()
    assert op.kernel_name() == "apply_batches_g" and st["n_batches"] >= 2 and st["max_batch_cells"] > 256 // (p + 1) ** 2
    check_vmult_and_add(op, od, c)


@pytest.mark.parametrize("nt,tol", [(mf.F64, 1e-12), (mf.F32, 1e-5)])
@pytest.mark.parametrize("p,n,cells", [(1, 9, 0), (2, 8, 0), (2, 32, 0), (3, 7, 9), (4, 6, 0), (4, 12, 30), (5, 5, 4), (6, 4, 0)])
def test_general_jacobian_2d(p, n, cells, nt, tol):
    od = deform(o.uniform_mesh_desc(2, p, n), eps=0.15, seed=p * 10 + n)
    c = random_c(od.n_cells, od.nd, nt, seed=p)
    desc, keep = desc_from_oracle(od, number_type=nt, max_cells_per_batch=cells, mass_coefficient=c)
    op = mf.Operator(desc, keep)
    assert op.kernel_name() == "apply_batches_g2"
    check_vmult_and_add(op, _rounded(od, nt), c, nt, tol=tol)


@pytest.mark.parametrize("dim,p,nref", [(3, 1, 4), (3, 2, 4), (3, 4, 4), (3, 3, 5), (2, 1, 4), (2, 2, 5), (2, 4, 4), (2, 3, 6)])
def test_general_jacobian_with_hanging_nodes(dim, p, nref):
    mesh = mf.Mesh.adaptive(dim, p, nref)
    od = deform(oracle_desc_from_mesh(mesh, dtype=np.float64), seed=nref)
    c = random_c(od.n_cells, od.nd, seed=p)
    desc, keep = desc_from_oracle(od, mass_coefficient=c)
    check_vmult_and_add(mf.Operator(desc, keep), od, c)


@pytest.mark.parametrize("dim,p,n_ref,nt,cells", [(3, 1, 2, mf.F64, 0), (3, 2, 1, mf.F64, 0), (3, 2, 2, mf.F64, 16),
                                                  (3, 3, 1, mf.F64, 8), (3, 4, 1, mf.F64, 0), (3, 2, 1, mf.F32, 0),
                                                  (3, 6, 0, mf.F64, 0), (2, 1, 3, mf.F64, 0), (2, 2, 2, mf.F64, 0),
                                                  (2, 4, 2, mf.F64, 0), (2, 4, 4, mf.F64, 0), (2, 6, 1, mf.F64, 0)])
def test_ball(dim, p, n_ref, nt, cells):
    mesh = mf.Mesh.ball(dim, p, n_ref, number_type=nt)
    od, c = mass_mesh(mesh, nt, seed=p + n_ref)
    mesh.desc.max_cells_per_batch = cells
    check_vmult_and_add(mf.Operator(mesh.desc, mesh), od, c, nt)


@pytest.mark.parametrize("p,n,wgs", [(4, 6, 0), (4, 12, 0), (4, 12, 3), (4, 18, 7), (4, 11, 2), (3, 12, 2), (2, 12, 3)])
@pytest.mark.parametrize("nt", [mf.F64, mf.F32])
def test_shared_records_equal_expanded_bit_for_bit(p, n, wgs, nt):
    """also the small max_workgroups of the issue: few workgroups walk many batches"""
    from test_gpu_shared_records import make_ops
    mesh = mf.Mesh.uniform(3, p, n, number_type=nt)
    od, c = mass_mesh(mesh, nt, seed=n)
    op, op_x = make_ops(mesh, max_workgroups=wgs, kernel=mf.KERNEL_PLANES if p <= 3 else mf.KERNEL_AUTO)
    assert op.kernel_name() == "apply_planes3"
    if p == 4 and n in (12, 18):
        assert op.plan_stats()["index_records"] == "shared"
    if wgs:
        assert op.plan_stats()["n_batches"] >= 3 * wgs
    x, y = check_vmult_and_add(op, od, c, nt)
    np.testing.assert_array_equal(gpu_vmult(op_x, x, nt), y)
    y0 = np.ones(mesh.n_dofs)
    np.testing.assert_array_equal(gpu_vmult(op_x, x, nt, y0=y0), gpu_vmult(op, x, nt, y0=y0))


@pytest.mark.parametrize("make,kern", [(lambda: mf.Mesh.uniform(3, 4, 6), 0), (lambda: mf.Mesh.uniform(3, 2, 9), 0),
                                       (lambda: mf.Mesh.uniform(3, 3, 6), mf.KERNEL_PLANES_2W),
                                       (lambda: mf.Mesh.uniform(3, 5, 4), 0), (lambda: mf.Mesh.adaptive(3, 4, 4), 0),
                                       (lambda: mf.Mesh.adaptive(3, 2, 4), 0), (lambda: mf.Mesh.ball(3, 2, 2), 0),
                                       (lambda: mf.Mesh.uniform(2, 2, 16), 0)],
                         ids=["cube_p4", "cube_p2", "cube_p3_2w", "cube_p5", "adaptive_p4", "adaptive_p2", "ball", "cube_2d"])
@pytest.mark.parametrize("segments,wgs", [(1, 0), (2, 0), (2, 3)])
def test_segments_and_few_workgroups(make, kern, segments, wgs):
    mesh = make()
    od, c = mass_mesh(mesh, seed=segments)
    mesh.desc.kernel = kern
    mesh.desc.cell_loop_segments = segments
    mesh.desc.max_workgroups = wgs
    check_vmult_and_add(mf.Operator(mesh.desc, mesh), od, c)


REPEAT = [("planes3", lambda: mf.Mesh.uniform(3, 4, 7), dict()), ("planes3_hn", lambda: mf.Mesh.adaptive(3, 4, 4), dict()),
          ("planes4", lambda: mf.Mesh.uniform(3, 3, 6), dict(kernel=mf.KERNEL_PLANES_2W)),
          ("x_one_cell_batches", lambda: mf.Mesh.uniform(3, 2, 5), dict()),
          ("batches_2d_colored", lambda: mf.Mesh.uniform(2, 2, 9), dict(colored=True)),
          ("g_one_cell_batches", lambda: mf.Mesh.ball(3, 2, 1), dict()), ("g2", lambda: mf.Mesh.ball(2, 2, 2), dict()),
          ("x_multi_cell_batches", lambda: mf.Mesh.uniform(3, 4, 6), dict(kernel=mf.KERNEL_PENCILS_X, max_cells_per_batch=27)),
          ("batches_multi_cell_batches", lambda: mf.Mesh.uniform(3, 2, 10), dict(kernel=mf.KERNEL_PENCILS, max_cells_per_batch=256)),
          ("g_multi_cell_batches", lambda: mf.Mesh.ball(3, 2, 2), dict(max_cells_per_batch=16))]


@pytest.mark.parametrize("name,make,knobs", REPEAT, ids=[r[0] for r in REPEAT])
def test_two_calls_are_bitwise_equal(name, make, knobs):
    """Two vmults on the same inputs give the same bits, in every family, also on batches of several cells.

    The plane kernels have it by construction (one wave owns a batch: its LDS adds execute in program order).  The
    pencil families' MASS instantiations add the cells of a chunk into the batch accumulator one after the other; the
    Laplace operator's do not (four waves' ds_add_f64 meet in arrival order: last-bit differences on batches of several
    cells), which the test prints for comparison and does not assert."""
    mesh = make()
    colored = knobs.pop("colored", False)
    for k, v in knobs.items():
        setattr(mesh.desc, k, v)
    if colored:
        mesh.desc.flags |= mf.COLORED_SCATTER
    x = np.random.default_rng(5).standard_normal(mesh.n_dofs)
    lap = mf.Operator(mesh.desc, mesh)
    y1, y2 = gpu_vmult(lap, x), gpu_vmult(lap, x)
    print(f"{name} ({lap.kernel_name()}): Laplace operator, entries that differ between two calls: {np.count_nonzero(y1 != y2)} "
          f"of {y1.size}, max rel {np.abs(y1 - y2).max() / np.abs(y1).max():.2e}")
    mass_mesh(mesh, seed=1)
    op = mf.Operator(mesh.desc, mesh)
    z1, z2 = gpu_vmult(op, x), gpu_vmult(op, x)
    print(f"{name} ({op.kernel_name()}): with the mass term: {np.count_nonzero(z1 != z2)} of {z1.size}, "
          f"max rel {np.abs(z1 - z2).max() / np.abs(z1).max():.2e}")
    np.testing.assert_array_equal(z1, z2)


# ---- 2. an all-zero mass coefficient is the Laplace operator


@pytest.mark.parametrize("make", [lambda nt: mf.Mesh.uniform(3, 4, 5, number_type=nt), lambda nt: mf.Mesh.uniform(2, 3, 8, number_type=nt),
                                  lambda nt: mf.Mesh.adaptive(3, 4, 4, number_type=nt), lambda nt: mf.Mesh.ball(3, 2, 1, number_type=nt),
                                  lambda nt: mf.Mesh.uniform(3, 6, 2, number_type=nt)],
                         ids=["cube_p4", "cube_2d", "adaptive", "ball", "cube_p6"])
@pytest.mark.parametrize("nt", [mf.F64, mf.F32])
def test_zero_mass_coefficient_agrees_with_null(make, nt):
    mesh = make(nt)
    x = np.random.default_rng(1).standard_normal(mesh.n_dofs)
    y_null = gpu_vmult(mf.Operator(mesh.desc, mesh), x, nt)
    mesh.set_mass_coefficient(np.zeros(mesh.n_cells * mesh.nd))
    y_zero = gpu_vmult(mf.Operator(mesh.desc, mesh), x, nt)
    assert rel(y_zero, y_null) <= TOL[nt]


# ---- 3. the analytic known answer


@pytest.mark.parametrize("make,dim", [(lambda p: mf.Mesh.uniform(2, p, 5), 2), (lambda p: mf.Mesh.uniform(3, p, 4), 3),
                                      (lambda p: mf.Mesh.adaptive(3, p, 4), 3), (lambda p: mf.Mesh.adaptive(2, p, 4), 2)],
                         ids=["cube_2d", "cube_3d", "adaptive_3d", "adaptive_2d"])
@pytest.mark.parametrize("p", [2, 4])
def test_known_answer_mass_energy(make, dim, p):
    """coefficient = 0, c = 1, u = prod_d (1 - x_d^2): u^T A u = (16/15)^dim"""
    mesh = make(p)
    a = mesh.arrays()
    zero = np.zeros(mesh.n_cells * mesh.nd)
    mesh.desc.coefficient = zero.ctypes.data
    mesh.set_mass_coefficient(np.ones(mesh.n_cells * mesh.nd))
    op = mf.Operator(mesh.desc, mesh)
    u = hr.known_answer_vector(mesh.dof_coords(), a["constrained_dofs"])
    exact = (16.0 / 15.0) ** dim
    got = u @ gpu_vmult(op, u)
    print(f"u^T A u = {got!r}, exact {exact!r}, rel {abs(got - exact) / exact:.3e}")
    assert abs(got - exact) <= 1e-12 * exact


# ---- 4. inverse diagonal


def _check_diag(op, od, c, nt=mf.F64):
    d = mf.DeviceVector(od.n_dofs, nt)
    d.fill(123.0)
    op.compute_inverse_diagonal(d)
    mf.synchronize()
    got, ref = d.to_host(), hr.inverse_diagonal(od, c)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    print("diag max rel", np.abs(got / ref - 1).max())
    np.testing.assert_allclose(got, ref, rtol=DIAG_TOL[nt])


@pytest.mark.parametrize("nt", [mf.F64, mf.F32])
@pytest.mark.parametrize("dim,p,n", [(2, 1, 7), (2, 2, 16), (2, 4, 5), (2, 6, 3), (3, 1, 5), (3, 2, 5), (3, 3, 3),
                                     (3, 4, 4), (3, 5, 2), (3, 6, 2)])
def test_inverse_diagonal(dim, p, n, nt):
    mesh = mf.Mesh.uniform(dim, p, n, number_type=nt)
    od, c = mass_mesh(mesh, nt, seed=p)
    op = mf.Operator(mesh.desc, mesh)
    _check_diag(op, od, c, nt)
    if nt == mf.F64:  # and against the assembled matrix
        d = mf.DeviceVector(od.n_dofs)
        op.compute_inverse_diagonal(d)
        np.testing.assert_allclose(1.0 / d.to_host(), hr.assemble(od, c).diagonal(), rtol=1e-11)


@pytest.mark.parametrize("dim,p,nref", [(2, 2, 4), (2, 4, 4), (3, 1, 4), (3, 2, 4), (3, 4, 4)])
def test_inverse_diagonal_with_hanging_nodes(dim, p, nref):
    mesh = mf.Mesh.adaptive(dim, p, nref)
    od, c = mass_mesh(mesh, seed=p)
    _check_diag(mf.Operator(mesh.desc, mesh), od, c)


@pytest.mark.parametrize("what", ["deformed_3d", "deformed_2d", "ball_3d", "ball_2d", "deformed_hanging"])
def test_inverse_diagonal_general_geometry(what):
    if what.startswith("ball"):
        mesh = mf.Mesh.ball(int(what[-2]), 3, 1)
        od, c = mass_mesh(mesh, seed=2)
        return _check_diag(mf.Operator(mesh.desc, mesh), od, c)
    if what == "deformed_3d":
        od = deformed_oracle_desc(4, 3, seed=5)
    elif what == "deformed_2d":
        od = deform(o.uniform_mesh_desc(2, 3, 6), eps=0.15, seed=5)
    else:
        mesh = mf.Mesh.adaptive(3, 2, 4)  # (the description's arrays are views into the mesh)
        od = deform(oracle_desc_from_mesh(mesh, dtype=np.float64), seed=4)
    c = random_c(od.n_cells, od.nd, seed=3)
    desc, keep = desc_from_oracle(od, mass_coefficient=c)
    _check_diag(mf.Operator(desc, keep), od, c)


# ---- 5. integrator


@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 1), ("cube", 2, 4), ("hanging", 2, 2), ("hanging", 2, 4), ("ball", 2, 2),
                                        ("cube", 3, 2), ("cube", 3, 4), ("cube", 3, 6), ("hanging", 3, 2),
                                        ("hanging", 3, 4), ("ball", 3, 2), ("ball", 3, 4)])
def test_rhs_with_lift_matches_reference(kind, dim, p):
    from test_gpu_poisson import small_mesh
    mesh = small_mesh(kind, dim, p)
    cells = pr.Cells(mesh)
    c = random_c(mesh.n_cells, mesh.nd, seed=p)
    u = dv(cells.interpolant())
    l2_plain = mf.Integrator(mesh.desc, mesh).l2_error(u)
    mesh.set_mass_coefficient(c)
    it = mf.Integrator(mesh.desc, mesh)
    ub = cells.lift()
    f = np.random.default_rng(p).standard_normal(cells.qpts.shape[:2])
    dst = mf.DeviceVector(mesh.n_dofs)
    dst.fill(np.nan)
    it.rhs(dst, dv(f.reshape(-1)), dv(ub))
    close(dst.to_host(), hr.rhs(cells, c, f, ub), 1e-12)
    it.rhs(dst, None, dv(ub))  # f_qp = NULL keeps meaning the built-in Poisson load
    close(dst.to_host(), hr.rhs(cells, c, None, ub), 1e-12)
    it.rhs(dst, dv(f.reshape(-1)))  # no lift: the field does not enter
    close(dst.to_host(), cells.rhs(f, None), 1e-12)
    assert it.l2_error(u) == l2_plain  # the L2 error is unchanged by the field


# ---- 6. level operator and interface matrices


@pytest.mark.parametrize("dim,p,n,nt", [(2, 2, 8, mf.F64), (2, 4, 6, mf.F64), (3, 1, 6, mf.F64), (3, 2, 4, mf.F64),
                                        (3, 4, 4, mf.F64), (3, 4, 6, mf.F32), (3, 3, 4, mf.F64), (3, 5, 3, mf.F64)])
@pytest.mark.parametrize("touch_boundary", [False, True])
def test_level_operator_and_interface_matrices(dim, p, n, nt, touch_boundary):
    from test_gpu_level import _edge_of_box
    mesh = mf.Mesh.uniform(dim, p, n, number_type=nt)
    od, c = mass_mesh(mesh, nt, seed=p)
    h = 2.0 / n
    edge = _edge_of_box(mesh, -1.0 + (0.0 if touch_boundary else h), -1.0 + h * (n // 2 + 1))
    assert 0 < len(edge) < mesh.n_dofs
    lev = mf.Level(mesh.desc, edge, mesh)
    x = np.random.default_rng(dim * 10 + p).standard_normal(mesh.n_dofs).astype(mf.np_dtype(nt)).astype(np.float64)
    a, b = mf.DeviceVector(mesh.n_dofs, nt), mf.DeviceVector(mesh.n_dofs, nt)
    a.from_host(x)
    odc = o.Desc(dim, p, od.n_dofs, od.loc2glob, od.JxW, od.inv_jac, od.coefficient,
                 np.union1d(od.constrained, edge).astype(np.uint32), None, np.float64, od.shape_values, od.shape_gradients)
    lev.vmult(b, a)
    mf.synchronize()
    assert rel(b.to_host(), hr.vmult(odc, c, x)) <= TOL[nt]
    for fn, ref, plain in ((lev.vmult_interface_down, hr.vmult_interface_down, o.vmult_interface_down),
                           (lev.vmult_interface_up, hr.vmult_interface_up, o.vmult_interface_up)):
        b.fill(5.0)
        fn(b, a)
        mf.synchronize()
        want = ref(od, c, edge, x)
        got = b.to_host().astype(np.float64)
        assert np.linalg.norm(got - want) <= TOL[nt] * np.linalg.norm(want)
        assert np.linalg.norm(want - plain(od, edge, x)) > 1e-6 * np.linalg.norm(want)  # (the term is there)
        np.testing.assert_array_equal(a.to_host(), x.astype(mf.np_dtype(nt)))


# ---- 7. two z-slabs on one GPU


def rough_c(x):
    """a mass coefficient in [0.5, 1.5] defined by position (the same on a slab and on the whole mesh), far from smooth
    on the scale of a cell"""
    return 1.0 + 0.5 * np.sin(37.0 * x[..., 0] + 11.0 * x[..., 1] ** 2 - 23.0 * x[..., -1])


@pytest.mark.parametrize("p,n,world", [(4, 6, 2), (2, 8, 2), (4, 12, 2), (5, 8, 2), (3, 6, 2)])
@pytest.mark.parametrize("nt", [mf.F64, mf.F32])
def test_two_slabs_in_process(p, n, world, nt):
    from pymfgpu.parallel import slab_ranges
    full = mf.Mesh.uniform(3, p, n, number_type=nt)
    od = oracle_desc_from_mesh(full, dtype=np.float64)
    c_full = rough_c(full.arrays()["quadrature_points"].astype(np.float64)).astype(mf.np_dtype(nt)).astype(np.float64)
    full.set_mass_coefficient(c_full)
    key = {tuple(np.round(q, 9)): i for i, q in enumerate(full.dof_coords())}
    slabs = []
    for r, (zb, ze) in enumerate(slab_ranges(n, world)):
        mesh = mf.Mesh.uniform(3, p, n, slab=(zb, ze), number_type=nt)
        mesh.set_mass_coefficient(rough_c(mesh.arrays()["quadrature_points"].astype(np.float64)))
        gi = np.array([key[tuple(np.round(q, 9))] for q in mesh.dof_coords()])
        op = mf.Operator(mesh.desc, mesh)
        dist = mf.Dist(mesh, r, world)
        dist.attach(op)
        slabs.append(dict(mesh=mesh, op=op, dist=dist, gi=gi, a=mf.DeviceVector(mesh.n_dofs, nt), b=mf.DeviceVector(mesh.n_dofs, nt)))
    for lo, up in zip(slabs, slabs[1:]):
        lo["dist"].connect_local(up["dist"])
    fx = full.dof_coords()
    x = (np.sin(3 * fx[:, 0]) + fx[:, 1] ** 2 - np.cos(2 * fx[:, 2]) * fx[:, 0]).astype(mf.np_dtype(nt)).astype(np.float64)
    single = gpu_vmult(mf.Operator(full.desc, full), x, nt)
    for s in slabs:
        s["a"].from_host(x[s["gi"]])
    for s in slabs:
        s["dist"].vmult_begin(s["op"], s["b"], s["a"])
    for s in slabs:
        s["dist"].vmult_end(s["op"], s["b"])
    mf.synchronize()
    ref = hr.vmult(od, c_full, x)
    assert rel(single, ref) <= TOL[nt]
    for s in slabs:
        assert rel(s["b"].to_host(), ref[s["gi"]]) <= TOL[nt]
        assert rel(s["b"].to_host(), single[s["gi"]]) <= TOL[nt]


# ---- 8. convergence of the driver's problem through the binding


def gpu_solve(mesh):
    """helmholtz.cc through the binding: u_b = Solution on the constrained dofs, f = RightHandSide + c Solution, rhs with
    the lift, the Jacobi-PCG of test_gpu_poisson.gpu_solve to 1e-12 |rhs|, u = u_b + x, L2 error against Solution"""
    qpts = mesh.arrays()["quadrature_points"].astype(np.float64)
    mesh.set_mass_coefficient(hr.mass_function(qpts))
    op = mf.Operator(mesh.desc, mesh)
    it = mf.Integrator(mesh.desc, mesh)
    N = mesh.n_dofs
    con = mesh.arrays()["constrained_dofs"]
    ub_h = np.zeros(N)
    ub_h[con] = pr.solution(mesh.dof_coords()[con])
    ub = dv(ub_h)
    b, x, r, z, pv, q, dinv = (mf.DeviceVector(N) for _ in range(7))
    it.rhs(b, dv(hr.load(qpts).reshape(-1)), ub)
    op.compute_inverse_diagonal(dinv)
    r.equ(1.0, b)
    z.equ(1.0, r)
    z.scale(dinv)
    pv.equ(1.0, z)
    rz = r.dot(z)
    tol = 1e-12 * b.l2_norm()
    for its in range(1, 20000):
        op.vmult(q, pv)
        alpha = rz / pv.dot(q)
        x.add(alpha, pv)
        r.add(-alpha, q)
        if r.l2_norm() <= tol:
            break
        z.equ(1.0, r)
        z.scale(dinv)
        rz_new = r.dot(z)
        pv.sadd(rz_new / rz, 1.0, z)
        rz = rz_new
    assert its < 19999, "CG did not converge"
    x.add(1.0, ub)
    return it.l2_error(x)


CPU_SOLVE_MAX_DOFS = 10000  # the levels the CPU reference solves (spsolve on the assembled matrix)


@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 2), ("cube", 3, 2), ("cube", 3, 4), ("hanging", 2, 2),
                                        ("hanging", 3, 2), ("ball", 2, 2), ("ball", 3, 2)])
def test_known_answer_convergence(kind, dim, p):
    errs, cpu = [], []
    for level in range(3):
        mesh = pr.family(kind, dim, p, level)
        small = mesh.n_dofs <= CPU_SOLVE_MAX_DOFS
        if small:
            cpu.append(hr.solve(pr.Cells(mesh))[1])
        errs.append(gpu_solve(mesh))
        if small:
            np.testing.assert_allclose(errs[-1], cpu[-1], rtol=1e-6)
    assert cpu
    order = pr.orders(errs)[-1]
    print(kind, dim, p, "errors", errs, "order", order)
    if kind == "ball":
        assert order >= (HELMHOLTZ_BALL_ORDER_2D_P2 if dim == 2 else HELMHOLTZ_BALL_ORDER_3D_P2) - 0.2, errs
    else:
        assert order >= p + 0.7, errs


# ---- 9. the drivers


def _run(exe, args):
    out = subprocess.run([os.path.join(ROOT, "dealii-cuda_amd", "host", "bin", exe)] + args, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert all(len(r) == 6 for r in rows), out.stdout
    return rows


@pytest.mark.parametrize("exe,dim,p,ndofs", [("helmholtz-2d-p2", 2, 2, [17 ** 2, 33 ** 2, 65 ** 2]),
                                             ("helmholtz-3d-p4", 3, 4, [17 ** 3, 33 ** 3, 65 ** 3])])
def test_helmholtz_driver_cube(exe, dim, p, ndofs):
    rows = _run(exe, ["-q", "0", "2"])
    assert len(rows) == 3
    for r, nd in zip(rows, ndofs):
        assert int(r[0]) == dim and int(r[1]) == p and int(r[2]) == nd and 1 <= int(r[3]) < 10000
    errs = [float(r[5]) for r in rows]
    print(exe, errs, pr.orders(errs))
    assert pr.orders(errs)[-1] >= p + 0.7, errs


@pytest.mark.parametrize("exe", ["helmholtz-3d-p2-ball", "helmholtz-3d-p4-adaptive"])
def test_helmholtz_driver_ball_and_adaptive(exe):
    rows = _run(exe, ["-q", "0", "1"])
    assert len(rows) == 2
    errs = [float(r[5]) for r in rows]
    print(exe, errs)
    assert all(np.isfinite(e) and e > 0 for e in errs) and errs[0] > errs[1], errs
