"""GPU cell integrals of a Poisson solve (mfgpu_integrator: poisson.cu:182-221 right-hand side with the Dirichlet
lift, poisson.cu:277-292 L2 error on QGauss(p+2)) against the numpy restatement in tests/poisson_reference.py, and
the known answer the reference holds: a Poisson solve whose L2 error against the analytic Solution<dim> falls at order
p + 1 on uniform, hanging-node and ball meshes."""
import os
import subprocess

import numpy as np
import pytest

import poisson_reference as pr
import pymfgpu as mf
from oracle import mf_oracle as o
from test_poisson_host import BALL_ORDER_2D_P2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured with the CPU reference (Cells.solve) on the ball, 3D p = 2, n_ref 1..3: L2 errors 0.1005, 0.01399,
# 0.002016, orders 2.84, 2.80
BALL_ORDER_3D_P2 = 2.80


def dv(a):
    v = mf.DeviceVector(len(a))
    v.from_host(np.ascontiguousarray(a, dtype=np.float64))
    return v


def close(got, ref, rtol):
    scale = max(np.abs(ref).max(), 1e-300)
    assert np.abs(got - ref).max() <= rtol * scale, (np.abs(got - ref).max(), scale)


CASES = [("cube", 2, 1), ("cube", 2, 2), ("cube", 2, 4), ("hanging", 2, 1), ("hanging", 2, 2), ("hanging", 2, 4),
         ("ball", 2, 2), ("ball", 2, 4), ("cube", 3, 1), ("cube", 3, 2), ("cube", 3, 4), ("cube", 3, 6),
         ("hanging", 3, 1), ("hanging", 3, 2), ("hanging", 3, 4), ("ball", 3, 1), ("ball", 3, 2), ("ball", 3, 4),
         ("ball", 3, 6)]


def small_mesh(kind, dim, p):
    if kind == "cube":
        return mf.Mesh.uniform(dim, p, 3 if dim == 2 or p <= 2 else 2)
    if kind == "hanging":
        return mf.Mesh.adaptive(dim, p, 3 if dim == 2 else 4)
    return mf.Mesh.ball(dim, p, 1 if dim == 2 else 0)


@pytest.mark.parametrize("kind,dim,p", CASES)
def test_rhs_matches_reference(kind, dim, p):
    mesh = small_mesh(kind, dim, p)
    c = pr.Cells(mesh)
    it = mf.Integrator(mesh.desc, mesh)
    N = mesh.n_dofs
    ub = c.lift()
    dst = mf.DeviceVector(N)
    dst.fill(np.nan)  # every entry is written
    it.rhs(dst, None, dv(ub))
    close(dst.to_host(), c.rhs(None, ub), 1e-12)
    f = np.random.default_rng(p).standard_normal(c.qpts.shape[:2])
    it.rhs(dst, dv(f.reshape(-1)))
    close(dst.to_host(), c.rhs(f, None), 1e-12)


def _unconstrained_with_mask(od):
    return o.Desc(od.dim, od.degree, od.n_dofs, od.loc2glob, od.JxW, od.inv_jac, od.coefficient,
                  np.zeros(0, np.uint32), od.constraint_mask, np.float64, od.shape_values, od.shape_gradients,
                  od.weights)


@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 2), ("hanging", 2, 2), ("ball", 2, 4), ("cube", 3, 4),
                                        ("hanging", 3, 2), ("ball", 3, 2)])
def test_lift_is_minus_stiffness(kind, dim, p):
    mesh = small_mesh(kind, dim, p)
    c = pr.Cells(mesh)
    od = c.od
    it = mf.Integrator(mesh.desc, mesh)
    ub = np.random.default_rng(7).standard_normal(mesh.n_dofs)
    dst = mf.DeviceVector(mesh.n_dofs)
    it.rhs(dst, dv(np.zeros(c.qpts.shape[0] * c.qpts.shape[1])), dv(ub))
    got = dst.to_host()
    K = o.assemble(_unconstrained_with_mask(od))
    free = np.ones(mesh.n_dofs, bool)
    free[od.constrained] = False
    close(got[free], -(K @ ub)[free], 1e-12)
    assert np.all(got[~free] == 0.0)


@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 2), ("hanging", 2, 3), ("cube", 3, 4), ("hanging", 3, 2),
                                        ("ball", 3, 2)])
def test_partition_of_unity(kind, dim, p):
    mesh = small_mesh(kind, dim, p)
    mesh.desc.n_constrained = 0
    it = mf.Integrator(mesh.desc, mesh)
    jxw = mesh.arrays()["JxW"]
    dst = mf.DeviceVector(mesh.n_dofs)
    it.rhs(dst, dv(np.ones(jxw.size)))
    assert abs(dst.to_host().sum() - jxw.sum()) <= 1e-13 * jxw.sum()


@pytest.mark.parametrize("kind,dim,p", CASES)
def test_error_integrals(kind, dim, p):
    mesh = small_mesh(kind, dim, p)
    c = pr.Cells(mesh)
    it = mf.Integrator(mesh.desc, mesh)
    nc, ne = mesh.n_cells, it.n_error_points
    # the error points
    np.testing.assert_allclose(it.error_points(), c.xe, rtol=0, atol=1e-13)
    # volume: exact = 1, u = 0
    l2 = it.l2_error(dv(np.zeros(mesh.n_dofs)), dv(np.ones(nc * ne)))
    assert abs(l2 ** 2 - c.od.JxW.sum()) <= 1e-13 * c.od.JxW.sum()
    # the Solution interpolant against the numpy reference; per-cell squared errors
    u = c.interpolant()
    pc = mf.DeviceVector(nc)
    l2 = it.l2_error(dv(u), None, pc)
    ref, ref_pc = c.l2_error(u)
    assert abs(l2 - ref) <= 1e-12 * ref
    close(pc.to_host(), ref_pc, 1e-12)
    assert abs(pc.to_host().sum() - l2 ** 2) <= 1e-13 * l2 ** 2


@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 2), ("cube", 2, 4), ("hanging", 2, 2), ("hanging", 2, 4),
                                        ("cube", 3, 3), ("hanging", 3, 2), ("hanging", 3, 4)])
def test_qp_polynomial_exact_and_hanging_dofs_unread(kind, dim, p):
    mesh = small_mesh(kind, dim, p)
    c = pr.Cells(mesh)
    it = mf.Integrator(mesh.desc, mesh)
    coef = np.random.default_rng(p).standard_normal((p + 1,) * dim)

    def poly(x):
        v = 0.0
        for idx in np.ndindex(*coef.shape):
            v = v + coef[idx] * np.prod([x[..., d] ** idx[d] for d in range(dim)], axis=0)
        return v

    u = c.interpolant(poly)
    unread = np.ones(mesh.n_dofs, bool)
    unread[c.od.loc2glob.reshape(-1)] = False
    assert (kind == "hanging") == bool(unread.any())
    u[unread] = np.nan
    l2 = it.l2_error(dv(u), dv(poly(it.error_points()).reshape(-1)))
    assert l2 <= 1e-12


def test_repeated_calls_are_bitwise_equal():
    mesh = mf.Mesh.adaptive(3, 2, 4)
    c = pr.Cells(mesh)
    it = mf.Integrator(mesh.desc, mesh)
    ub = dv(c.lift())
    a, b = mf.DeviceVector(mesh.n_dofs), mf.DeviceVector(mesh.n_dofs)
    it.rhs(a, None, ub)
    it.rhs(b, None, ub)
    assert np.array_equal(a.to_host(), b.to_host())
    u = dv(c.interpolant())
    assert it.l2_error(u) == it.l2_error(u)


def test_argument_checks():
    mesh = mf.Mesh.uniform(3, 2, 2, number_type=mf.F32)
    with pytest.raises(mf.MfgpuError, match="error -4"):
        mf.Integrator(mesh.desc, mesh)
    mesh = mf.Mesh.uniform(3, 2, 2)
    mesh.desc.quadrature_points = None
    with pytest.raises(mf.MfgpuError, match="error -1.*quadrature_points"):
        mf.Integrator(mesh.desc, mesh)


def gpu_solve(mesh):
    """poisson.cu:152-292 on the GPU: u_b = Solution on the constrained dofs, rhs with the lift, Jacobi-PCG to
    1e-12 |rhs|, u = u_b + x, L2 error against Solution"""
    op = mf.Operator(mesh.desc, mesh)
    it = mf.Integrator(mesh.desc, mesh)
    N = mesh.n_dofs
    con = mesh.arrays()["constrained_dofs"]
    ub_h = np.zeros(N)
    ub_h[con] = pr.solution(mesh.dof_coords()[con])
    ub = dv(ub_h)
    b, x, r, z, pv, q, dinv = (mf.DeviceVector(N) for _ in range(7))
    it.rhs(b, None, ub)
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


@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 2), ("cube", 3, 2), ("cube", 3, 4), ("hanging", 2, 2),
                                        ("hanging", 3, 2), ("ball", 2, 2), ("ball", 3, 2)])
def test_known_answer_convergence(kind, dim, p):
    errs, cpu = [], []
    for level in range(3):
        mesh = pr.family(kind, dim, p, level)
        errs.append(gpu_solve(mesh))
        if dim == 2:
            cpu.append(pr.Cells(mesh).solve()[1])
    if cpu:
        np.testing.assert_allclose(errs, cpu, rtol=1e-6)
    order = pr.orders(errs)[-1]
    if kind == "ball":
        assert order >= (BALL_ORDER_2D_P2 if dim == 2 else BALL_ORDER_3D_P2) - 0.2, errs
    else:
        assert order >= p + 0.7, errs


def _run(exe, args):
    out = subprocess.run([os.path.join(ROOT, "dealii-cuda_amd", "host", "bin", exe)] + args, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert all(len(r) == 6 for r in rows), out.stdout
    return rows


@pytest.mark.parametrize("exe,dim,p,ndofs", [("poisson-2d-p2", 2, 2, [17 ** 2, 33 ** 2, 65 ** 2]),
                                             ("poisson-3d-p2", 3, 2, [9 ** 3, 17 ** 3, 33 ** 3]),
                                             ("poisson-3d-p4", 3, 4, [17 ** 3, 33 ** 3, 65 ** 3])])
def test_poisson_driver_cube(exe, dim, p, ndofs):
    rows = _run(exe, ["-q", "0", "2"])
    assert len(rows) == 3
    for r, nd in zip(rows, ndofs):
        assert int(r[0]) == dim and int(r[1]) == p and int(r[2]) == nd and 1 <= int(r[3]) < 10000
    errs = [float(r[5]) for r in rows]
    assert pr.orders(errs)[-1] >= p + 0.7, errs


@pytest.mark.parametrize("exe", ["poisson-3d-p2-ball", "poisson-3d-p4-adaptive"])
def test_poisson_driver_ball_and_adaptive(exe):
    rows = _run(exe, ["-q", "0", "2"])
    assert len(rows) == 3
    errs = [float(r[5]) for r in rows]
    assert errs[0] > errs[1] > errs[2], errs
