"""The device-side coefficient loop end to end: a Picard iteration for -div((1 + u^2) grad u) = f through pymfgpu
(Integrator.evaluate, a = 1 + u^2 by vector operations, update_coefficients of operator and integrator, inverse
diagonal, right-hand side with the lift, Jacobi-PCG) against tests/nonlinear_reference.picard, and the nonlinear-*
drivers of dealii-cuda_amd/host."""
import os
import subprocess

import numpy as np
import pytest

import nonlinear_reference as nr
import poisson_reference as pr
import pymfgpu as mf
from test_gpu import rel
from test_gpu_poisson import dv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 8
# How far the reference's 8th iterate moves (relative l2) when its direct solve is replaced by the GPU test's solver,
# Jacobi-PCG to 1e-12 |rhs| (nonlinear_reference.jacobi_pcg), measured on the CPU: 2D p=2 n=8 1.35e-13, 3D p=2 n=4
# 7.78e-13.  The GPU iterate may differ from the reference by 10x that (the factor covers the summation order).
CG_DRIFT = {(2, 2, 8): 1.35e-13, (3, 2, 4): 7.78e-13}
# Picard steps of the reference (direct solve) to a relative update of 1e-10 at the drivers' two smallest meshes,
# measured on the CPU: 2D p=2 n=8, 16: 16, 14 (L2 errors 1.400e-2, 1.711e-3); 3D p=4 n=4, 8: 19, 15 (4.531e-3, 1.660e-4)
CPU_PICARD_STEPS = {"nonlinear-2d-p2": [16, 14], "nonlinear-3d-p4": [19, 15]}


def gpu_picard(mesh, steps):
    mesh.desc.flags |= mf.UPDATABLE_COEFFICIENTS
    op = mf.Operator(mesh.desc, mesh)  # (the built-in coefficient until the first update)
    it = mf.Integrator(mesh.desc, mesh)
    N, nq = mesh.n_dofs, mesh.n_cells * mesh.nd
    con = mesh.arrays()["constrained_dofs"]
    ub_h = np.zeros(N)
    ub_h[con] = pr.solution(mesh.dof_coords()[con])
    ub, u = dv(ub_h), dv(ub_h)
    f = dv(nr.load(mesh.arrays()["quadrature_points"].astype(np.float64)).reshape(-1))
    ones, u_qp, a = mf.DeviceVector(nq), mf.DeviceVector(nq), mf.DeviceVector(nq)
    ones.fill(1.0)
    b, x, r, z, pv, q, dinv = (mf.DeviceVector(N) for _ in range(7))
    for _ in range(steps):
        it.evaluate(u, values=u_qp)
        a.equ(1.0, u_qp)
        a.scale(u_qp)
        a.sadd(1.0, 1.0, ones)  # a = 1 + u^2
        op.update_coefficients(a)
        it.update_coefficients(a)
        op.compute_inverse_diagonal(dinv)
        it.rhs(b, f, ub)
        x.fill(0.0)
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
        u.equ(1.0, ub)
        u.add(1.0, x)
    return u.to_host()


@pytest.mark.parametrize("dim,p,n", [(2, 2, 8), (3, 2, 4)])
def test_picard_matches_reference(dim, p, n):
    """8 fixed Picard steps.  Reference with its direct solve against the same reference with Jacobi-PCG at the GPU
    solve's tolerance, relative l2 of the 8th iterate, measured on the CPU: 1.35e-13 (2D p=2 n=8), 7.78e-13 (3D p=2
    n=4); allowed here: 10x, i.e. 1.35e-12 and 7.78e-12."""
    mesh = mf.Mesh.uniform(dim, p, n)
    ref, hist = nr.picard(pr.Cells(mesh), steps=STEPS)
    got = gpu_picard(mesh, STEPS)
    err = rel(got, ref)
    print(f"{dim}D p={p} n={n}: GPU vs reference {err:.3e} (allowed {10 * CG_DRIFT[(dim, p, n)]:.3e}); reference update "
          f"norms {hist[0]:.2e} .. {hist[-1]:.2e}")
    assert err <= 10 * CG_DRIFT[(dim, p, n)]


@pytest.mark.parametrize("exe,dim,p,ndofs", [("nonlinear-2d-p2", 2, 2, [17 ** 2, 33 ** 2]),
                                             ("nonlinear-3d-p4", 3, 4, [17 ** 3, 33 ** 3])])
def test_nonlinear_driver_cube(exe, dim, p, ndofs):
    out = subprocess.run([os.path.join(ROOT, "dealii-cuda_amd", "host", "bin", exe), "-q", "0", "1"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    print(out.stdout)
    assert len(rows) == 2 and all(len(r) == 7 for r in rows), out.stdout
    for r, nd, cpu_steps in zip(rows, ndofs, CPU_PICARD_STEPS[exe]):
        assert int(r[0]) == dim and int(r[1]) == p and int(r[2]) == nd
        assert 1 <= int(r[3]) <= cpu_steps + 2, (r, cpu_steps)
        assert int(r[3]) <= int(r[4]) < 10000 * int(r[3])
    errs = [float(r[6]) for r in rows]
    assert pr.orders(errs)[-1] >= p + 0.7, errs
