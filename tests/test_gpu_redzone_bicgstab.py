"""BiCGStab.solve with x, b and the borrowed inverse diagonal between red zones (tests/redzone.py): 4096 NaN elements
on each side of every caller-owned array, once 16-byte aligned and once one element off (the scalar path of every
solver kernel).  The bounds are those of tests/test_gpu_bicgstab.py::test_solve_to_convergence_*."""
import numpy as np
import pytest

import pymfgpu as mf
from redzone import Zoned
from test_bicgstab_host import CASES
from test_gpu_bicgstab import device, laplace_reference
from test_gpu_cg import NT, problem

pytestmark = pytest.mark.gpu

ALIGN = pytest.mark.parametrize("offset_one", [False, True], ids=["aligned", "offset"])


def zoned_solve(make_solver, reference, A, dinv, b, dt, tol, bound, offset_one):
    nt = NT[dt]
    tolerance = tol * np.linalg.norm(b)
    ref_it, ref_status, ref_res, _ = list(reference(tolerance))[-1]
    assert ref_status == 1 and ref_res <= tolerance
    zd, zb, zx = Zoned(dinv, nt, offset_one), Zoned(b, nt, offset_one), Zoned(len(b), nt, offset_one)
    solver = make_solver(zd.vec)
    info = solver.solve(zx.vec, zb.vec, tolerance, 10000, check_every=5)  # (begin writes every entry of x)
    x = zx.result()
    zb.unchanged()
    zd.unchanged()
    true = np.linalg.norm(b - A @ x.astype(np.float64)) / np.linalg.norm(b)
    print(f"iterations {info.iterations} (reference {ref_it}), true residual {true:.3e} (bound {bound:.0e})")
    assert info.status == 1 and info.residual <= tolerance and true <= bound
    assert 0 < info.iterations <= 2 * ref_it


@ALIGN
def test_qop_solve_double(offset_one):
    kind, dim, p, cset, prec = CASES[1]
    D = device(kind, dim, p, cset)
    P = D.P
    b = P.rhs()
    zoned_solve(lambda dinv: mf.BiCGStab(D.q, mf.CG_JACOBI, dinv), lambda t: P.reference(prec, np.float64, b, t, 10000),
                P.A, P.dinv, b, np.float64, 1e-10, 2e-10, offset_one)


@ALIGN
def test_laplace_solve_float(offset_one):
    P = problem(2, 2, 8)
    b = P.rhs(1)
    zoned_solve(lambda dinv: mf.BiCGStab(P.op(np.float32), mf.CG_JACOBI, dinv),
                lambda t: laplace_reference(P, "jacobi", np.float32, b, t, 10000), P.A, P.dinv, b, np.float32, 1e-4, 2e-4,
                offset_one)
