"""BiCGStab with the library's own device arrays guarded and poisoned (mfgpu_debug_guard_*), by the scheme of
tests/test_gpu_guards.py: the scenario runs once with the mode off and once inside it; no guard byte may change, no NaN
may come out of the poisoned work vectors, partial sums or state block, the two runs agree bit for bit, and destroying
the handles leaves no array registered."""
import numpy as np
import pytest

import pymfgpu as mf
from test_bicgstab_host import CASES, qop_problem
from test_gpu_bicgstab import ITERATE_TOL, Device
from test_gpu_cg import dv
from test_gpu_guards import guard_mode, guarded  # noqa: F401  (guard_mode: the module's autouse fixture)

pytestmark = pytest.mark.gpu


def bicgstab_scenario(run, prec):
    kind, dim, p, cset, _ = CASES[1]
    P = qop_problem(kind, dim, p, cset)
    D = Device(P)  # integrator, operator and inverse diagonal allocated inside the mode
    solver = D.solver(prec)
    run.own(D.it, D.q, solver)
    b = P.rhs()
    db = dv(b)
    want6 = [h for _, h in zip(range(7), P.reference(prec, np.float64, b, 0.0, 1000))][6]
    assert want6[0] == 6

    def six_iterates():
        x = mf.DeviceVector(P.N)
        x.fill(np.nan)  # begin writes every entry
        solver.begin(x, db, 0.0, 1000)
        solver.iterate(6)
        info = solver.status()
        assert (info.iterations, info.status) == (6, 0)
        return x.to_host()

    run.twice("six_iterates", six_iterates, want6[3], ITERATE_TOL[np.float64], exact=True)
    tolerance = 1e-10 * np.linalg.norm(b)
    ref_it = list(P.reference(prec, np.float64, b, tolerance, 10000))[-1][0]

    def solve():
        x = mf.DeviceVector(P.N)
        x.fill(np.nan)
        info = solver.solve(x, db, tolerance, 10000, check_every=5)
        assert info.status == 1 and 0 < info.iterations <= 2 * ref_it and info.residual <= tolerance
        run.note("iterations", int(info.iterations))
        return x.to_host()

    def true_residual(got, want):
        """the solve's own bound (tests/test_gpu_bicgstab.py): |b - A x| / |b|; `want` is not used"""
        return float(np.linalg.norm(b - P.A @ got) / np.linalg.norm(b))

    run.twice("solve", solve, None, 2e-10, err=true_residual, exact=True)
    run.note("memory_consumption", solver.memory_consumption())


@pytest.mark.parametrize("prec", ["none", "jacobi"])
def test_bicgstab(prec):
    guarded(bicgstab_scenario, prec)
