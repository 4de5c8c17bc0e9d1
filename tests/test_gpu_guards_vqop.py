"""The mfgpu_vqop_* calls inside the guard mode (pymfgpu.guards, as tests/test_gpu_guards_qop.py): every device array of
the integrator and of the operator -- the folded coefficients, its constraint flags and its dim - 1 local-vector
buffers -- sits between guards and starts as NaN bytes.  No guard is damaged, no NaN from poisoned scratch reaches a
result, and the results are bitwise those of a run outside the mode."""
import functools

import numpy as np
import pytest

import poisson_reference as pr
import pymfgpu as mf
import vqop_reference as vr
from test_gpu_evaluate import integrator
from test_gpu_guards import _integrator_mesh, guard_mode, guarded, max_rel  # noqa: F401 (guard_mode: the module's fixture)
from test_gpu_pmg import dev
from test_vqop_host import pick, vfields

pytestmark = pytest.mark.gpu

ISO, TEN = ("lam", "mu", "mass"), ("tensor",)


@functools.lru_cache(maxsize=None)
def _reference(kind, dim, p):
    mesh = _integrator_mesh(kind, dim, p)
    cells = pr.Cells(mesh)
    n = dim * mesh.n_dofs
    x = np.random.default_rng(dim + p).standard_normal(n)
    co = vfields(cells, 3 * dim + p)
    con = vr.constrained_flags(cells)
    return dict(mesh=mesh, x=x, co=co, n=n, iso=vr.apply(cells, x, **pick(co, *ISO)),
                ten=vr.apply(cells, x, **pick(co, *TEN)), dinv=vr.inverse_diagonal(cells, **pick(co, *ISO)),
                mass=vr.apply(cells, x, mass=co["mass"]), fixed=np.where(con, -3.5, x))


def vqop_scenario(run, kind, dim, p):
    R = _reference(kind, dim, p)
    mesh, n = R["mesh"], R["n"]
    it = run.own(integrator(mesh))
    x = dev(R["x"])
    co = {k: dev(a.reshape(-1)) for k, a in R["co"].items()}
    q = run.own(mf.VectorQpOperator(it, mf.VQOP_ISOTROPIC | mf.VQOP_MASS))
    q.set_coefficients(**pick(co, *ISO))
    qt = run.own(mf.VectorQpOperator(it, mf.VQOP_TENSOR4))
    qt.set_coefficients(**pick(co, *TEN))
    # a mass-only operator on an integrator without inv_jac on the device
    plain = run.own(integrator(mesh, updatable=False))
    qm = run.own(mf.VectorQpOperator(plain, mf.VQOP_MASS))
    qm.set_coefficients(mass=co["mass"])

    def call(f):
        def go():
            d = mf.DeviceVector(n)
            d.fill(np.nan)  # every entry is written
            f(d)
            mf.synchronize()
            return d.to_host()
        return go

    def constrained():
        v = dev(R["x"])
        q.set_constrained_values(v, -3.5)
        mf.synchronize()
        return v.to_host()

    run.twice("vmult_isotropic_mass", call(lambda d: q.vmult(d, x)), R["iso"], 1e-12, err=max_rel, exact=True)
    run.twice("vmult_tensor4", call(lambda d: qt.vmult(d, x)), R["ten"], 1e-12, err=max_rel, exact=True)
    run.twice("inverse_diagonal", call(lambda d: q.inverse_diagonal(d)), R["dinv"], 1e-12, err=max_rel, exact=True)
    run.twice("vmult_mass_only", call(lambda d: qm.vmult(d, x)), R["mass"], 1e-12, err=max_rel, exact=True)
    run.twice("set_constrained_values", constrained, R["fixed"], 0.0, err=max_rel, exact=True)
    run.note("memory", (q.memory_consumption(), qt.memory_consumption(), qm.memory_consumption()))


@pytest.mark.parametrize("dim,p", [(2, 2), (3, 4)])
@pytest.mark.parametrize("kind", ["cube", "hanging", "ball"])
def test_vqop(kind, dim, p):
    guarded(vqop_scenario, kind, dim, p)
