"""mfgpu_integrator_integrate and the mfgpu_qop_* calls inside the guard mode (pymfgpu.guards, as
tests/test_gpu_guards.py): every device array of the integrator and of the operator sits between guards and starts as NaN
bytes.  No guard is damaged, no NaN from poisoned scratch reaches a result, and the results are bitwise those of a run
outside the mode."""
import functools

import numpy as np
import pytest

import pymfgpu as mf
import qop_reference as qr
from test_gpu_evaluate import integrator
from test_gpu_guards import _integrator_mesh, guard_mode, guarded, max_rel  # noqa: F401 (guard_mode: the module's fixture)
from test_gpu_pmg import dev
from test_gpu_qop import ALL
from test_qop_host import fields
import poisson_reference as pr

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(kind, dim, p):
    mesh = _integrator_mesh(kind, dim, p)
    cells = pr.Cells(mesh)
    rng = np.random.default_rng(dim + p)
    npts = mesh.n_cells * mesh.nd
    v, g, x = rng.standard_normal(npts), rng.standard_normal(npts * dim), rng.standard_normal(mesh.n_dofs)
    co = fields(cells, 3 * dim + p)
    return dict(mesh=mesh, v=v, g=g, x=x, co=co, integrate=qr.integrate(cells, v, g), apply=qr.apply(cells, x, **co),
                transpose=qr.apply(cells, x, transpose=True, **co), dinv=qr.inverse_diagonal(cells, **co),
                reaction=qr.apply(cells, x, reaction=co["reaction"]))


def qop_scenario(run, kind, dim, p):
    R = _reference(kind, dim, p)
    mesh = R["mesh"]
    N = mesh.n_dofs
    it = run.own(integrator(mesh))
    q = run.own(mf.QpOperator(it, ALL))
    v, g, x = (dev(R[k]) for k in ("v", "g", "x"))
    co = {k: dev(a.reshape(-1)) for k, a in R["co"].items()}
    q.set_coefficients(**co)
    # a reaction-only operator on an integrator without inv_jac on the device
    plain = run.own(integrator(mesh, updatable=False))
    qc = run.own(mf.QpOperator(plain, mf.QOP_REACTION))
    qc.set_coefficients(reaction=co["reaction"])

    def out():
        d = mf.DeviceVector(N)
        d.fill(np.nan)  # every entry is written
        return d

    def call(f):
        def go():
            d = out()
            f(d)
            mf.synchronize()
            return d.to_host()
        return go

    run.twice("integrate", call(lambda d: it.integrate(d, v, g)), R["integrate"], 1e-12, err=max_rel, exact=True)
    run.twice("vmult", call(lambda d: q.vmult(d, x)), R["apply"], 1e-12, err=max_rel, exact=True)
    run.twice("vmult_transpose", call(lambda d: q.vmult(d, x, transpose=True)), R["transpose"], 1e-12, err=max_rel, exact=True)
    run.twice("inverse_diagonal", call(lambda d: q.inverse_diagonal(d)), R["dinv"], 1e-12, err=max_rel, exact=True)
    run.twice("vmult_reaction_only", call(lambda d: qc.vmult(d, x)), R["reaction"], 1e-12, err=max_rel, exact=True)
    run.note("memory", (q.memory_consumption(), qc.memory_consumption()))


@pytest.mark.parametrize("dim,p", [(2, 2), (3, 4)])
@pytest.mark.parametrize("kind", ["cube", "hanging", "ball"])
def test_qop(kind, dim, p):
    guarded(qop_scenario, kind, dim, p)
