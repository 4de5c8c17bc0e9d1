"""mfgpu_integrator_evaluate: a finite element field and its real-space gradient at the quadrature points
(evaluate_cell_kernel, the read_dof_values + evaluate + get_value / get_gradient half of FEEvaluationGpu) against the
numpy restatement in tests/nonlinear_reference.py, on the level-0 members of poisson_reference.family.  The field is a
seeded random dof vector, nonzero on the constrained dofs (they are read); the dofs no cell references are NaN (they are
not).  Tolerance: 1e-12 relative to the largest reference entry."""
import numpy as np
import pytest

import nonlinear_reference as nr
import poisson_reference as pr
import pymfgpu as mf
from test_gpu_poisson import close, dv

pytestmark = pytest.mark.gpu

CASES = [("cube", 2, 1), ("cube", 2, 3), ("cube", 2, 6), ("cube", 3, 2), ("cube", 3, 4), ("cube", 3, 5),
         ("hanging", 2, 2), ("hanging", 2, 4), ("hanging", 3, 2), ("ball", 2, 2), ("ball", 3, 2)]

_cache = {}


def setup(kind, dim, p):
    """(mesh, u, reference values, reference gradients), computed once per case"""
    key = (kind, dim, p)
    if key not in _cache:
        mesh = pr.family(kind, dim, p, 0)
        cells = pr.Cells(mesh)
        u = np.random.default_rng(dim * 10 + p).standard_normal(mesh.n_dofs)
        unread = np.ones(mesh.n_dofs, bool)
        unread[cells.od.loc2glob.reshape(-1)] = False
        assert (kind == "hanging") == bool(unread.any())
        assert np.all(u[cells.od.constrained[~unread[cells.od.constrained]]] != 0.0)
        vals, grads = nr.evaluate(cells, np.where(unread, 0.0, u))
        u[unread] = np.nan
        for a in (u, vals, grads):
            a.setflags(write=False)
        _cache[key] = (mesh, u, vals, grads)
    return _cache[key]


def integrator(mesh, updatable=True):
    flags = mesh.desc.flags
    mesh.desc.flags = (flags | mf.UPDATABLE_COEFFICIENTS) if updatable else (flags & ~mf.UPDATABLE_COEFFICIENTS)
    try:
        return mf.Integrator(mesh.desc, mesh)
    finally:
        mesh.desc.flags = flags


def nan_vector(n):
    v = mf.DeviceVector(n)
    v.fill(np.nan)  # every entry is written
    return v


@pytest.mark.parametrize("kind,dim,p", CASES)
def test_values_and_gradients_match_reference(kind, dim, p):
    mesh, u, vals, grads = setup(kind, dim, p)
    it = integrator(mesh)
    npts = mesh.n_cells * mesh.nd
    v, g = nan_vector(npts), nan_vector(npts * dim)
    it.evaluate(dv(u), v, g)
    mf.synchronize()
    got_v, got_g = v.to_host(), g.to_host()
    close(got_v, vals.reshape(-1), 1e-12)
    close(got_g, grads.reshape(-1), 1e-12)
    # values only, gradients only: the same bits, the other array untouched
    v2, g2 = nan_vector(npts), nan_vector(npts * dim)
    it.evaluate(dv(u), values=v2)
    it.evaluate(dv(u), gradients=g2)
    mf.synchronize()
    np.testing.assert_array_equal(v2.to_host(), got_v)
    np.testing.assert_array_equal(g2.to_host(), got_g)


@pytest.mark.parametrize("kind,dim,p", [("cube", 3, 4), ("hanging", 3, 2), ("ball", 2, 2)])
def test_values_work_without_the_flag_and_gradients_are_refused(kind, dim, p):
    mesh, u, vals, _ = setup(kind, dim, p)
    it = integrator(mesh, updatable=False)
    npts = mesh.n_cells * mesh.nd
    v, g = nan_vector(npts), nan_vector(npts * dim)
    it.evaluate(dv(u), v)
    mf.synchronize()
    close(v.to_host(), vals.reshape(-1), 1e-12)
    with pytest.raises(mf.MfgpuError, match="error -1.*MFGPU_UPDATABLE_COEFFICIENTS"):
        it.evaluate(dv(u), v, g)
    with pytest.raises(mf.MfgpuError, match="error -1.*MFGPU_UPDATABLE_COEFFICIENTS"):
        it.evaluate(dv(u), gradients=g)
    with pytest.raises(mf.MfgpuError, match="error -1.*both NULL"):
        it.evaluate(dv(u))
    mf.synchronize()
    assert np.all(np.isnan(g.to_host()))  # a refused call writes nothing


def test_evaluate_reproduces_polynomial_on_hanging_mesh():
    """known answer without the reference: a tensor polynomial of degree p and its gradient, hanging nodes included"""
    from test_nonlinear_host import _poly
    dim, p = 3, 2
    mesh = pr.family("hanging", dim, p, 0)
    value, gradient = _poly(dim, p, 3)
    x = mesh.arrays()["quadrature_points"].reshape(-1, dim)
    npts = len(x)
    v, g = nan_vector(npts), nan_vector(npts * dim)
    integrator(mesh).evaluate(dv(value(mesh.dof_coords())), v, g)
    mf.synchronize()
    close(v.to_host(), value(x), 1e-12)
    close(g.to_host(), gradient(x).reshape(-1), 1e-12)
