"""Host checks of tests/qop_reference.py, the checker of mfgpu_integrator_integrate and mfgpu_qop_*, and of the part of
the new ABI that needs no device.

Newton against Picard, measured here with the sparse direct solve to a relative update of 1e-10 (NEWTON_STEPS /
PICARD_STEPS below): Newton's update norm falls quadratically once it is below about 1e-2, Picard's by 5-7x per step."""
import ctypes as C
import itertools

import numpy as np
import pytest

import helmholtz_reference as hr
import nonlinear_reference as nr
import poisson_reference as pr
import pymfgpu as mf
import qop_reference as qr
from oracle import mf_oracle as o

# (dim, p, n) -> steps to |u_{k+1} - u_k| / |u_{k+1}| <= 1e-10 on Mesh.uniform(dim, p, n), direct solves
NEWTON_MESHES = [(2, 2, 8), (2, 4, 8), (3, 2, 4)]
NEWTON_STEPS = {(2, 2, 8): 7, (2, 4, 8): 7, (3, 2, 4): 7}
PICARD_STEPS = {(2, 2, 8): 16, (2, 4, 8): 14, (3, 2, 4): 22}

_cells = {}


def cells_of(kind, dim, p):
    if (kind, dim, p) not in _cells:
        _cells[(kind, dim, p)] = pr.Cells(pr.family(kind, dim, p, 0))
    return _cells[(kind, dim, p)]


def fields(cells, seed, tensor=True):
    """seeded coefficients: diffusion (non-symmetric tensor or positive scalar), convection, flux, reaction"""
    od, dim = cells.od, cells.dim
    rng = np.random.default_rng(seed)
    shape = (od.n_cells, od.nd)
    D = rng.standard_normal(shape + (dim, dim)) + 3.0 * np.eye(dim) if tensor else rng.uniform(0.5, 2.0, shape)
    return {"diffusion": D, "convection": rng.standard_normal(shape + (dim,)), "flux": rng.standard_normal(shape + (dim,)),
            "reaction": rng.uniform(0.5, 2.0, shape)}


MESHES = [("cube", 2, 2), ("hanging", 2, 3), ("ball", 2, 2), ("hanging", 3, 2), ("ball", 3, 1)]


@pytest.mark.parametrize("kind,dim,p", MESHES)
def test_integrate_is_the_adjoint_of_evaluate(kind, dim, p):
    c = cells_of(kind, dim, p)
    od = c.od
    rng = np.random.default_rng(p)
    v, g = rng.standard_normal((od.n_cells, od.nd)), rng.standard_normal((od.n_cells, od.nd, dim))
    u = rng.standard_normal(od.n_dofs)
    u[od.constrained] = 0.0
    val, grad = nr.evaluate(c, u)
    w = od.JxW.astype(np.float64)
    rhs = np.sum(w * (v * val + np.sum(g * grad, axis=-1)))
    lhs = qr.integrate(c, v, g) @ u
    assert abs(lhs - rhs) <= 1e-12 * np.sum(w * (np.abs(v * val) + np.abs(np.sum(g * grad, axis=-1))))
    assert np.all(qr.integrate(c, v, g)[od.constrained] == 0.0)
    np.testing.assert_allclose(qr.integrate(c, v, None) + qr.integrate(c, None, g), qr.integrate(c, v, g), rtol=0,
                               atol=1e-13 * np.abs(qr.integrate(c, v, g)).max())


@pytest.mark.parametrize("kind,dim,p", MESHES)
def test_scalar_diffusion_and_reaction_reproduce_the_existing_references(kind, dim, p):
    c = cells_of(kind, dim, p)
    od = c.od
    a, m = od.coefficient.astype(np.float64), fields(c, 1)["reaction"]
    ref = hr.assemble(od, m)
    got = qr.assemble(c, diffusion=a, reaction=m)
    assert abs(got - ref).max() <= 1e-12 * abs(ref).max()
    ref = o.assemble(od)
    got = qr.assemble(c, diffusion=a)
    assert abs(got - ref).max() <= 1e-12 * abs(ref).max()
    x = np.random.default_rng(2).standard_normal(od.n_dofs)
    y = qr.apply(c, x, diffusion=a)
    assert np.linalg.norm(y - ref @ x) <= 1e-12 * np.linalg.norm(y)


def _polynomial(dim, p, seed):
    """deriv(x, orders): the mixed derivative of a seeded tensor polynomial of degree p per direction"""
    coef = np.random.default_rng(seed).standard_normal((p + 1,) * dim)

    def deriv(x, orders):
        out = np.zeros(x.shape[:-1])
        for idx in np.ndindex(*coef.shape):
            term = coef[idx] * np.ones(x.shape[:-1])
            for d in range(dim):
                k, n = orders[d], idx[d]
                if k > n:
                    term = 0.0 * term
                    break
                fall = np.prod([n - j for j in range(k)]) if k else 1.0
                term = term * fall * x[..., d] ** (n - k)
            out = out + term
        return out

    return deriv


@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 2), ("hanging", 2, 3), ("hanging", 3, 2)])
def test_greens_identity(kind, dim, p):
    """Constant D and beta, u an interpolated tensor polynomial of degree p on affine cells: at an interior dof
    (A u)_i = int phi_i (-div(D grad u) + beta . grad u), both sides exact on QGauss(p+1)."""
    mesh = pr.family(kind, dim, p, 0)
    mesh.desc.n_constrained = 0  # every dof free: u is read on the boundary too
    c = pr.Cells(mesh)
    od = c.od
    assert len(od.constrained) == 0
    rng = np.random.default_rng(5)
    D, beta = rng.standard_normal((dim, dim)) + 3.0 * np.eye(dim), rng.standard_normal(dim)
    deriv = _polynomial(dim, p, 7)
    e = np.eye(dim, dtype=int)
    u = deriv(c.dof_coords, [0] * dim)
    strong = np.zeros(c.qpts.shape[:2])
    for k, l in itertools.product(range(dim), repeat=2):
        strong -= D[k, l] * deriv(c.qpts, list(e[k] + e[l]))
    for k in range(dim):
        strong += beta[k] * deriv(c.qpts, list(e[k]))
    shape = (od.n_cells, od.nd)
    got = qr.apply(c, u, diffusion=np.broadcast_to(D, shape + (dim, dim)), convection=np.broadcast_to(beta, shape + (dim,)))
    ref = qr.integrate(c, strong)
    referenced = np.zeros(od.n_dofs, bool)
    referenced[od.loc2glob.reshape(-1)] = True
    interior = referenced & np.all(np.abs(c.dof_coords) < 1.0 - 1e-9, axis=1)
    assert interior.sum() > 0
    assert np.abs(got - ref)[interior].max() <= 1e-11 * np.abs(got).max()


@pytest.mark.parametrize("kind,dim,p", MESHES)
def test_transpose_is_the_matrix_transpose(kind, dim, p):
    c = cells_of(kind, dim, p)
    t = fields(c, 3)
    A = qr.assemble(c, **t)
    x = np.random.default_rng(4).standard_normal(c.od.n_dofs)
    for tr, M in ((False, A), (True, A.T)):
        y = qr.apply(c, x, transpose=tr, **t)
        assert np.linalg.norm(y - M @ x) <= 1e-12 * np.linalg.norm(y)
    # the stated rule: A^T is the operator with D -> D^T and beta <-> gamma
    swapped = qr.assemble(c, diffusion=np.swapaxes(t["diffusion"], -1, -2), convection=t["flux"], flux=t["convection"],
                          reaction=t["reaction"])
    assert abs(swapped - A.T).max() <= 1e-12 * abs(A).max()


@pytest.mark.parametrize("kind,dim,p", MESHES + [("cube", 3, 2), ("hanging", 2, 5)])
def test_cell_diagonal_is_the_diagonal_of_the_assembled_matrix(kind, dim, p):
    c = cells_of(kind, dim, p)
    for t in (fields(c, 8), fields(c, 9, tensor=False), {"convection": fields(c, 8)["convection"]},
              {"diffusion": fields(c, 8)["diffusion"], "flux": fields(c, 8)["flux"]}):
        ref = qr.assemble(c, **t).diagonal()
        got = qr.diagonal(c, **t)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_inverse_diagonal_is_one_on_constrained_and_unreferenced_dofs():
    c = cells_of("hanging", 2, 3)
    od = c.od
    d = qr.inverse_diagonal(c, **fields(c, 6))
    unref = np.ones(od.n_dofs, bool)
    unref[od.loc2glob.reshape(-1)] = False
    assert unref.any() and np.all(d[unref] == 1.0) and np.all(d[od.constrained] == 1.0) and np.all(np.isfinite(d))


@pytest.mark.parametrize("dim,p,n", NEWTON_MESHES)
def test_newton_needs_fewer_steps_than_picard(dim, p, n):
    c = pr.Cells(mf.Mesh.uniform(dim, p, n))
    u, hist = qr.newton(c)
    up, hist_p = nr.picard(c)
    print(f"{dim}D p={p} n={n}: Newton {len(hist)} steps {hist}, Picard {len(hist_p)} steps")
    assert len(hist) == NEWTON_STEPS[(dim, p, n)] and len(hist_p) == PICARD_STEPS[(dim, p, n)]
    assert len(hist) < len(hist_p)
    assert hist[-1] <= 1e-10 and hist[-1] <= 10 * hist[-2] ** 2 + 1e-14  # quadratic at the end
    # both stop at a relative update of 1e-10; Picard's remaining error is that update times its contraction, 5-7x per step
    assert np.linalg.norm(u - up) <= 1e-10 * np.linalg.norm(u)


def test_newton_residual_vanishes_at_the_solution():
    c = pr.Cells(mf.Mesh.uniform(2, 2, 8))
    u, _ = qr.newton(c)
    R, _ = qr.newton_terms(c, u)
    R0, _ = qr.newton_terms(c, c.lift())
    assert np.linalg.norm(R) <= 1e-12 * np.linalg.norm(R0)


def test_argument_errors_without_a_device():
    L = mf.lib()
    for s in ("mfgpu_integrator_integrate", "mfgpu_qop_create", "mfgpu_qop_set_coefficients", "mfgpu_qop_vmult",
              "mfgpu_qop_compute_inverse_diagonal", "mfgpu_qop_memory_consumption", "mfgpu_qop_destroy"):
        assert s in mf.SYMBOLS and hasattr(L, s)
    h = C.c_void_p()
    assert L.mfgpu_qop_create(None, mf.QOP_REACTION, C.byref(h)) == mf.EINVAL and not h.value
    assert L.mfgpu_qop_create(None, 0, None) == mf.EINVAL
    assert L.mfgpu_integrator_integrate(None, None, None, None, None) == mf.EINVAL
    co = mf.QopCoefficients()
    assert L.mfgpu_qop_set_coefficients(None, C.byref(co), None) == mf.EINVAL
    assert L.mfgpu_qop_vmult(None, None, None, 0, None) == mf.EINVAL
    assert L.mfgpu_qop_compute_inverse_diagonal(None, None, None) == mf.EINVAL
    assert L.mfgpu_qop_memory_consumption(None) == 0
    L.mfgpu_qop_destroy(None)
    assert (mf.QOP_DIFFUSION_SCALAR, mf.QOP_DIFFUSION_TENSOR, mf.QOP_CONVECTION, mf.QOP_FLUX, mf.QOP_REACTION,
            mf.QOP_TRANSPOSE) == (1, 2, 4, 8, 16, 1)
    assert C.sizeof(mf.QopCoefficients) == 4 * C.sizeof(C.c_void_p)
    assert L.mfgpu_desc_size() == C.sizeof(mf.Desc)
