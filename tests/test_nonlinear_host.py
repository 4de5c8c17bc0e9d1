"""Host checks of tests/nonlinear_reference.py, the checker of mfgpu_integrator_evaluate, the coefficient updates and the
nonlinear driver; and of the new ABI's host-visible part.

Measured here with the direct solve (Picard steps to a relative update of 1e-12, max nodal error against u*):
  2D p=2 n=8: 19 steps, 7.4e-3    2D p=2 n=16: 16 steps, 3.0e-4    2D p=4 n=8: 16 steps, 2.6e-5    3D p=2 n=4: 27 steps
The update norm falls by 5-7x per step."""
import ctypes as C

import numpy as np
import pytest

import nonlinear_reference as nr
import poisson_reference as pr
import pymfgpu as mf


def _poly(dim, p, seed):
    coef = np.random.default_rng(seed).standard_normal((p + 1,) * dim)

    def value(x):
        v = 0.0
        for idx in np.ndindex(*coef.shape):
            v = v + coef[idx] * np.prod([x[..., d] ** idx[d] for d in range(dim)], axis=0)
        return v

    def gradient(x):
        g = []
        for k in range(dim):
            v = 0.0
            for idx in np.ndindex(*coef.shape):
                if idx[k] == 0:
                    continue
                v = v + coef[idx] * idx[k] * np.prod([x[..., d] ** (idx[d] - (d == k)) for d in range(dim)], axis=0)
            g.append(v + np.zeros(x.shape[:-1]))
        return np.stack(g, axis=-1)

    return value, gradient


@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 1), ("cube", 2, 3), ("cube", 3, 2), ("hanging", 2, 2),
                                        ("hanging", 3, 2), ("hanging", 2, 4)])
def test_evaluate_reproduces_polynomial(kind, dim, p):
    """tensor-product polynomials of degree <= p per direction are in the space on affine cells, hanging nodes included"""
    c = pr.Cells(pr.family(kind, dim, p, 0))
    value, gradient = _poly(dim, p, p)
    vals, grads = nr.evaluate(c, c.interpolant(value))
    scale = np.abs(value(c.qpts)).max()
    assert np.abs(vals - value(c.qpts)).max() <= 1e-12 * scale
    assert np.abs(grads - gradient(c.qpts)).max() <= 1e-12 * np.abs(gradient(c.qpts)).max()


@pytest.mark.parametrize("dim", [2, 3])
def test_evaluate_reproduces_linear_on_ball(dim):
    """MappingQ1 cells of the ball are not affine: the space holds the polynomials of degree <= 1 in x"""
    c = pr.Cells(pr.family("ball", dim, 2, 0))
    w = np.random.default_rng(dim).standard_normal(dim)
    vals, grads = nr.evaluate(c, c.interpolant(lambda x: 0.3 + x @ w))
    assert np.abs(vals - (0.3 + c.qpts @ w)).max() <= 1e-12
    assert np.abs(grads - w).max() <= 1e-12


def test_load_is_minus_div_a_grad_u():
    """f = -div((1 + u^2) grad u), checked by central differences"""
    x = np.random.default_rng(1).uniform(-0.9, 0.9, (20, 3))
    h = 1e-4

    def flux(y, d):
        return (1.0 + pr.solution(y) ** 2) * pr.solution_gradient(y)[..., d]

    div = sum((flux(x + h * np.eye(3)[d], d) - flux(x - h * np.eye(3)[d], d)) / (2 * h) for d in range(3))
    np.testing.assert_allclose(nr.load(x), -div, rtol=1e-6, atol=1e-6)


def test_picard_converges():
    c = pr.Cells(mf.Mesh.uniform(2, 2, 8))
    u, hist = nr.picard(c, tol=1e-12)
    print(len(hist), hist)
    assert hist[-1] <= 1e-12 and len(hist) <= 25
    assert all(b < 0.5 * a for a, b in zip(hist[1:], hist[2:]))  # (linear convergence, 5-7x per step)
    assert np.abs(u - pr.solution(c.dof_coords)).max() <= 1e-2


def test_abi_declares_the_update_calls():
    L = mf.lib()
    for s in ("mfgpu_update_coefficients", "mfgpu_level_update_coefficients", "mfgpu_integrator_update_coefficients",
              "mfgpu_integrator_evaluate"):
        assert s in mf.SYMBOLS and hasattr(L, s)
    assert mf.UPDATABLE_COEFFICIENTS == 1 << 10
    assert L.mfgpu_desc_size() == C.sizeof(mf.Desc)


def test_plan_and_renumbering_ignore_the_flag():
    mesh = mf.Mesh.uniform(3, 4, 5)
    base = mf.Plan(mesh.desc, mesh)
    order, bco, new_index = base.cell_order, base.batch_cell_off, mesh.suggest_renumbering()
    mesh.desc.flags |= mf.UPDATABLE_COEFFICIENTS
    flagged = mf.Plan(mesh.desc, mesh)
    np.testing.assert_array_equal(flagged.cell_order, order)
    np.testing.assert_array_equal(flagged.batch_cell_off, bco)
    np.testing.assert_array_equal(flagged.pr_dofs, base.pr_dofs)
    np.testing.assert_array_equal(mesh.suggest_renumbering(), new_index)
