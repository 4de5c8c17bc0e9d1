"""Host checks of the numpy Poisson reference (tests/poisson_reference.py), the checker of the GPU integrator.

Measured here (2D, p = 2, levels 0, 1, 2 of poisson_reference.family; L2 error of the CPU solve / of the interpolant):
  cube     0.2077, 0.01465, 0.001732   orders 3.83, 3.08   (interpolant 3.29, 3.00)
  hanging  0.06025, 0.006722, 0.000850 orders 3.16, 2.98   (interpolant 3.30, 3.02)
  ball     0.1309, 0.01466, 0.001991   orders 3.16, 2.88   (interpolant 3.13, 2.88)
Asymptotically p + 1 = 3; the ball (MappingQ1 on a curved boundary) settles just below.  The GPU thresholds of
tests/test_gpu_poisson.py are set from these numbers."""
import numpy as np
import pytest

import poisson_reference as pr

BALL_ORDER_2D_P2 = 2.88


@pytest.mark.parametrize("kind,dim,p,level", [("cube", 2, 2, 0), ("cube", 3, 1, 0), ("hanging", 2, 2, 0),
                                              ("hanging", 3, 2, 0), ("ball", 2, 2, 1), ("ball", 3, 2, 0)])
def test_volume_is_sum_of_jxw(kind, dim, p, level):
    c = pr.Cells(pr.family(kind, dim, p, level))
    assert abs(c.jxw_e.sum() - c.od.JxW.sum()) <= 1e-13 * c.od.JxW.sum()


@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 1), ("cube", 2, 3), ("cube", 3, 2), ("hanging", 2, 2),
                                        ("hanging", 3, 2), ("hanging", 2, 4)])
def test_qp_polynomial_is_reproduced(kind, dim, p):
    c = pr.Cells(pr.family(kind, dim, p, 0))
    coef = np.random.default_rng(p).standard_normal((p + 1,) * dim)

    def poly(x):
        v = 0.0
        for idx in np.ndindex(*coef.shape):
            v = v + coef[idx] * np.prod([x[..., d] ** idx[d] for d in range(dim)], axis=0)
        return v

    l2, _ = c.l2_error(c.interpolant(poly), exact=poly(c.xe))
    assert l2 <= 1e-12


@pytest.mark.parametrize("kind,min_order", [("cube", 2.9), ("hanging", 2.9), ("ball", BALL_ORDER_2D_P2 - 0.05)])
def test_interpolation_error_order(kind, min_order):
    errs = []
    for level in range(3):
        c = pr.Cells(pr.family(kind, 2, 2, level))
        errs.append(c.l2_error(c.interpolant())[0])
    assert pr.orders(errs)[-1] >= min_order, errs


@pytest.mark.parametrize("kind,min_order", [("cube", 2.7), ("hanging", 2.7), ("ball", BALL_ORDER_2D_P2 - 0.05)])
def test_cpu_solve_converges(kind, min_order):
    errs = []
    for level in range(3):
        c = pr.Cells(pr.family(kind, 2, 2, level))
        errs.append(c.solve()[1])
    assert pr.orders(errs)[-1] >= min_order, errs


def test_right_hand_side_is_minus_div_a_grad_u():
    """RightHandSide = -div(a grad u), checked by central differences"""
    x = np.random.default_rng(1).uniform(-0.9, 0.9, (20, 3))
    h = 1e-4

    def flux(y, d):
        a = 1.0 / (0.05 + 2.0 * np.sum(y * y, axis=-1))
        return a * pr.solution_gradient(y)[..., d]

    div = sum((flux(x + h * np.eye(3)[d], d) - flux(x - h * np.eye(3)[d], d)) / (2 * h) for d in range(3))
    np.testing.assert_allclose(pr.right_hand_side(x), -div, rtol=1e-6, atol=1e-6)
