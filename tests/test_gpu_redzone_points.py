"""mfgpu_points_evaluate and mfgpu_points_integrate on vectors that sit inside red zones (tests/redzone.py): values,
gradients, rhs, u and weights, 16-byte aligned and one element off.  The zones stay untouched, the read-only inputs
unchanged, and the results are those of the reference.  The points are the setups' of tests/test_gpu_points.py plus one
cell with three work items and a few points outside the mesh (whose zeros are written by the workgroups behind the last
work item)."""
import numpy as np
import pytest

import points_reference as ptr
import pymfgpu as mf
from redzone import Zoned
from test_gpu_points import many_points, setup
from test_gpu_poisson import close

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("offset_one", [False, True])
@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 1), ("hanging", 2, 4), ("hanging", 3, 2), ("cube", 3, 6), ("ball", 3, 2)])
def test_points_calls_stay_inside_their_vectors(kind, dim, p, offset_one):
    s = setup(kind, dim, p)
    cell, xi = many_points(s, 9)
    lost = np.arange(0, len(cell), 97)
    cell = cell.copy()
    cell[lost] = mf.POINT_NOT_FOUND
    pts = mf.Points.in_cells(s.it, cell, xi)
    assert pts.n_not_found == len(lost)
    ref = ptr.PointsRef(s.cells, cell, xi)
    n, nd = len(cell), s.mesh.n_dofs
    w = np.random.default_rng(21).standard_normal(n)
    zu, zw = Zoned(s.u, offset_one=offset_one), Zoned(w, offset_one=offset_one)
    zv, zg, zr = (Zoned(m, offset_one=offset_one) for m in (n, n * dim, nd))
    pts.evaluate(zu.vec, zv.vec, zg.vec)
    pts.integrate(zr.vec, zw.vec)
    vals, grads = ref.evaluate(s.u0)
    v, g, r = zv.result(), zg.result(), zr.result()
    zu.unchanged()
    zw.unchanged()
    close(v, vals, 1e-12)
    close(g, grads.reshape(-1), 1e-12)
    close(r, ref.integrate(w), 1e-12)
    assert np.all(v[lost] == 0.0) and np.all(g.reshape(-1, dim)[lost] == 0.0)
    # each output alone, and integrate without weights
    zv2, zg2, zr2 = (Zoned(m, offset_one=offset_one) for m in (n, n * dim, nd))
    pts.evaluate(zu.vec, values=zv2.vec)
    pts.evaluate(zu.vec, gradients=zg2.vec)
    pts.integrate(zr2.vec)
    np.testing.assert_array_equal(zv2.result(), v)
    np.testing.assert_array_equal(zg2.result(), g)
    close(zr2.result(), ref.integrate(), 1e-12)
    zu.unchanged()
