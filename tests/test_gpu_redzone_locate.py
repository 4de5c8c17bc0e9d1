"""mfgpu_locator_locate on vectors that sit inside red zones (tests/redzone.py): x, xi, cell (and the hint, which is the
cell buffer in the second call), 16-byte aligned and one element off.  The zones stay untouched, x unchanged, and the
outputs are those of the call on plain vectors.  The points are the setups' of tests/test_gpu_points.py (in an order that
is not the cell order) plus the dof coordinates and a few points outside the mesh; their number is no multiple of 64, so
the last wave has tail lanes."""
import numpy as np
import pytest

import pymfgpu as mf
from redzone import Zoned
from test_gpu_locate import device_locate
from test_gpu_points import setup

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("offset_one", [False, True])
@pytest.mark.parametrize("kind,dim,p", [(kind, dim, p) for kind in ("hanging", "ball") for dim in (2, 3) for p in (2, 4)])
def test_locate_stays_inside_its_vectors(kind, dim, p, offset_one):
    s = setup(kind, dim, p)
    if not hasattr(s, "loc"):  # (device_locate reads s.loc and s.dim)
        s.loc = mf.Locator(s.it, s.mesh.desc)
    x = np.concatenate([s.x, s.mesh.dof_coords(), [[2.0] * dim, [np.nan] * dim]])
    if len(x) % 64 == 0:
        x = x[:-1]
    n = len(x)
    cell, xi, missing = device_locate(s, x)
    assert missing >= 1 and np.sum(cell != mf.POINT_NOT_FOUND) >= len(s.x)
    zx, zxi = Zoned(x, offset_one=offset_one), Zoned(n * dim, offset_one=offset_one)
    zc, zn = Zoned(n, mf.F32, offset_one=offset_one), Zoned(1, mf.F32, offset_one=offset_one)
    s.loc.locate(zx.vec, zc.vec, zxi.vec, n_not_found=zn.vec)
    np.testing.assert_array_equal(zc.result().view(np.uint32), cell)
    np.testing.assert_array_equal(zxi.result().reshape(n, dim), xi)
    assert int(zn.result().view(np.uint32)[0]) == missing
    zx.unchanged()
    # once more with the cells of the first call as hints, in the cell buffer itself, and no counter
    zxi2 = Zoned(n * dim, offset_one=offset_one)
    s.loc.locate(zx.vec, zc.vec, zxi2.vec, hint=zc.vec)
    np.testing.assert_array_equal(zc.result().view(np.uint32), cell)
    np.testing.assert_array_equal(zxi2.result().reshape(n, dim), xi)
    zx.unchanged()
