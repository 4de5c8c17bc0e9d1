"""mfgpu_integrator_integrate, mfgpu_qop_set_coefficients, mfgpu_qop_vmult and mfgpu_qop_compute_inverse_diagonal on
vectors and per-point arrays that sit inside red zones (tests/redzone.py), 16-byte aligned and one element off.  The zones
stay untouched, the read-only inputs unchanged, and the results are those of the reference."""
import numpy as np
import pytest

import pymfgpu as mf
import qop_reference as qr
from redzone import Zoned
from test_gpu_poisson import close
from test_gpu_qop import ALL, setup

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("offset_one", [False, True])
@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 2), ("hanging", 2, 5), ("hanging", 3, 2), ("ball", 3, 4), ("hanging", 3, 6)])
def test_qop_calls_stay_inside_their_arrays(kind, dim, p, offset_one):
    s = setup(kind, dim, p)
    rng = np.random.default_rng(31)
    v, g = rng.standard_normal(s.npts), rng.standard_normal(s.npts * dim)
    zv, zg, zx = (Zoned(a, offset_one=offset_one) for a in (v, g, s.x))
    zc = {k: Zoned(a, offset_one=offset_one) for k, a in s.tensor.items()}
    zr, zy, zt, zd = (Zoned(s.n, offset_one=offset_one) for _ in range(4))
    s.it.integrate(zr.vec, zv.vec, zg.vec)
    q = mf.QpOperator(s.it, ALL)
    q.set_coefficients(**{k: z.vec for k, z in zc.items()})
    q.vmult(zy.vec, zx.vec)
    q.vmult(zt.vec, zx.vec, transpose=True)
    q.inverse_diagonal(zd.vec)
    close(zr.result(), qr.integrate(s.cells, v, g), 1e-12)
    close(zy.result(), qr.apply(s.cells, s.x, **s.tensor), 1e-12)
    close(zt.result(), qr.apply(s.cells, s.x, transpose=True, **s.tensor), 1e-12)
    d = zd.result()
    assert np.all(np.isfinite(d)) and np.all(d[~s.free] == 1.0)
    close(d, qr.inverse_diagonal(s.cells, **s.tensor), 1e-12)
    for z in [zv, zg, zx] + list(zc.values()):
        z.unchanged()
    # each input of integrate alone
    zr1, zr2 = Zoned(s.n, offset_one=offset_one), Zoned(s.n, offset_one=offset_one)
    s.it.integrate(zr1.vec, values=zv.vec)
    s.it.integrate(zr2.vec, gradients=zg.vec)
    close(zr1.result(), qr.integrate(s.cells, v, None), 1e-12)
    close(zr2.result(), qr.integrate(s.cells, None, g), 1e-12)
