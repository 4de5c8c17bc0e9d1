"""mfgpu_vqop_set_coefficients, mfgpu_vqop_vmult, mfgpu_vqop_compute_inverse_diagonal, mfgpu_vqop_set_constrained_values
and mfgpu_bicgstab on a VectorQpOperator, on vectors and per-point arrays that sit inside red zones (tests/redzone.py),
16-byte aligned and one element off.  The zones stay untouched, the read-only inputs unchanged, and the results are those
of the reference."""
import numpy as np
import pytest

import pymfgpu as mf
import vqop_reference as vr
from redzone import Zoned
from test_gpu_poisson import close
from test_gpu_vqop import setup
from test_vqop_host import pick

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("offset_one", [False, True])
@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 2), ("hanging", 2, 5), ("hanging", 3, 2), ("ball", 3, 4), ("hanging", 3, 6)])
def test_vqop_calls_stay_inside_their_arrays(kind, dim, p, offset_one):
    s = setup(kind, dim, p)
    iso, ten = ("lam", "mu", "mass"), ("tensor", "mass")
    zx = Zoned(s.x, offset_one=offset_one)
    zc = {k: Zoned(s.f[k], offset_one=offset_one) for k in ("lam", "mu", "tensor", "mass")}
    zy, zt, zd = (Zoned(s.n, offset_one=offset_one) for _ in range(3))
    q = mf.VectorQpOperator(s.it, mf.VQOP_ISOTROPIC | mf.VQOP_MASS)
    q.set_coefficients(**{k: zc[k].vec for k in iso})
    q.vmult(zy.vec, zx.vec)
    q.inverse_diagonal(zd.vec)
    qt = mf.VectorQpOperator(s.it, mf.VQOP_TENSOR4 | mf.VQOP_MASS)
    qt.set_coefficients(**{k: zc[k].vec for k in ten})
    qt.vmult(zt.vec, zx.vec)
    close(zy.result(), s.ref(iso), 1e-12)
    close(zt.result(), s.ref(ten), 1e-12)
    d = zd.result()
    assert np.all(np.isfinite(d)) and np.all(d[s.con] == 1.0)
    close(d, vr.inverse_diagonal(s.cells, **pick(s.f, *iso)), 1e-12)
    # in place, and the constrained values
    zi = Zoned(s.x, offset_one=offset_one)
    q.vmult(zi.vec, zi.vec)
    np.testing.assert_array_equal(zi.result(), zy.result())
    zv = Zoned(s.x, offset_one=offset_one)
    q.set_constrained_values(zv.vec, -3.5)
    np.testing.assert_array_equal(zv.result(), np.where(s.con, -3.5, s.x))
    for z in [zx] + list(zc.values()):
        z.unchanged()


@pytest.mark.parametrize("offset_one", [False, True])
def test_bicgstab_on_a_vqop_stays_inside_its_vectors(offset_one):
    s = setup("hanging", 3, 2)
    names = ("lam", "mu", "mass")
    q = mf.VectorQpOperator(s.it, mf.VQOP_ISOTROPIC | mf.VQOP_MASS)
    zc = {k: Zoned(s.f[k], offset_one=offset_one) for k in names}
    q.set_coefficients(**{k: z.vec for k, z in zc.items()})
    b = np.where(s.con, 0.0, s.x)
    zb, zd, zs = Zoned(b, offset_one=offset_one), Zoned(s.n, offset_one=offset_one), Zoned(s.n, offset_one=offset_one)
    q.inverse_diagonal(zd.vec)
    solver = mf.BiCGStab(q, mf.CG_JACOBI, zd.vec)
    info = solver.solve(zs.vec, zb.vec, 1e-10 * np.linalg.norm(b), 2000)
    assert info.status == 1
    x = zs.result()
    assert np.linalg.norm(vr.apply(s.cells, x, **pick(s.f, *names)) - b) <= 1e-9 * np.linalg.norm(b)
    zb.unchanged()
    zd.result()
    for z in zc.values():
        z.unchanged()
