"""Host side of the device-resident CG (mfgpu_cg, include/mfgpu.h): the scalars of the Chebyshev sweep against the
recurrence of PreconditionChebyshev::run_fused (host/mfgpu_shim_mg.h) restated in numpy, and the argument checks that
need no device."""
import ctypes as C

import numpy as np
import pytest

import cg_reference as ref
import pymfgpu as mf


@pytest.mark.parametrize("degree", [1, 2, 5])
@pytest.mark.parametrize("lambda_max,smoothing_range", [(2.3, 15.0), (1.9871, 30.0), (417.0, 1.5)])
def test_chebyshev_scalars_match_the_recurrence(degree, lambda_max, smoothing_range):
    got = mf.cg_chebyshev_scalars(degree, lambda_max, smoothing_range)
    want = ref.chebyshev_scalars(degree, lambda_max, smoothing_range)
    assert got.shape == (2 * degree - 1,)
    assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max()
    np.testing.assert_allclose(got, want, rtol=1e-15, atol=0)


def test_chebyshev_scalars_first_entry_and_fixed_point():
    # f[0] = 1 / theta with theta the centre of [lambda_max / range, lambda_max]; rho_k decreases to sigma - sqrt(sigma^2 - 1)
    f = mf.cg_chebyshev_scalars(40, 3.0, 15.0)
    theta, delta = 0.5 * (3.0 + 0.2), 0.5 * (3.0 - 0.2)
    assert abs(f[0] - 1.0 / theta) <= 1e-15 / theta
    sigma = theta / delta
    rho = sigma - np.sqrt(sigma * sigma - 1.0)
    assert abs(f[-2] - rho * rho) <= 1e-12 and abs(f[-1] - 2.0 * rho / delta) <= 1e-12


@pytest.mark.parametrize("degree,lambda_max,smoothing_range", [(0, 2.0, 15.0), (3, 0.0, 15.0), (3, -1.0, 15.0),
                                                               (3, 2.0, 1.0), (3, 2.0, 0.5), (3, float("nan"), 15.0)])
def test_chebyshev_scalars_rejects_bad_arguments(degree, lambda_max, smoothing_range):
    out = (C.c_double * 8)(*([7.0] * 8))
    assert mf.lib().mfgpu_cg_chebyshev_scalars(degree, lambda_max, smoothing_range, out) == mf.EINVAL
    assert list(out) == [7.0] * 8  # nothing written
    with pytest.raises(mf.MfgpuError, match="error -1"):
        mf.cg_chebyshev_scalars(degree, lambda_max, smoothing_range)


def test_null_arguments():
    L = mf.lib()
    assert L.mfgpu_cg_chebyshev_scalars(3, 2.0, 15.0, None) == mf.EINVAL
    h = C.c_void_p()
    assert L.mfgpu_cg_create(None, mf.CG_NONE, None, 0, 0.0, 0.0, C.byref(h)) == mf.EINVAL
    assert not h.value
    info = mf.CGInfo()
    assert L.mfgpu_cg_set_callback(None, mf.CG_CALLBACK_TYPE(lambda *a: 0), None) == mf.EINVAL
    assert L.mfgpu_cg_begin(None, None, None, 1e-10, 10, None) == mf.EINVAL
    assert L.mfgpu_cg_iterate(None, 1, None) == mf.EINVAL
    assert L.mfgpu_cg_status(None, None, C.byref(info)) == mf.EINVAL
    assert L.mfgpu_cg_solve(None, None, None, 1e-10, 10, 1, None, C.byref(info)) == mf.EINVAL
    assert L.mfgpu_cg_memory_consumption(None) == 0
    L.mfgpu_cg_destroy(None)


def test_info_mirror_matches_the_header():
    assert C.sizeof(mf.CGInfo) == 24
    assert (mf.CG_NONE, mf.CG_JACOBI, mf.CG_CHEBYSHEV, mf.CG_CALLBACK) == (0, 1, 2, 3)
    assert all(hasattr(mf.lib(), s) for s in mf.SYMBOLS if s.startswith("mfgpu_cg_"))
