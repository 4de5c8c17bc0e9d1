"""Host side of the V-cycle object (no GPU): the Cholesky inverse behind the dense coarse solve, mfgpu_spd_inverse, and the
argument checks of mfgpu_vcycle_create that need no device.

The level-0 matrices are the oracle's (tests/mg_reference.py) of mg.Hierarchy(2,2,3), (2,4,3) and (3,2,4): n0 = 9, 25, 27
with condition numbers 4.2, 26.7 and 6.2, plus a seeded 343 x 343 SPD matrix (the size of the 3D p = 6 coarse level).
Bound: max |inv A - I| <= 1e-10.  A backward-stable inverse leaves about cond * n * 2^-53, 1e-14 here, so the bound is four
orders above rounding and cannot hide a wrong factorisation, whose error is of order one."""
import ctypes as C

import numpy as np
import pytest

import mg_reference as mg
import pymfgpu as mf


def check_inverse(A):
    n = A.shape[0]
    inv = mf.spd_inverse(A)
    err = np.abs(inv @ A - np.eye(n)).max()
    print(f"n = {n}, cond = {np.linalg.cond(A):.1f}: max |inv A - I| = {err:.2e}")
    assert err <= 1e-10
    np.testing.assert_array_equal(inv, inv.T)  # the upper triangle is the mirror of the lower
    # only the lower triangle is read
    B = np.tril(A) + np.triu(np.full_like(A, 7.0), 1)
    np.testing.assert_array_equal(mf.spd_inverse(B), inv)


@pytest.mark.parametrize("dim,p,n_ref,n0", [(2, 2, 3, 9), (2, 4, 3, 25), (3, 2, 4, 27)])
def test_spd_inverse_of_the_level_0_matrices(dim, p, n_ref, n0):
    H = mg.Hierarchy(dim, p, n_ref, matrices=False)
    from oracle import mf_oracle as o

    A = o.assemble(H.odc[0]).toarray()
    assert A.shape == (n0, n0)
    check_inverse(A)


def test_spd_inverse_343():
    rng = np.random.default_rng(343)
    Q = rng.standard_normal((343, 343))
    check_inverse(Q @ Q.T / 343 + np.eye(343))


def test_spd_inverse_refuses_an_indefinite_matrix():
    A = np.diag(np.arange(1.0, 8.0))
    A[3, 3] = -1.0
    rc, _ = mf.spd_inverse(A, check=False)
    assert rc == mf.EINVAL
    rc, _ = mf.spd_inverse(np.zeros((3, 3)), check=False)
    assert rc == mf.EINVAL
    a = np.eye(2)
    assert mf.lib().mfgpu_spd_inverse(2, None, a.ctypes.data) == mf.EINVAL
    assert mf.lib().mfgpu_spd_inverse(2, a.ctypes.data, a.ctypes.data) == mf.EINVAL  # in place
    assert mf.spd_inverse(np.array([[4.0]]))[0, 0] == 0.25


def test_vcycle_create_refuses_null_and_inconsistent_descriptions():
    L = mf.lib()
    out = C.c_void_p()
    lev = (mf.VCycleLevelDesc * 2)()

    def desc(**kw):
        d = mf.VCycleDesc()
        d.n_levels, d.levels, d.active_type, d.n_active = 1, lev, mf.F64, 9
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert L.mfgpu_vcycle_create(None, C.byref(out)) == mf.EINVAL
    assert L.mfgpu_vcycle_create(C.byref(desc()), None) == mf.EINVAL
    for d in [desc(n_levels=0), desc(levels=None), desc(active_type=2), desc(coarse=3), desc(smoothing_range=1.0),
              desc(smoothing_range=-2.0), desc(coarse_tolerance=-1.0), desc(), desc(n_levels=2)]:  # the last two: no op
        assert L.mfgpu_vcycle_create(C.byref(d), C.byref(out)) == mf.EINVAL
        assert not out.value
    assert b"operator" in L.mfgpu_last_error()
    with pytest.raises(mf.MfgpuError, match="error -1"):
        mf.VCycle([], mf.F64, 0)
    with pytest.raises(mf.MfgpuError, match="error -1"):
        mf.VCycle([{"op": None}], mf.F64, 9)
    assert L.mfgpu_vcycle_apply(None, None, None, None) == mf.EINVAL
    assert L.mfgpu_vcycle_lambda_max(None, None) == mf.EINVAL
    assert L.mfgpu_vcycle_memory_consumption(None) == 0
    L.mfgpu_vcycle_destroy(None)
    assert L.mfgpu_cg_set_vcycle(None, None) == mf.EINVAL
    assert L.mfgpu_estimate_lambda_max(None, None, 15, None) == mf.EINVAL
    assert L.mfgpu_cg_begin_relative(None, None, None, 1e-3, 10, None) == mf.EINVAL
    assert L.mfgpu_transfer_prolongate_add(None, None, None, None) == mf.EINVAL
    assert L.mfgpu_vec_residual(None, None, None, 4, mf.F64, None) == mf.EINVAL
    assert L.mfgpu_vec_residual(None, None, None, 4, 2, None) == mf.EINVAL
