"""The host side of the refresh calls (include/mfgpu.h): the two workspace-size functions against
their documented formulas, the layout of the structs the callers copy out, and the argument errors that are found before
anything touches a device."""
import ctypes as C

import pytest

import pymfgpu as mf

F64, F32 = mf.F64, mf.F32


def round16(b):
    return (b + 15) // 16 * 16


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 27, 343, 4097, 1 << 20, (1 << 32) - 1])
def test_eig_workspace_bytes(n):
    """the 64-byte state block, 2 * 2048 doubles of partial sums, two work vectors each rounded up to 16 bytes"""
    for nt, es in ((F64, 8), (F32, 4)):
        assert mf.eig_workspace_bytes(n, nt) == 64 + 2 * 2048 * 8 + 2 * round16(n * es)
        assert mf.eig_workspace_bytes(n, nt) % 16 == 0
    assert mf.eig_workspace_bytes(n, 7) == 0  # an unknown number type
    assert (mf.EIG_STATE_BYTES, mf.EIG_PARTIAL_BYTES) == (64, 2 * 2048 * 8)


@pytest.mark.parametrize("n", [0, 1, 2, 9, 343, 512, 513, 65536])
def test_spd_inverse_workspace_bytes(n):
    """L and L^-1, n * n doubles each"""
    assert mf.spd_inverse_workspace_bytes(n) == 2 * n * n * 8


def test_struct_layouts():
    assert C.sizeof(mf.EigResult) == 24 <= mf.EIG_STATE_BYTES
    assert (mf.EigResult.lambda_max.offset, mf.EigResult.estimate.offset, mf.EigResult.steps.offset,
            mf.EigResult.status.offset) == (0, 8, 16, 20)
    assert C.sizeof(mf.VCycleRefreshInfo) == 16
    assert mf.SPD_INVERSE_DEVICE_MAX == 512 <= mf.VCYCLE_DENSE_MAX


def test_argument_errors_without_a_device():
    """every one of these returns before its first HIP call; the addresses are never read"""
    L = mf.lib()
    p = 4096  # a non-null, 16-byte aligned stand-in for a device address
    EINVAL = mf.EINVAL
    # the device inverse: n == 0, n above the cap, null pointers, short rows, overlapping ranges
    assert mf.spd_inverse_enqueue(0, p, 0, 2 * p, 0, 3 * p, 4 * p, check=False) == EINVAL
    assert mf.spd_inverse_enqueue(513, p, 513, 1 << 30, 514, 1 << 31, 16, check=False) == EINVAL
    assert "MFGPU_SPD_INVERSE_DEVICE_MAX" in L.mfgpu_last_error().decode()
    for hole in range(4):
        args = [p, 1 << 20, 1 << 21, 16]
        args[hole] = None
        assert mf.spd_inverse_enqueue(4, args[0], 4, args[1], 4, args[2], args[3], check=False) == EINVAL
    assert mf.spd_inverse_enqueue(4, p, 3, 1 << 20, 4, 1 << 21, 16, check=False) == EINVAL  # lda < n
    assert mf.spd_inverse_enqueue(4, p, 4, 1 << 20, 3, 1 << 21, 16, check=False) == EINVAL  # ld < n
    assert mf.spd_inverse_enqueue(4, p, 4, p + 64, 4, 1 << 21, 16, check=False) == EINVAL   # inv inside a
    assert mf.spd_inverse_enqueue(4, p, 4, 1 << 20, 4, p + 8, 16, check=False) == EINVAL    # workspace inside a
    assert mf.spd_inverse_enqueue(4, p, 4, 1 << 20, 4, (1 << 21) + 4, 16, check=False) == EINVAL  # misaligned workspace
    # the device power iteration
    assert mf.estimate_lambda_max_enqueue(None, p, 15, 10, p, check=False) == EINVAL
    assert "null" in L.mfgpu_last_error().decode()
    # the Chebyshev scalars and the two sweeps
    assert mf.chebyshev_scalars_dev(0, p, 15.0, p, check=False) == EINVAL
    assert mf.chebyshev_scalars_dev(5, p, 1.0, p, check=False) == EINVAL
    assert mf.chebyshev_scalars_dev(5, p, float("nan"), p, check=False) == EINVAL
    assert mf.chebyshev_scalars_dev(5, None, 15.0, p, check=False) == EINVAL
    assert mf.chebyshev_scalars_dev(5, p, 15.0, None, check=False) == EINVAL
    v = [p * k for k in range(1, 7)]
    assert mf.chebyshev_start_dev(v[0], v[1], v[2], v[3], None, v[4], None, 1, 8, F64, check=False) == EINVAL
    assert mf.chebyshev_start_dev(v[0], v[1], v[2], v[3], None, v[4], v[5] + 4, 1, 8, F64, check=False) == EINVAL
    assert mf.chebyshev_start_dev(v[0], v[1], v[2], v[3], None, v[4], v[5], 1, 8, 2, check=False) == EINVAL
    assert mf.chebyshev_start_dev(v[0], v[0], v[2], v[3], None, v[4], v[5], 1, 8, F32, check=False) == EINVAL
    assert mf.chebyshev_start_dev(v[0], v[1], v[2], v[3], None, v[4], v[5], 1, 0, F32, check=False) == mf.OK  # n == 0
    assert mf.chebyshev_update_dev(v[0], v[1], v[2], v[3], v[4], None, 8, F64, check=False) == EINVAL
    assert mf.chebyshev_update_dev(v[0], v[1], v[2], v[2], v[4], v[5], 8, F64, check=False) == EINVAL
    assert mf.chebyshev_update_dev(v[0], v[1], v[2], v[3], v[4], v[5], 0, F64, check=False) == mf.OK
    # the V-cycle
    assert L.mfgpu_vcycle_refresh(None, 0, None) == EINVAL
    assert L.mfgpu_vcycle_refresh_status(None, None, C.byref(mf.VCycleRefreshInfo())) == EINVAL
    lam, steps = C.c_double(), C.c_uint32()
    assert L.mfgpu_estimate_lambda_max_steps(None, p, 15, C.byref(lam), C.byref(steps)) == EINVAL
