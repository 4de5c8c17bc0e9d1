"""Guard mode of the library's device arrays, the part that needs no device: the padding arithmetic
(mfgpu_debug_guard_layout) and the argument checks of the mfgpu_debug_guard_* entry points."""
import ctypes as C

import pytest

import pymfgpu as mf

SIZES = [1, 7, 8, 255, 256, 257, 10**6 + 3]
GUARDS = [256, 32768]


@pytest.mark.parametrize("guard", GUARDS)
@pytest.mark.parametrize("n_bytes", SIZES)
def test_layout(n_bytes, guard):
    total, off = mf.guard_layout(n_bytes, guard)
    assert off % 256 == 0  # the alignment of a bare allocation
    assert off >= guard  # a whole front guard
    back = off + n_bytes  # the back guard begins at the payload's last byte + 1, not rounded up
    assert total == back + guard
    assert total >= guard + n_bytes + guard


def test_layout_rounds_an_odd_guard_up_in_front_only():
    total, off = mf.guard_layout(100, 300)
    assert (off, total) == (512, 512 + 100 + 300)


def test_bad_arguments_fail_loudly():
    L = mf.lib()
    t, o = C.c_size_t(), C.c_size_t()
    assert L.mfgpu_debug_guard_layout(8, 0, C.byref(t), C.byref(o)) == mf.EINVAL
    assert L.mfgpu_debug_guard_layout(8, (1 << 30) + 1, C.byref(t), C.byref(o)) == mf.EINVAL
    assert L.mfgpu_debug_guard_layout(8, 256, None, C.byref(o)) == mf.EINVAL
    assert L.mfgpu_debug_guard_begin(0) == mf.EINVAL
    assert L.mfgpu_debug_guard_begin((1 << 30) + 1) == mf.EINVAL
    assert L.mfgpu_debug_guard_check(None, None, None, 0) == mf.EINVAL
    p, z = C.c_int(), C.c_int()
    d = C.c_uint64()
    assert L.mfgpu_debug_guard_selftest(C.byref(d), None, 0, C.byref(p), C.byref(z)) == mf.EINVAL  # the mode is off
    assert b"guard mode is off" in L.mfgpu_last_error()


def test_check_with_nothing_registered_needs_no_device():
    assert mf.guard_check_raw() == (0, 0, "")
    assert mf.guard_check() == 0


def test_symbols_are_declared():
    for s in ("mfgpu_debug_guard_begin", "mfgpu_debug_guard_end", "mfgpu_debug_guard_layout", "mfgpu_debug_guard_check",
              "mfgpu_debug_guard_selftest"):
        assert s in mf.SYMBOLS and hasattr(mf.lib(), s)
