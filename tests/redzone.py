"""Device vectors that sit inside red zones.  Plain helper module, no tests.

A Zoned is ONE device allocation of ZONE + n + ZONE (+ 1) elements.  The n payload elements begin ZONE elements in (with
offset_one: one element further, so the payload pointer is aligned to the element size only); `.vec` is a
DeviceVector.view of the payload.  No view extends past the allocation.

Every zone element holds a fixed quiet NaN with a recognisable payload (NAN_BITS): a zone value that enters arithmetic
poisons the result, and a store of anything else is visible in the bits.  A vector the call overwrites gets the same
pattern in its payload (Zoned(n, nt)); a vector the call reads or adds to gets its values (Zoned(values, nt)).

  result()     copies the whole allocation back, asserts both zones bitwise unchanged -- it names the first differing
               index and its distance from the payload -- and returns the payload
  unchanged()  the same, and the payload bitwise equal to what was uploaded (a read-only input)

ZONE = 4096 elements on each side is a condition, not a measurement: it exceeds the longest per-batch dof list any kernel
walks (p_kgu(7) * 64 = 2624 slots at p = 6, csrc/mfgpu_internal.h), so an access displaced by up to one whole batch list
still lands in a zone.  The zones prove nothing about indices that are wrong by more than a zone, about reads whose value
is discarded, or about the library's own buffers: those sit between guards in tests/test_gpu_guards.py (the guard mode of
include/mfgpu.h), all but g_red_buf, the static scratch of the blocking reductions."""
import numpy as np

import pymfgpu as mf

ZONE = 4096
NAN_BITS = {mf.F64: 0x7ff8dead0000beef, mf.F32: 0x7fc0beef}
BITS = {mf.F64: np.uint64, mf.F32: np.uint32}


def pattern(n, nt):
    """n elements of the zone pattern in the number type"""
    return np.full(int(n), NAN_BITS[nt], dtype=BITS[nt]).view(mf.np_dtype(nt))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


class Zoned:
    def __init__(self, values_or_n, nt=mf.F64, offset_one=False):
        dt = mf.np_dtype(nt)
        if np.ndim(values_or_n) == 0:
            payload = pattern(values_or_n, nt)  # a vector the call overwrites
        else:
            payload = np.ascontiguousarray(np.asarray(values_or_n).reshape(-1), dtype=dt)
        self.n, self.nt, self.es = payload.size, nt, np.dtype(dt).itemsize
        self.off = ZONE + (1 if offset_one else 0)
        self.before = pattern(self.off + self.n + ZONE, nt)
        self.before[self.off:self.off + self.n] = payload
        self.before.setflags(write=False)
        self.buf = mf.DeviceVector(self.before.size, nt)
        self.buf.from_host(self.before)
        self.ptr = self.buf.ptr + self.off * self.es
        assert self.ptr % 16 == (self.es if offset_one else 0), (self.ptr, offset_one)
        self.vec = self.view(0, self.n)

    def view(self, first, count):
        """`count` elements from payload element `first` (which may be negative): inside the allocation, or refused"""
        lo = self.off + int(first)
        assert 0 <= lo and lo + int(count) <= self.before.size, "a view must stay inside its allocation"
        v = mf.DeviceVector.view(self.ptr + int(first) * self.es, count, self.nt)
        v._zoned = self  # the view keeps the allocation alive
        return v

    def _check(self, expect_payload):
        mf.synchronize()
        got = self.buf.to_host()
        g, b = bits(got), bits(self.before)
        lo, hi = self.off, self.off + self.n
        front = np.nonzero(g[:lo] != b[:lo])[0]
        back = np.nonzero(g[hi:] != b[hi:])[0]
        if back.size:
            k = int(back[0])
            raise AssertionError(f"back zone touched: {back.size} element(s), the first at offset +{k} behind the payload "
                                 f"(index {hi + k} of the allocation, payload [{lo}, {hi})): bits {int(g[hi + k]):#x}, "
                                 f"value {got[hi + k]!r}")
        if front.size:
            k = int(front[-1])
            raise AssertionError(f"front zone touched: {front.size} element(s), the nearest at offset -{lo - k} in front of "
                                 f"the payload (index {k} of the allocation, payload [{lo}, {hi})): bits {int(g[k]):#x}, "
                                 f"value {got[k]!r}")
        if expect_payload:
            diff = np.nonzero(g[lo:hi] != b[lo:hi])[0]
            assert not diff.size, (f"read-only input changed: {diff.size} element(s), the first at payload index "
                                   f"{int(diff[0])}: {got[lo + int(diff[0])]!r}, uploaded {self.before[lo + int(diff[0])]!r}")
        return got[lo:hi]

    def result(self):
        return self._check(False)

    def unchanged(self):
        return self._check(True)
