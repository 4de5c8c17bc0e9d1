"""The streaming vector kernels of csrc/mfgpu_mixed.hip at the sizes where the chunk-and-tail skeleton
(csrc/mfgpu_stream.h) changes what a thread does: with W elements per 16-byte chunk (2 doubles, 4 floats; 4 for the
conversion in both directions),
  n = W - 1, W, W + 1          no chunk / one chunk and no tail / one chunk and a one-element tail
  n = 256 W + 1                more than one block
  n = 2048 * 256 W + 256 W + 3 above the 2048-block cap: every thread loops twice over chunks, the last trip is partial,
                               and the tail has three elements
each once on 16-byte aligned vectors and once through views offset by one element (the scalar path from 0).  Conversion
and residual are compared bitwise with numpy, the Chebyshev calls with the per-entry relative tolerances of
tests/test_gpu_mixed_mg.py (1e-14 / 1e-6 for r, four times that for upd and x; positive data).  Every vector a call
writes is a view into a larger buffer whose other elements -- the guard in front and the guard behind among them -- must
keep their values.  The CG kernels of csrc/mfgpu_cg.hip are at such a size and on misaligned vectors in
tests/test_gpu_cg.py."""
import functools

import numpy as np
import pytest

import pymfgpu as mf

pytestmark = pytest.mark.gpu

GUARD = -77.0


def _sizes(W):
    return [W - 1, W, W + 1, 256 * W + 1, 2048 * 256 * W + 256 * W + 3]


def _lanes(nt):
    return 16 // np.dtype(mf.np_dtype(nt)).itemsize


# (index into _sizes, number type, aligned)
CASES = [pytest.param(i, nt, al, id="n%d-%s-%s" % (i, "f64" if nt == mf.F64 else "f32", "aligned" if al else "offset"))
         for i in range(5) for nt in (mf.F64, mf.F32) for al in (True, False)]


class View:
    """n elements of a device buffer: 16 bytes in (aligned) or one element further (not), GUARD everywhere else"""

    def __init__(self, a, nt, aligned):
        dt = mf.np_dtype(nt)
        self.n, self.es = a.size, np.dtype(dt).itemsize
        self.off = 16 // self.es + (0 if aligned else 1)
        self.before = np.full(self.n + self.off + 2, GUARD, dtype=dt)
        self.before[self.off:self.off + self.n] = a
        self.buf = mf.DeviceVector(self.before.size, nt)
        self.buf.from_host(self.before)
        self.ptr = self.buf.ptr + self.off * self.es
        assert (self.ptr % 16 == 0) == aligned

    def result(self):
        """the view's elements after the calls; everything around it must be as it was"""
        got = self.buf.to_host()
        lo, hi = self.off, self.off + self.n
        assert got[lo - 1] == GUARD and got[hi] == GUARD, "guard element overwritten"
        np.testing.assert_array_equal(got[:lo], self.before[:lo])
        np.testing.assert_array_equal(got[hi:], self.before[hi:])
        return got[lo:hi]


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(maxsize=None)
def _convert_values(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)
    special = np.array([1e39, -1e300, 3.4028235677973366e38, 3.4028236e38, 1e-40, -0.0, np.inf, 1.0 + 3 * 2.0 ** -24])
    x[n - min(n, special.size):] = special[:min(n, special.size)]  # in the last chunk and the tail
    with np.errstate(over="ignore"):
        x32 = x.astype(np.float32)
    x.setflags(write=False)
    x32.setflags(write=False)
    return x, x32


@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset"])
def test_convert_both_directions_bitwise(i, aligned):
    n = _sizes(4)[i]
    x64, x32 = _convert_values(n)
    src, dst = View(x64, mf.F64, aligned), View(np.zeros(n), mf.F32, aligned)
    mf.vec_convert(dst.ptr, mf.F32, src.ptr, mf.F64, n)
    back = View(np.zeros(n), mf.F64, aligned)
    mf.vec_convert(back.ptr, mf.F64, dst.ptr, mf.F32, n)
    mf.synchronize()
    np.testing.assert_array_equal(_bits(dst.result()), _bits(x32))
    np.testing.assert_array_equal(_bits(back.result()), _bits(x32.astype(np.float64)))  # float -> double is exact
    np.testing.assert_array_equal(_bits(src.result()), _bits(x64))


@functools.lru_cache(maxsize=None)
def _inputs(n, nt):
    rng = np.random.default_rng(1000 * n + nt)
    dt = mf.np_dtype(nt)
    # positive data: no cancellation, so a per-entry relative bound is meaningful (as tests/test_gpu_mixed_mg.py)
    h = {k: rng.uniform(lo, hi, n).astype(dt) for k, lo, hi in
         (("x", 1, 2), ("upd", 0.5, 1), ("r", 1, 2), ("b", 1, 2), ("t", 0, 0.5), ("dinv", 0.1, 1), ("e", 0, 0.5))}
    for a in h.values():
        a.setflags(write=False)
    return h


def _close(got, want, tol):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= tol * np.abs(want)), np.max(err / np.abs(want))


def _tol(nt):
    return 1e-14 if nt == mf.F64 else 1e-6


@pytest.mark.parametrize("i,nt,aligned", CASES)
def test_chebyshev_start(i, nt, aligned):
    n, dt, tol = _sizes(_lanes(nt))[i], mf.np_dtype(nt), _tol(nt)
    h = _inputs(n, nt)
    H = {k: a.astype(np.float64) for k, a in h.items()}
    f = 0.37
    for zero_start in (True, False):
        for with_t in (True, False):
            v = {k: View(h[k], nt, aligned) for k in ("x", "upd", "r", "b", "t", "dinv")}
            mf.chebyshev_start(v["x"].ptr, v["upd"].ptr, v["r"].ptr, v["b"].ptr, v["t"].ptr if with_t else None,
                               v["dinv"].ptr, f, zero_start, n, nt)
            mf.synchronize()
            r = (H["b"] - H["t"] if with_t else H["b"]).astype(dt).astype(np.float64)
            u = float(dt(f)) * r * H["dinv"]
            _close(v["r"].result(), r, tol)
            _close(v["upd"].result(), u, 4 * tol)
            _close(v["x"].result(), u if zero_start else H["x"] + u, 4 * tol)
            for k in ("b", "t", "dinv"):
                np.testing.assert_array_equal(_bits(v[k].result()), _bits(h[k]))


@pytest.mark.parametrize("i,nt,aligned", CASES)
def test_chebyshev_update(i, nt, aligned):
    n, dt, tol = _sizes(_lanes(nt))[i], mf.np_dtype(nt), _tol(nt)
    h = _inputs(n, nt)
    H = {k: a.astype(np.float64) for k, a in h.items()}
    f1, f2 = 0.81, 1.23
    v = {k: View(h[k], nt, aligned) for k in ("x", "upd", "r", "t", "dinv")}
    mf.chebyshev_update(v["x"].ptr, v["upd"].ptr, v["r"].ptr, v["t"].ptr, v["dinv"].ptr, f1, f2, n, nt)
    mf.synchronize()
    r = (H["r"] - H["t"]).astype(dt).astype(np.float64)
    u = float(dt(f1)) * H["upd"] + float(dt(f2)) * r * H["dinv"]
    _close(v["r"].result(), r, tol)
    _close(v["upd"].result(), u, 4 * tol)
    _close(v["x"].result(), H["x"] + u, 4 * tol)
    for k in ("t", "dinv"):
        np.testing.assert_array_equal(_bits(v[k].result()), _bits(h[k]))


@pytest.mark.parametrize("i,nt,aligned", CASES)
def test_residual_bitwise(i, nt, aligned):
    n = _sizes(_lanes(nt))[i]
    h = _inputs(n, nt)
    for with_e in (False, True):
        v = {k: View(h[k], nt, aligned) for k in ("t", "b", "e")}
        mf.vec_residual(v["t"].ptr, v["b"].ptr, v["e"].ptr if with_e else None, n, nt)
        mf.synchronize()
        want = h["b"] - (h["t"] + h["e"]) if with_e else h["b"] - h["t"]  # in the number type: one rounding per operation
        np.testing.assert_array_equal(_bits(v["t"].result()), _bits(want))
        for k in ("b", "e"):
            np.testing.assert_array_equal(_bits(v[k].result()), _bits(h[k]))
