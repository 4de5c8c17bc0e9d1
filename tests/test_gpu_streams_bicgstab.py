"""mfgpu_bicgstab_begin + mfgpu_bicgstab_iterate on the caller's stream (tests/stream_harness.py, as
tests/test_gpu_streams.py does for every other asynchronous call): ordered behind a delay on a non-blocking stream, and
captured once in a graph that is replayed on new right-hand sides.  Value sets 0 and 1 are compared with the numpy
recurrence of tests/bicgstab_reference.py at the iterate tolerance of tests/test_gpu_bicgstab.py (1e-12 relative,
double)."""
import functools

import numpy as np
import pytest

import pymfgpu as mf
from stream_harness import Case, check_graph, check_ordered, sets
from test_bicgstab_host import CASES as ROWS, rel
from test_gpu_bicgstab import device

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K = 3
CASES = {"qop-jacobi": ROWS[1], "qop-none": ROWS[3]}


@functools.lru_cache(maxsize=None)
def build(name):
    kind, dim, p, cset, prec = CASES[name]
    D = device(kind, dim, p, cset)
    P = D.P
    solver = D.solver(prec)

    def make(rng):
        b = rng.standard_normal(P.N)
        b[P.constrained] = 0.0
        return b

    b = sets(make, 260)

    def call(bufs, s):
        solver.begin(bufs["x"], bufs["b"], 0.0, 1000, s)
        solver.iterate(K, s)

    def check(k, got, ret):
        want = list(zip(range(K + 1), P.reference(prec, np.float64, b[k], 0.0, 1000)))[-1][1]
        assert want[:2] == (K, 0)
        err = rel(got["x"], want[3])
        print(f"{name} value set {k}: rel l2 {err:.3e}")
        assert err <= 1e-12
        assert solver.status().as_tuple()[:2] == (K, 0)

    return Case(f"bicgstab_begin_iterate{K}-{name}", {"b": b}, {"x": (np.float64, P.N)}, call, check)


@pytest.mark.parametrize("name", list(CASES))
def test_ordered_behind_a_delay(name):
    check_ordered(build(name))


@pytest.mark.parametrize("name", list(CASES))
def test_captured_and_replayed(name):
    check_graph(build(name))
