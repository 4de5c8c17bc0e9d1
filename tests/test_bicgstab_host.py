"""Host side of the device-resident BiCGStab (mfgpu_bicgstab, include/mfgpu.h): the numpy
reference of the GPU tests (tests/bicgstab_reference.py) against qop_reference.bicgstab, the argument checks that need
no device, and the measurements that the tolerances of tests/test_gpu_bicgstab.py rest on.

BiCGStab's iterates depend on the order in which its five sums per iteration are formed, far more than CG's: over a
whole solve the iteration count moves with the order (by up to 13 % in the measurements behind this change; the counts
below depend on the host's BLAS), so no test demands the reference's count.  Over six iterations the iterates of two
summation orders (np.dot, and 37 interleaved subsequences summed first) differ by at most 7e-15 relative on the cases of
CASES; the bound asserted here is 1e-14, which leaves the suite's 1e-12 a factor of 100.  The table is recomputed and
asserted (test_sensitivity_table), so that the GPU tolerances rest on the reference alone.  One run here, as
(iterations with np.dot / strided, six-iterate sensitivity, float32 against float64 over six iterates):
    hanging 2D p3 five jacobi   122 / 122   6.0e-16   2.2e-7
    ball 2D p2    five jacobi    30 / 30    6.6e-16   2.9e-7
    cube 3D p4    five jacobi    46 / 46    2.8e-16   3.2e-7
    cube 3D p4    five none      47 / 48    2.8e-16   2.3e-7
    hanging 3D p2 cd   jacobi    58 / 58    2.3e-16   2.2e-7
    hanging 3D p2 cd   none     140 / 143   1.6e-15   3.8e-7
The true residual was at most 1.0e-10 |b| in every row.  Two combinations are NOT used for iterate comparisons: cube 2D
p2 cd jacobi (81 dofs; order sensitivity 1e-12) and cube 3D p4 cd none (float32 differs by 5e-5).
The float tests of the GPU run on the Laplacian of Mesh.uniform at (2,2,8), (3,2,4), (3,4,3): float32 numpy against
float64 numpy over six iterates is 1.1e-7 to 2.8e-7 there and asserted below 1e-6
(test_float_reference_on_the_laplacian), which leaves the GPU's 1e-5 a factor of 10."""
import ctypes as C
import functools

import numpy as np
import pytest

import bicgstab_reference as ref
import poisson_reference as pr
import pymfgpu as mf
import qop_reference as qr
from oracle import mf_oracle as o
from test_qop_host import fields
from util import oracle_desc_from_mesh

# (mesh kind, dim, p, coefficient set, preconditioner): the rows of the table above
CASES = [("hanging", 2, 3, "five", "jacobi"), ("ball", 2, 2, "five", "jacobi"), ("cube", 3, 4, "five", "jacobi"),
         ("cube", 3, 4, "five", "none"), ("hanging", 3, 2, "cd", "jacobi"), ("hanging", 3, 2, "cd", "none")]
CD_BETA = (8.0, 4.0, 2.0)
LAPLACE = [(2, 2, 8), (3, 2, 4), (3, 4, 3)]
SENSITIVITY_BOUND = 1e-14  # of six iterates to the summation order: 100 below the suite's 1e-12
WAYS = 37


class QopProblem:
    """one mesh and one coefficient set: the assembled matrix of qop_reference and its inverse diagonal"""

    def __init__(self, kind, dim, p, cset):
        self.mesh = mf.Mesh.uniform(3, 4, 3) if (kind, dim) == ("cube", 3) else pr.family(kind, dim, p, 0)
        self.cells = pr.Cells(self.mesh)
        od = self.cells.od
        self.N, self.dim = od.n_dofs, dim
        shape = (od.n_cells, od.nd)
        if cset == "five":
            self.coefs, self.tensor = fields(self.cells, 10 * dim + p), True
        else:
            self.coefs = {"diffusion": np.ones(shape), "convection": np.broadcast_to(np.array(CD_BETA[:dim]), shape + (dim,)).copy()}
            self.tensor = False
        self.A = qr.assemble(self.cells, **self.coefs).tocsr()
        self.AT = self.A.T.tocsr()
        self.dinv = qr.inverse_diagonal(self.cells, **self.coefs)
        self.constrained = od.constrained

    def rhs(self, seed=1):
        b = np.random.default_rng(seed).standard_normal(self.N)
        b[self.constrained] = 0.0
        return b

    def reference(self, prec, dt, b, tolerance, max_iterations, dot=ref.dot, transpose=False):
        A = (self.AT if transpose else self.A).astype(dt)
        return ref.bicgstab(lambda v: A @ v, b, ref.preconditioner(prec, self.dinv.astype(dt)), dt, tolerance,
                            max_iterations, dot)


@functools.lru_cache(maxsize=None)
def qop_problem(kind, dim, p, cset):
    return QopProblem(kind, dim, p, cset)


@functools.lru_cache(maxsize=None)
def laplace(dim, p, n):
    """(matrix, inverse diagonal, constrained dofs) of the Laplacian on Mesh.uniform(dim, p, n)"""
    mesh = mf.Mesh.uniform(dim, p, n)  # the description's arrays are views into it
    od = oracle_desc_from_mesh(mesh)
    A = o.assemble(od).tocsr()
    return A, 1.0 / A.diagonal(), np.array(od.constrained)


def rel(got, want):
    return np.linalg.norm(got.astype(np.float64) - want.astype(np.float64)) / np.linalg.norm(want.astype(np.float64))


def six(gen):
    return [x.copy() for (it, status, res, x), _ in zip(gen, range(7))][1:]


@pytest.mark.parametrize("kind,dim,p,cset,prec", [CASES[1], CASES[3]])
def test_reference_reproduces_qop_reference_bit_for_bit(kind, dim, p, cset, prec):
    P = qop_problem(kind, dim, p, cset)
    b = P.rhs()
    dinv = P.dinv if prec == "jacobi" else np.ones(P.N)
    want, want_it = qr.bicgstab(lambda v: P.A @ v, b, dinv, rtol=1e-10)
    last = list(P.reference(prec, np.float64, b, 1e-10 * np.linalg.norm(b), 10000))[-1]
    assert (last[0], last[1]) == (want_it, 1)
    assert np.array_equal(last[3], want)


def test_reference_exits():
    A, dinv, con = laplace(2, 2, 8)
    b = np.random.default_rng(0).standard_normal(A.shape[0])
    b[con] = 0.0
    none = ref.preconditioner("none", None)
    assert [(h[0], h[1]) for h in ref.bicgstab(lambda v: A @ v, b, none, np.float64, 0.0, 3)] == [(0, 0), (1, 0), (2, 0), (3, 2)]
    assert [(h[0], h[1], h[2]) for h in ref.bicgstab(lambda v: A @ v, 0 * b, none, np.float64, 0.0, 3)] == [(0, 1, 0.0)]
    out = list(ref.bicgstab(lambda v: 0 * v, b, none, np.float64, 0.0, 3))  # r0.v = 0
    assert [(h[0], h[1]) for h in out] == [(0, 0), (0, 3)] and not out[-1][3].any()


def half_exit_tolerance(P, prec, b):
    """a tolerance strictly between |s| of some iteration and the |r| before it, where no earlier norm is as small: the
    solve ends at that half step.  Returns (tolerance, iteration)"""
    hist, _ = ref.history(lambda v: P.A @ v, b, ref.preconditioner(prec, P.dinv), np.float64, 1e-8 * np.linalg.norm(b), 10000)
    low = np.inf
    for k, (it, kind, norm) in enumerate(hist):
        if kind == "half" and it >= 3 and norm < 0.9 * low:
            return np.sqrt(norm * low), it
        low = min(low, norm)
    raise AssertionError("no half step undercuts the norms before it")


def test_a_half_step_exit_exists():
    P = qop_problem(*CASES[1][:4])
    b = P.rhs()
    tolerance, it = half_exit_tolerance(P, "jacobi", b)
    last = list(P.reference("jacobi", np.float64, b, tolerance, 10000))[-1]
    full = list(P.reference("jacobi", np.float64, b, 0.0, it))
    print(f"half-step exit in iteration {it} at tolerance {tolerance:.3e}: |s| = {last[2]:.3e}")
    assert (last[0], last[1]) == (it, 1) and last[2] <= tolerance
    assert full[it - 1][2] > tolerance  # |r| of the iteration before
    assert not np.array_equal(last[3], full[it][3])  # x + alpha y, not the full step


@pytest.mark.parametrize("kind,dim,p,cset,prec", CASES)
def test_sensitivity_table(kind, dim, p, cset, prec):
    P = qop_problem(kind, dim, p, cset)
    b = P.rhs()
    tolerance = 1e-10 * np.linalg.norm(b)
    ends = [list(P.reference(prec, np.float64, b, tolerance, 10000, dot))[-1] for dot in (ref.dot, ref.strided_dot(WAYS))]
    true = [np.linalg.norm(b - P.A @ e[3]) / np.linalg.norm(b) for e in ends]
    xa, xb = (six(P.reference(prec, np.float64, b, 0.0, 1000, dot)) for dot in (ref.dot, ref.strided_dot(WAYS)))
    xf = six(P.reference(prec, np.float32, b, 0.0, 1000))
    order = max(rel(a, c) for a, c in zip(xa, xb))
    single = max(rel(f, a) for f, a in zip(xf, xa))
    print(f"{kind} {dim}D p{p} ({P.N} dofs) {cset} {prec}: iterations {ends[0][0]} / {ends[1][0]}, true residuals "
          f"{true[0]:.2e} {true[1]:.2e}, six iterates: order {order:.1e}, float32 {single:.1e}")
    assert all(e[1] == 1 for e in ends) and max(true) <= 2e-10
    assert abs(ends[0][0] - ends[1][0]) <= 0.15 * ends[0][0]  # the count moves with the order: no test may pin it
    assert order <= SENSITIVITY_BOUND
    assert single <= 1e-5


@pytest.mark.parametrize("prec", ["none", "jacobi"])
@pytest.mark.parametrize("m", LAPLACE)
def test_float_reference_on_the_laplacian(m, prec):
    """float32 numpy against float64 numpy over six iterates: below 1e-6, so the GPU's float tolerance is 1e-5"""
    A, dinv, con = laplace(*m)
    b = np.random.default_rng(0).standard_normal(A.shape[0])
    b[con] = 0.0
    runs = []
    for dt in (np.float64, np.float32):
        M = A.astype(dt)
        runs.append(six(ref.bicgstab(lambda v: M @ v, b, ref.preconditioner(prec, dinv.astype(dt)), dt, 0.0, 1000)))
    worst = max(rel(f, d) for d, f in zip(*runs))
    print(f"{m} {prec}: float32 against float64 over six iterates {worst:.2e}")
    assert worst <= 1e-6


def test_argument_checks_without_a_device():
    L = mf.lib()
    h = C.c_void_p()
    dummy = C.c_void_p(256)  # never dereferenced: every call below is refused first
    for args in [(0, mf.F64, mf.CG_NONE, None), (10, mf.F64, mf.CG_JACOBI, None), (10, mf.F64, mf.CG_CHEBYSHEV, dummy),
                 (10, mf.F64, 4, dummy), (10, mf.F64, -1, None), (10, 7, mf.CG_NONE, None)]:
        assert L.mfgpu_bicgstab_create(*args, C.byref(h)) == mf.EINVAL, args
        assert not h.value  # nothing created
    assert L.mfgpu_bicgstab_create(10, mf.F64, mf.CG_NONE, None, None) == mf.EINVAL
    info = mf.CGInfo()
    fn = mf.CG_CALLBACK_TYPE(lambda *a: 0)
    assert L.mfgpu_bicgstab_set_operator(None, fn, None) == mf.EINVAL
    assert L.mfgpu_bicgstab_set_operator_handle(None, dummy) == mf.EINVAL
    assert L.mfgpu_bicgstab_set_operator_qop(None, dummy, 0) == mf.EINVAL
    assert L.mfgpu_bicgstab_set_callback(None, fn, None) == mf.EINVAL
    assert L.mfgpu_bicgstab_set_vcycle(None, dummy) == mf.EINVAL
    assert L.mfgpu_bicgstab_begin(None, dummy, dummy, 1e-10, 10, None) == mf.EINVAL
    assert L.mfgpu_bicgstab_begin_relative(None, dummy, dummy, 1e-10, 10, None) == mf.EINVAL
    assert L.mfgpu_bicgstab_iterate(None, 1, None) == mf.EINVAL
    assert L.mfgpu_bicgstab_status(None, None, C.byref(info)) == mf.EINVAL
    assert L.mfgpu_bicgstab_solve(None, dummy, dummy, 1e-10, 10, 1, None, C.byref(info)) == mf.EINVAL
    assert L.mfgpu_bicgstab_memory_consumption(None) == 0
    L.mfgpu_bicgstab_destroy(None)
    assert all(hasattr(L, s) for s in mf.SYMBOLS if s.startswith("mfgpu_bicgstab_"))
    assert mf.BICGSTAB_STATE_BYTES == 128 and mf.BICGSTAB_PARTIAL_BYTES == 6 * 2048 * 8
