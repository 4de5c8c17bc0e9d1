"""Device-resident BiCGStab (mfgpu_bicgstab, pymfgpu.BiCGStab) against the numpy recurrence of
tests/bicgstab_reference.py: the same right-preconditioned loop with a zero start, sums in float64, alpha, omega and
beta rounded to the vectors' type.  The reference's matvec is the assembled matrix of qop_reference (double, through
QpOperator) or the oracle's Laplacian (float, through Operator on Mesh.uniform).

Tolerances (tests/test_bicgstab_host.py recomputes what they rest on): six iterates 1e-12 relative in double -- their
sensitivity to the summation order is below 1e-14 on the cases used -- and 1e-5 in float, ten times what float32 numpy
shows against float64 numpy.  Solves to 1e-10 |b| (1e-4 |b| in float): status 1, the solver's residual within the
tolerance, the true residual of the assembled matrix at most 2e-10 (2e-4), and at most twice the reference's iteration
count: BiCGStab's count moves with the summation order (by up to 13 % between two orders on the host), so the bound is a
cap against stagnation, not a parity check.  Everything that compares two device runs is bitwise."""
import ctypes as C
import functools

import numpy as np
import pytest

import torch  # before the library is loaded: libmfgpu.so binds to the HIP runtime torch brings (as in bench.py)

import bicgstab_reference as ref
import poisson_reference as pr
import pymfgpu as mf
from oracle import mf_oracle as o
from test_bicgstab_host import CASES, LAPLACE, half_exit_tolerance, qop_problem, rel
from test_gpu_cg import NT, dv, problem
from test_gpu_evaluate import integrator
from test_gpu_qop import BETA, BIT, _driver
from test_qop_host import NEWTON_STEPS

pytestmark = pytest.mark.gpu

KIND = {"none": mf.CG_NONE, "jacobi": mf.CG_JACOBI}
ITERATE_TOL = {np.float64: 1e-12, np.float32: 1e-5}
IDS = ["-".join(str(v) for v in c) for c in CASES]


class Device:
    """the device side of a QopProblem: integrator, operator, inverse diagonal (the reference's, uploaded)"""

    def __init__(self, P):
        self.P = P
        self.it = integrator(P.mesh)
        terms = 0
        for name in P.coefs:
            terms |= BIT[name] if BIT[name] else (mf.QOP_DIFFUSION_TENSOR if P.tensor else mf.QOP_DIFFUSION_SCALAR)
        self.q = mf.QpOperator(self.it, terms)
        self.q.set_coefficients(**{k: dv(v.reshape(-1)) for k, v in P.coefs.items()})
        self.dinv = dv(P.dinv)
        mf.synchronize()

    def solver(self, prec, **kw):
        return mf.BiCGStab(self.q, KIND[prec], self.dinv if prec == "jacobi" else None, **kw)


@functools.lru_cache(maxsize=None)
def device(kind, dim, p, cset):
    return Device(qop_problem(kind, dim, p, cset))


def laplace_solver(P, prec, dt):
    op = P.op(dt)
    return mf.BiCGStab(op, KIND[prec], P.dinv_dev[dt] if prec == "jacobi" else None)


def laplace_reference(P, prec, dt, b, tolerance, max_iterations):
    A = P.A.astype(dt)
    return ref.bicgstab(lambda v: A @ v, b, ref.preconditioner(prec, P.dinv.astype(dt)), dt, tolerance, max_iterations)


def check_six_iterates(solver, x, b, reference, dt):
    """begin, then iterate(1) six times: x against the float64 reference after each; count and status after each"""
    solver.begin(x, b, 0.0, 1000)
    worst = 0.0
    for k, (it, status, res, want) in zip(range(7), reference):
        if k:
            solver.iterate(1)
            worst = max(worst, rel(x.to_host(), want))
        info = solver.status()
        assert (info.iterations, info.status) == (it, status) == (k, 0)
        assert abs(info.residual - res) <= 1e3 * ITERATE_TOL[dt] * res
    print(f"largest relative difference of six iterates: {worst:.3e} (tolerance {ITERATE_TOL[dt]:.0e})")
    assert worst <= ITERATE_TOL[dt]


@pytest.mark.parametrize("case,transpose", [(c, False) for c in CASES] + [(CASES[1], True)],
                         ids=IDS + [IDS[1] + "-transpose"])
def test_iterates_match_reference_double(case, transpose):
    kind, dim, p, cset, prec = case
    D = device(kind, dim, p, cset)
    P = D.P
    b = P.rhs()
    solver = D.solver(prec, transpose=transpose)
    x = mf.DeviceVector(P.N)
    x.fill(np.nan)  # begin writes every entry
    check_six_iterates(solver, x, dv(b), P.reference(prec, np.float64, b, 0.0, 1000, transpose=transpose), np.float64)


@pytest.mark.parametrize("prec", ["none", "jacobi"])
@pytest.mark.parametrize("m", LAPLACE)
def test_iterates_match_reference_float(m, prec):
    """(2, 2, 8) has 289 dofs: one block of the 16-byte path plus a tail"""
    P = problem(*m)
    b = P.rhs(0)
    solver = laplace_solver(P, prec, np.float32)
    x = mf.DeviceVector(P.N, mf.F32)
    x.fill(np.nan)
    check_six_iterates(solver, x, dv(b, np.float32), laplace_reference(P, prec, np.float64, b, 0.0, 1000), np.float32)


def check_solve(solver, reference, A, b, N, dt, tol, bound):
    tolerance = tol * np.linalg.norm(b)
    ref_it, ref_status, ref_res, _ = list(reference(tolerance))[-1]
    assert ref_status == 1 and ref_res <= tolerance
    x = mf.DeviceVector(N, NT[dt])
    x.fill(np.nan)
    info = solver.solve(x, dv(b, dt), tolerance, 10000, check_every=5)
    true = np.linalg.norm(b - A @ x.to_host().astype(np.float64)) / np.linalg.norm(b)
    print(f"iterations {info.iterations} (reference {ref_it}), residual {info.residual / np.linalg.norm(b):.3e}, "
          f"true residual {true:.3e} (bound {bound:.0e})")
    assert info.status == 1 and info.residual <= tolerance
    assert abs(info.initial_residual - np.linalg.norm(b.astype(dt))) <= 1e-6 * np.linalg.norm(b)
    assert true <= bound
    assert 0 < info.iterations <= 2 * ref_it


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_solve_to_convergence_double(case):
    kind, dim, p, cset, prec = case
    D = device(kind, dim, p, cset)
    P = D.P
    b = P.rhs()
    check_solve(D.solver(prec), lambda t: P.reference(prec, np.float64, b, t, 10000), P.A, b, P.N, np.float64, 1e-10, 2e-10)


@pytest.mark.parametrize("prec", ["none", "jacobi"])
@pytest.mark.parametrize("m", LAPLACE)
def test_solve_to_convergence_float(m, prec):
    P = problem(*m)
    b = P.rhs(1)
    check_solve(laplace_solver(P, prec, np.float32), lambda t: laplace_reference(P, prec, np.float32, b, t, 10000), P.A, b,
                P.N, np.float32, 1e-4, 2e-4)


# ---- the convection-diffusion known-answer problem of test_gpu_qop.py
def convection_diffusion_error(mesh):
    """test_gpu_qop.convection_diffusion_error with the solve on the device: BiCGStab(q, JACOBI) to 1e-12 |b|"""
    dim = int(mesh.desc.dim)
    it = integrator(mesh)
    N, npts = mesh.n_dofs, mesh.n_cells * mesh.nd
    xq = mesh.arrays()["quadrature_points"].astype(np.float64).reshape(-1, dim)
    beta = np.broadcast_to(BETA[dim], (npts, dim))
    q = mf.QpOperator(it, mf.QOP_DIFFUSION_SCALAR | mf.QOP_CONVECTION)
    q.set_coefficients(diffusion=dv(np.ones(npts)), convection=dv(beta.reshape(-1)))
    con = mesh.arrays()["constrained_dofs"]
    ub_h = np.zeros(N)
    ub_h[con] = pr.solution(mesh.dof_coords()[con])
    ub = dv(ub_h)
    gb = mf.DeviceVector(npts * dim)
    it.evaluate(ub, gradients=gb)
    g_h = gb.to_host().reshape(-1, dim)
    f = -pr.solution_laplacian(xq) + pr.solution_gradient(xq) @ BETA[dim]
    b, dinv, x = mf.DeviceVector(N), mf.DeviceVector(N), mf.DeviceVector(N)
    it.integrate(b, dv(f - g_h @ BETA[dim]), dv(-g_h.reshape(-1)))
    q.inverse_diagonal(dinv)
    solver = mf.BiCGStab(q, mf.CG_JACOBI, dinv)
    solver.begin_relative(x, b, 1e-12, 20000)
    info = solver.status()
    while info.status == 0:
        solver.iterate(10)
        info = solver.status()
    assert info.status == 1, info.as_tuple()
    x.add(1.0, ub)
    return it.l2_error(x), info.iterations


@pytest.mark.parametrize("dim,p", [(2, 2), (3, 2)])
def test_convection_diffusion_known_answer(dim, p):
    errs = []
    for level in range(3):
        err, its = convection_diffusion_error(pr.family("cube", dim, p, level))
        print(f"{dim}D p={p} level {level}: L2 error {err:.4e}, {its} BiCGStab iterations")
        errs.append(err)
    assert pr.orders(errs)[-1] >= p + 0.7, errs  # the bound of test_gpu_qop.py


# ---- the half-step exit
def test_half_step_exit():
    kind, dim, p, cset, prec = CASES[1]
    D = device(kind, dim, p, cset)
    P = D.P
    b = P.rhs()
    tolerance, it = half_exit_tolerance(P, prec, b)
    want = list(P.reference(prec, np.float64, b, tolerance, 10000))[-1]
    before = list(P.reference(prec, np.float64, b, 0.0, it - 1))[-1]
    assert (want[0], want[1]) == (it, 1) and want[2] <= tolerance < before[2]  # |s| of iteration it, |r| before it
    solver = D.solver(prec)
    x = mf.DeviceVector(P.N)
    x.fill(np.nan)
    solver.begin(x, dv(b), tolerance, 10000)
    solver.iterate(it + 4)  # the exit takes effect on the device: no host visit between the iterations
    info = solver.status()
    print(f"half-step exit in iteration {it}: |s| = {info.residual:.6e} (reference {want[2]:.6e}), tolerance {tolerance:.3e}")
    assert (info.iterations, info.status) == (it, 1)
    assert abs(info.residual - want[2]) <= 1e-9 * want[2] and info.residual <= tolerance
    assert rel(x.to_host(), want[3]) <= 1e-12
    full = list(P.reference(prec, np.float64, b, 0.0, it))[-1]
    assert rel(full[3], want[3]) > 1e-6  # (the full step would have moved x visibly)


# ---- freeze and chunking: bitwise
def _qop_setup():
    kind, dim, p, cset, prec = CASES[2]
    D = device(kind, dim, p, cset)
    return D.solver(prec), D.P.N, D.P.rhs()


def _laplace_setup():
    P = problem(3, 4, 3)
    return laplace_solver(P, "jacobi", np.float64), P.N, P.rhs(1)


SETUPS = pytest.mark.parametrize("setup", [_qop_setup, _laplace_setup], ids=["qop", "laplace-3-4-3"])


@SETUPS
def test_check_every_does_not_change_the_solve(setup):
    solver, N, b = setup()
    bd, tolerance = dv(b), 1e-10 * np.linalg.norm(b)
    results = []
    for check_every in (1, 7, 1000, 1000):  # the last two: two solves on the same inputs
        x = mf.DeviceVector(N)
        x.fill(np.nan)
        info = solver.solve(x, bd, tolerance, 10000, check_every=check_every)
        results.append((x.to_host(), info.as_tuple()))
    assert results[0][1][1] == 1 and results[0][1][0] > 10
    for xh, info in results[1:]:
        assert np.array_equal(xh, results[0][0]) and info == results[0][1]


@SETUPS
def test_chunking_and_iterations_past_the_end(setup):
    solver, N, b = setup()
    bd, tolerance = dv(b), 1e-10 * np.linalg.norm(b)
    x1, x6 = mf.DeviceVector(N), mf.DeviceVector(N)
    solver.begin(x1, bd, tolerance, 10000)
    for _ in range(6):
        solver.iterate(1)
    solver.begin(x6, bd, tolerance, 10000)
    solver.iterate(6)
    assert solver.status().as_tuple()[:2] == (6, 0)
    assert np.array_equal(x1.to_host(), x6.to_host())
    info = solver.status()
    while info.status == 0:
        solver.iterate(3)
        info = solver.status()
    assert info.status == 1
    xh = x6.to_host()
    solver.iterate(50)
    after = solver.status()
    assert after.as_tuple() == info.as_tuple() and np.array_equal(x6.to_host(), xh)


@SETUPS
def test_max_iterations_zero_rhs_and_relative_begin(setup):
    solver, N, b = setup()
    x = mf.DeviceVector(N)
    info = solver.solve(x, dv(b), 1e-10 * np.linalg.norm(b), 3, check_every=2)
    assert (info.iterations, info.status) == (3, 2)
    x3 = x.to_host()
    assert np.all(np.isfinite(x3)) and np.linalg.norm(x3) > 0
    solver.iterate(4)  # frozen
    assert solver.status().as_tuple() == info.as_tuple() and np.array_equal(x.to_host(), x3)
    zero = dv(np.zeros(N))
    for begin in (solver.begin, solver.begin_relative):
        x.fill(np.nan)
        begin(x, zero, 1e-10, 100)
        solver.iterate(3)
        info = solver.status()
        assert (info.iterations, info.status, info.residual, info.initial_residual) == (0, 1, 0.0, 0.0)
        assert np.array_equal(x.to_host(), np.zeros(N))
    # begin_relative against begin with the tolerance formed on the host from the device's own |b|
    bd = dv(b)
    xa, xr = mf.DeviceVector(N), mf.DeviceVector(N)
    solver.begin(xa, bd, 0.0, 0)
    norm_b = solver.status().initial_residual
    infos = []
    for xv, begin, tol in ((xa, solver.begin, 1e-6 * norm_b), (xr, solver.begin_relative, 1e-6)):
        begin(xv, bd, tol, 10000)
        info = solver.status()
        while info.status == 0:
            solver.iterate(5)
            info = solver.status()
        infos.append(info.as_tuple())
    assert infos[0] == infos[1] and infos[0][1] == 1
    assert np.array_equal(xa.to_host(), xr.to_host())


def test_breakdown_freezes_with_status_3():
    """an operator that writes zeros: r0.v = 0 in the first iteration, an arithmetic exit with x untouched"""
    P = problem(2, 2, 8)
    solver = mf.BiCGStab(lambda dst, src, stream: dst.fill(0.0, stream), n=P.N)
    x = mf.DeviceVector(P.N)
    x.fill(np.nan)
    solver.begin(x, dv(P.rhs(0)), 1e-10, 100)
    solver.iterate(3)
    info = solver.status()
    assert (info.iterations, info.status) == (0, 3)
    assert np.array_equal(x.to_host(), np.zeros(P.N))
    solver.iterate(2)
    assert solver.status().as_tuple() == info.as_tuple() and np.array_equal(x.to_host(), np.zeros(P.N))


# ---- callbacks
def test_operator_callable_gives_the_bits_of_set_operator_qop():
    kind, dim, p, cset, prec = CASES[1]
    D = device(kind, dim, p, cset)
    P = D.P
    bd = dv(P.rhs())
    calls = []

    def apply(dst, src, stream):
        calls.append(stream)
        D.q.vmult(dst, src, stream=stream)

    builtin = D.solver(prec)
    through = mf.BiCGStab(apply, KIND[prec], D.dinv, n=P.N)
    xb, xc = mf.DeviceVector(P.N), mf.DeviceVector(P.N)
    builtin.begin(xb, bd, 0.0, 1000)
    builtin.iterate(6)
    through.begin(xc, bd, 0.0, 1000)
    through.iterate(6)
    assert through.status().as_tuple() == builtin.status().as_tuple() and through.status().iterations == 6
    assert len(calls) == 12 and np.array_equal(xb.to_host(), xc.to_host())


def test_callback_jacobi_matches_builtin_and_error_codes_pass_through():
    kind, dim, p, cset, prec = CASES[1]
    D = device(kind, dim, p, cset)
    P = D.P
    bd = dv(P.rhs())
    rc = [0]

    def jacobi(z, r, stream):
        z.equ(1.0, r, stream)
        z.scale(D.dinv, stream)
        return rc[0]

    cb = mf.BiCGStab(D.q, mf.CG_CALLBACK, callback=jacobi)
    builtin = D.solver("jacobi")
    xc, xb = mf.DeviceVector(P.N), mf.DeviceVector(P.N)
    cb.begin(xc, bd, 0.0, 1000)
    builtin.begin(xb, bd, 0.0, 1000)
    for _ in range(6):
        cb.iterate(1)
        builtin.iterate(1)
        assert rel(xc.to_host(), xb.to_host()) <= 1e-12
    assert cb.status().iterations == 6
    assert cb.memory_consumption() == 7 * P.N * 8 + mf.BICGSTAB_PARTIAL_BYTES + mf.BICGSTAB_STATE_BYTES
    rc[0] = -7
    assert cb.iterate(1, check=False) == -7
    assert cb.begin(xc, bd, 0.0, 1000, check=False) == -7


@pytest.mark.parametrize("hierarchy", ["uniform", "adaptive_mg"])
def test_vcycle_preconditioner_needs_fewer_iterations_than_jacobi(hierarchy):
    """the Laplacian's V-cycle under a convection-diffusion operator on the same mesh (the mesh's own coefficient as the
    scalar diffusion, beta = BETA of test_gpu_qop.py): uniform 2D p2 cubes of 4, 8, 16 cells per direction through
    VCycle.from_meshes, and the local-smoothing hierarchy of Mesh.adaptive_mg(2, 2, 3) through VCycle.from_hierarchy"""
    if hierarchy == "uniform":
        meshes = [mf.Mesh.uniform(2, 2, n) for n in (4, 8, 16)]
        mesh, V = meshes[-1], mf.VCycle.from_meshes(meshes)
    else:
        mesh = mf.Mesh.adaptive_mg(2, 2, 3)
        V = mf.VCycle.from_hierarchy(mesh)
    it = integrator(mesh)
    N, npts = mesh.n_dofs, mesh.n_cells * mesh.nd
    xq = mesh.arrays()["quadrature_points"].astype(np.float64)
    q = mf.QpOperator(it, mf.QOP_DIFFUSION_SCALAR | mf.QOP_CONVECTION)
    q.set_coefficients(diffusion=dv(np.asarray(o.coefficient_value(xq), np.float64).reshape(-1)),
                       convection=dv(np.broadcast_to(BETA[2], (npts, 2)).reshape(-1)))
    dinv = mf.DeviceVector(N)
    q.inverse_diagonal(dinv)
    b = np.random.default_rng(1).standard_normal(N)
    b[mesh.arrays()["constrained_dofs"]] = 0.0
    bd = dv(b)
    jacobi = mf.BiCGStab(q, mf.CG_JACOBI, dinv)
    mg = mf.BiCGStab(q, mf.CG_CALLBACK)
    mg.set_vcycle(V)
    counts = []
    for solver in (jacobi, mg):
        x = mf.DeviceVector(N)
        info = solver.solve(x, bd, 1e-10 * np.linalg.norm(b), 10000, check_every=1)
        assert info.status == 1
        src, dst = x, mf.DeviceVector(N)
        q.vmult(dst, src)
        assert np.linalg.norm(b - dst.to_host()) <= 2e-10 * np.linalg.norm(b)
        counts.append(int(info.iterations))
    print(f"{hierarchy}: {N} dofs, iterations JACOBI {counts[0]}, V-cycle {counts[1]}")
    assert counts[1] < counts[0]


# ---- memory
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["double", "float"])
@pytest.mark.parametrize("prec,n_vectors", [("none", 5), ("jacobi", 7)])
def test_memory_consumption(prec, n_vectors, dt):
    """r, r0, p, v, t (+ y, z with a preconditioner) + 6 x 2048 partial sums + the 128-byte state block"""
    P = problem(3, 4, 3)
    P.op(dt)
    x, b = mf.DeviceVector(P.N, NT[dt]), dv(P.rhs(1), dt)

    def cycle():
        solver = laplace_solver(P, prec, dt)
        assert solver.memory_consumption() == (n_vectors * P.N * np.dtype(dt).itemsize + mf.BICGSTAB_PARTIAL_BYTES +
                                               mf.BICGSTAB_STATE_BYTES)
        assert solver.solve(x, b, 1e-3 * np.linalg.norm(P.rhs(1)), 100).status == 1
        solver.destroy()
        mf.synchronize()

    cycle()  # (the first use of a kernel loads its code object: not the solver's memory)
    free0, _ = mf.device_memory_info()
    cycle()
    free1, _ = mf.device_memory_info()
    assert free1 == free0, (free0, free1)


# ---- argument checks that need a device
def test_argument_checks():
    P = problem(2, 2, 8)
    op, op32 = P.op(np.float64), P.op(np.float32)
    dinv = P.dinv_dev[np.float64]
    kind, dim, p, cset, _ = CASES[1]
    D = device(kind, dim, p, cset)
    L = mf.lib()
    with pytest.raises(mf.MfgpuError, match="error -1"):
        mf.BiCGStab(op, mf.CG_JACOBI)  # no inv_diag
    for prec in (mf.CG_CHEBYSHEV, 4, -1):
        with pytest.raises(mf.MfgpuError, match="error -1"):
            mf.BiCGStab(op, prec, dinv)
    x, b = mf.DeviceVector(P.N), dv(P.rhs(0))
    x.fill(3.0)
    bare = mf.BiCGStab(lambda dst, src, s: 0, n=P.N)
    h = bare._h
    # operators that do not fit
    assert L.mfgpu_bicgstab_set_operator_handle(h, op32._h) == mf.EINVAL  # type
    assert L.mfgpu_bicgstab_set_operator_handle(h, problem(3, 2, 4).op(np.float64)._h) == mf.EINVAL  # length
    assert L.mfgpu_bicgstab_set_operator_qop(h, D.q._h, 0) == mf.EINVAL  # length
    single = mf.BiCGStab(lambda d, s, t: 0, n=D.P.N, number_type=mf.F32)
    assert L.mfgpu_bicgstab_set_operator_qop(single._h, D.q._h, 0) == mf.EINVAL  # type
    fits = mf.BiCGStab(lambda d, s, t: 0, n=D.P.N)
    assert L.mfgpu_bicgstab_set_operator_qop(fits._h, D.q._h, 2) == mf.EINVAL  # unknown flag
    assert L.mfgpu_bicgstab_set_operator_qop(fits._h, D.q._h, mf.QOP_TRANSPOSE) == mf.OK
    assert L.mfgpu_bicgstab_set_operator(h, mf.CG_CALLBACK_TYPE(0), None) == mf.EINVAL
    # begin before an operator is set
    fresh = C_create(P.N, mf.F64, mf.CG_NONE, None)
    assert L.mfgpu_bicgstab_begin(fresh, x.ptr, b.ptr, 1e-10, 10, None) == mf.EINVAL
    assert L.mfgpu_bicgstab_iterate(fresh, 1, None) == mf.EINVAL
    L.mfgpu_bicgstab_destroy(fresh)
    solver = mf.BiCGStab(op, mf.CG_JACOBI, dinv)
    assert solver.iterate(1, check=False) == mf.EINVAL  # before begin
    with pytest.raises(mf.MfgpuError, match="error -1.*begin"):
        solver.status()
    assert solver.begin(None, b, 1e-10, 10, check=False) == mf.EINVAL
    assert solver.begin(x, None, 1e-10, 10, check=False) == mf.EINVAL
    assert solver.begin(x, x, 1e-10, 10, check=False) == mf.EINVAL
    big = mf.DeviceVector(2 * P.N)
    big.fill(3.0)
    assert solver.begin(big.ptr + 8 * (P.N - 1), big, 1e-10, 10, check=False) == mf.EINVAL  # one element overlaps
    for bad in (-1e-3, float("nan"), float("inf")):
        assert solver.begin_relative(x, b, bad, 10, check=False) == mf.EINVAL
    assert solver.iterate(1, check=False) == mf.EINVAL  # none of those began a solve
    info = mf.CGInfo()
    assert L.mfgpu_bicgstab_solve(solver._h, x.ptr, b.ptr, 1e-10, 10, 0, None, info) == mf.EINVAL  # check_every 0
    assert np.all(x.to_host() == 3.0) and np.all(big.to_host() == 3.0)  # nothing written
    assert solver.begin(big.ptr + 8 * P.N, big, 1e-10, 10, check=False) == mf.OK  # adjacent is fine
    assert L.mfgpu_bicgstab_status(solver._h, None, None) == mf.EINVAL
    # callback solvers
    cb = mf.BiCGStab(op, mf.CG_CALLBACK)
    assert cb.begin(x, b, 1e-10, 10, check=False) == mf.EINVAL  # no callback set
    assert L.mfgpu_bicgstab_set_callback(cb._h, mf.CG_CALLBACK_TYPE(0), None) == mf.EINVAL
    with pytest.raises(mf.MfgpuError, match="error -1"):
        solver.set_callback(lambda z, r, s: 0)  # not a CALLBACK solver
    # a V-cycle whose type or length differ
    meshes = [mf.Mesh.uniform(2, 2, n) for n in (4, 8)]
    V = mf.VCycle.from_meshes(meshes)
    assert meshes[-1].n_dofs == P.N
    assert solver.set_vcycle(V, check=False) == mf.EINVAL  # not a CALLBACK solver
    longer, other = mf.BiCGStab(lambda d, s, t: 0, mf.CG_CALLBACK, n=P.N + 1), mf.BiCGStab(op32, mf.CG_CALLBACK)
    assert longer.set_vcycle(V, check=False) == mf.EINVAL  # length
    assert other.set_vcycle(V, check=False) == mf.EINVAL  # type
    assert cb.set_vcycle(V, check=False) == mf.OK
    assert np.all(x.to_host() == 3.0)


def C_create(n, nt, prec, dinv):
    h = C.c_void_p()
    assert mf.lib().mfgpu_bicgstab_create(n, nt, prec, dinv, C.byref(h)) == mf.OK
    return h


# ---- drivers
@pytest.mark.parametrize("dim,p,n", [(2, 2, 8), (3, 2, 4)])
def test_newton_devbicg_drivers(dim, p, n):
    """First cycle of newton-* and newton-*-devbicg: dim  degree  n_dofs  newton_steps  inner_iterations  wall_seconds
    l2_error.  Same Newton step count, L2 errors to 1e-8 relative; the inner iteration count may differ."""
    host, dev = _driver(f"newton-{dim}d-p{p}"), _driver(f"newton-{dim}d-p{p}-devbicg")
    print(host, dev)
    assert host[:3] == dev[:3] and [int(v) for v in dev[:3]] == [dim, p, (p * n + 1) ** dim]
    assert int(host[3]) == int(dev[3]) == NEWTON_STEPS[(dim, p, n)]
    assert int(dev[3]) <= int(dev[4]) <= 2 * int(host[4])
    assert abs(float(host[6]) - float(dev[6])) <= 1e-8 * float(host[6])
