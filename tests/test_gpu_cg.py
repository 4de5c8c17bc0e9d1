"""Device-resident CG (mfgpu_cg, pymfgpu.CG) against a plain numpy CG (tests/cg_reference.py: the
same recurrence, the same zero start, sums in float64, alpha and beta rounded to the vectors' type).  The reference's
matvec is the oracle's assembled matrix on the small meshes and op.vmult through the device on the large one; the
Chebyshev reference is written in numpy from the same scalars.  Meshes are (dim, degree, cells per direction) of the
uniform cube.

Tolerances: the project's parity tolerances for the iterates, 1e-12 relative in double and 1e-5 in float (float32
numpy against float64 numpy on these meshes differs by at most 1.6e-6 over six iterations).  Solves: tolerance 1e-10 |b|
in double (true residual recomputed with the oracle matrix at most 2e-10) and 1e-4 |b| in float (at most 2e-4; float32
numpy reaches 1.6e-5 to 8.9e-5 on these cases), iteration count within one of the reference's.  The reference's counts in
double: (2,2,8) JACOBI 53, (3,2,4) CHEBYSHEV 11, (3,4,3) NONE 118 or 119 depending on the host's BLAS (its residual after
118 iterations is 0.78 to 0.87 of the tolerance), (3,4,3) CHEBYSHEV 17, (3,3,4) CHEBYSHEV 15.

Measured on an MI355X: the six iterates differ from the reference by at most 3.1e-15 in double and 2.3e-7 in float; the
solves take exactly the reference's iteration counts, true residuals 1.4e-11 to 8.2e-11 in double, 1.6e-5 to 8.9e-5 in
float.

The (2,2,8) mesh has 289 dofs: an odd number, not a multiple of 4 and a single block of the 16-byte path plus a tail."""
import functools
import os
import subprocess

import numpy as np
import pytest

try:
    import torch  # before the library is loaded: libmfgpu.so binds to the HIP runtime torch brings (as in bench.py)
except ImportError:
    torch = None

import cg_reference as ref
import pymfgpu as mf
from oracle import mf_oracle as o
from util import oracle_desc_from_mesh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-cuda_amd", "host", "bin")
KIND = {"none": mf.CG_NONE, "jacobi": mf.CG_JACOBI, "chebyshev": mf.CG_CHEBYSHEV}
DEGREE, RANGE = 5, 15.0
NT = {np.float64: mf.F64, np.float32: mf.F32}


class Problem:
    """one mesh: the oracle matrix, its inverse diagonal, lambda_max = 1.2 max eig(D^-1 A), the device operators"""

    def __init__(self, dim, p, n):
        self.mesh = {np.float64: mf.Mesh.uniform(dim, p, n), np.float32: mf.Mesh.uniform(dim, p, n, number_type=mf.F32)}
        self.od = oracle_desc_from_mesh(self.mesh[np.float64])
        self.A = o.assemble(self.od).toarray()
        self.N = self.od.n_dofs
        self.dinv = 1.0 / np.diag(self.A)
        s = np.sqrt(self.dinv)
        self.lambda_max = 1.2 * np.linalg.eigvalsh(s[:, None] * self.A * s[None, :]).max()
        self.ops, self.dinv_dev = {}, {}

    def op(self, dt):
        if dt not in self.ops:
            self.ops[dt] = mf.Operator(self.mesh[dt].desc, self.mesh[dt])
            self.dinv_dev[dt] = dv(self.dinv, dt)
        return self.ops[dt]

    def rhs(self, seed):
        b = np.random.default_rng(seed).standard_normal(self.N)
        b[self.od.constrained] = 0.0
        return b

    def solver(self, kind, dt, **kw):
        op = self.op(dt)
        return mf.CG(op, KIND[kind], None if kind == "none" else self.dinv_dev[dt], DEGREE, self.lambda_max, RANGE, **kw)

    def reference(self, kind, dt, b, tolerance, max_iterations):
        A = self.A.astype(dt)
        prec = ref.preconditioner(kind, lambda v: A @ v, self.dinv.astype(dt), dt, (DEGREE, self.lambda_max, RANGE))
        return ref.cg(lambda v: A @ v, b, prec, dt, tolerance, max_iterations)


@functools.lru_cache(maxsize=None)
def problem(dim, p, n):
    return Problem(dim, p, n)


def dv(a, dt=np.float64):
    v = mf.DeviceVector(len(a), NT[dt])
    v.from_host(np.ascontiguousarray(a, dtype=dt))
    return v


def rel(got, want):
    return np.linalg.norm(got.astype(np.float64) - want.astype(np.float64)) / np.linalg.norm(want.astype(np.float64))


ITERATE_TOL = {np.float64: 1e-12, np.float32: 1e-5}


def check_six_iterates(cg, x, b, reference, dt, read=None):
    """begin, then iterate(1) six times: x against the float64 reference after each"""
    read = read or x.to_host
    cg.begin(x, b, 0.0, 1000)
    worst = 0.0
    for k, (it, status, _, want) in zip(range(7), reference):
        if k:
            cg.iterate(1)
            worst = max(worst, rel(read(), want))
        info = cg.status()
        assert (info.iterations, info.status) == (it, status) == (k, 0)
    print(f"largest relative difference of six iterates: {worst:.3e} (tolerance {ITERATE_TOL[dt]:.0e})")
    assert worst <= ITERATE_TOL[dt]
    return worst


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["double", "float"])
@pytest.mark.parametrize("kind", ["none", "jacobi", "chebyshev"])
@pytest.mark.parametrize("m", [(2, 2, 8), (3, 2, 4), (3, 4, 3)])
def test_iterates_match_reference(m, kind, dt):
    P = problem(*m)
    b = P.rhs(0)
    cg = P.solver(kind, dt)
    x = mf.DeviceVector(P.N, NT[dt])
    check_six_iterates(cg, x, dv(b, dt), P.reference(kind, np.float64, b, 0.0, 1000), dt)


SOLVES = [((2, 2, 8), "jacobi"), ((3, 2, 4), "chebyshev"), ((3, 4, 3), "none"), ((3, 4, 3), "chebyshev"),
          ((3, 3, 4), "chebyshev")]


@pytest.mark.parametrize("dt,tol,bound", [(np.float64, 1e-10, 2e-10), (np.float32, 1e-4, 2e-4)], ids=["double", "float"])
@pytest.mark.parametrize("m,kind", SOLVES)
def test_solve_to_convergence(m, kind, dt, tol, bound):
    P = problem(*m)
    b = P.rhs(1)
    tolerance = tol * np.linalg.norm(b)
    hist = list(P.reference(kind, dt, b, tolerance, 10000))
    ref_it, ref_status, ref_res, _ = hist[-1]
    assert ref_status == 1 and ref_res <= tolerance < hist[-2][2]
    cg = P.solver(kind, dt)
    x = mf.DeviceVector(P.N, NT[dt])
    info = cg.solve(x, dv(b, dt), tolerance, 10000, check_every=5)
    true = np.linalg.norm(b - P.A @ x.to_host().astype(np.float64)) / np.linalg.norm(b)
    print(f"iterations {info.iterations} (reference {ref_it}), true residual {true:.3e} (bound {bound:.0e})")
    assert info.status == 1 and abs(int(info.iterations) - ref_it) <= 1
    assert info.residual <= tolerance and abs(info.initial_residual - np.linalg.norm(b.astype(dt))) <= 1e-6 * np.linalg.norm(b)
    assert true <= bound


# ---- freeze and chunking, on (3, 4, 3): the plane kernel, no atomics, so everything is bitwise reproducible
FREEZE = (3, 4, 3)


@pytest.mark.parametrize("kind", ["none", "jacobi", "chebyshev"])
def test_check_every_does_not_change_the_solve(kind):
    P = problem(*FREEZE)
    b = P.rhs(1)
    bd, tolerance = dv(b), 1e-10 * np.linalg.norm(b)
    cg = P.solver(kind, np.float64)
    results = []
    for check_every in (1, 7, 1000, 1000):  # the last two: two solves on the same inputs
        x = mf.DeviceVector(P.N)
        x.fill(np.nan)  # begin writes every entry
        info = cg.solve(x, bd, tolerance, 10000, check_every=check_every)
        results.append((x.to_host(), info.as_tuple()))
    assert results[0][1][1] == 1 and results[0][1][0] > 10
    for xh, info in results[1:]:
        assert np.array_equal(xh, results[0][0]) and info == results[0][1]


@pytest.mark.parametrize("kind", ["jacobi", "chebyshev"])
def test_chunking_and_iterations_past_the_end(kind):
    P = problem(*FREEZE)
    b = P.rhs(1)
    bd, tolerance = dv(b), 1e-10 * np.linalg.norm(b)
    cg = P.solver(kind, np.float64)
    x1, x6 = mf.DeviceVector(P.N), mf.DeviceVector(P.N)
    cg.begin(x1, bd, tolerance, 10000)
    for _ in range(6):
        cg.iterate(1)
    cg.begin(x6, bd, tolerance, 10000)
    cg.iterate(6)
    assert cg.status().as_tuple()[:2] == (6, 0)
    assert np.array_equal(x1.to_host(), x6.to_host())
    # on to convergence, then 50 more
    info = cg.status()
    while info.status == 0:
        cg.iterate(3)
        info = cg.status()
    assert info.status == 1
    xh = x6.to_host()
    cg.iterate(50)
    after = cg.status()
    assert after.as_tuple() == info.as_tuple() and np.array_equal(x6.to_host(), xh)


def test_max_iterations_and_zero_rhs():
    P = problem(*FREEZE)
    b = P.rhs(1)
    cg = P.solver("jacobi", np.float64)
    x = mf.DeviceVector(P.N)
    info = cg.solve(x, dv(b), 1e-10 * np.linalg.norm(b), 3, check_every=2)
    assert (info.iterations, info.status) == (3, 2)
    x3 = x.to_host()
    want = [h for h in P.reference("jacobi", np.float64, b, 0.0, 3)][-1]
    assert want[0] == 3 and want[1] == 2 and rel(x3, want[3]) <= 1e-12
    cg.iterate(4)  # frozen
    assert cg.status().as_tuple() == info.as_tuple() and np.array_equal(x.to_host(), x3)
    x.fill(np.nan)
    info = cg.solve(x, dv(np.zeros(P.N)), 1e-10, 100, check_every=3)
    assert (info.iterations, info.status, info.residual, info.initial_residual) == (0, 1, 0.0, 0.0)
    assert np.array_equal(x.to_host(), np.zeros(P.N))


def test_breakdown_freezes_with_status_3():
    # an infinite entry in b makes p.q NaN in the first iteration: nothing is written, the status is 3 and stays
    P = problem(2, 2, 8)
    b = P.rhs(0)
    b[5] = np.inf
    cg = P.solver("none", np.float64)
    x = mf.DeviceVector(P.N)
    cg.begin(x, dv(b), 1e-10, 100)
    cg.iterate(3)
    info = cg.status()
    assert (info.iterations, info.status) == (0, 3)
    assert np.array_equal(x.to_host(), np.zeros(P.N))


# ---- shapes that can go wrong
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["double", "float"])
@pytest.mark.parametrize("kind", ["jacobi", "chebyshev"])
def test_unaligned_vectors_take_the_scalar_path(kind, dt):
    P = problem(2, 2, 8)
    b = P.rhs(0)
    size = np.dtype(dt).itemsize
    xbuf, bbuf = mf.DeviceVector(P.N + 1, NT[dt]), dv(np.concatenate([[np.nan], b]), dt)
    xbuf.fill(7.0)
    cg = P.solver(kind, dt)
    check_six_iterates(cg, xbuf.ptr + size, bbuf.ptr + size, P.reference(kind, np.float64, b, 0.0, 1000), dt,
                       read=lambda: xbuf.to_host()[1:])
    assert xbuf.to_host()[0] == 7.0  # the element before the view is not touched


def test_grid_stride_and_all_partials():
    """1041^2 = 1 083 681 dofs > 2048 * 256 * 2: every block of the 2048 loops more than once over its 16-byte chunks and
    all 2048 partial sums are in use.  Three JACOBI iterations; the reference's matvec is op.vmult."""
    mesh = mf.Mesh.uniform(2, 2, 520)
    N = mesh.n_dofs
    assert N > 2048 * 256 * 2 and N % 2 == 1
    op = mf.Operator(mesh.desc, mesh)
    dinv_dev, src, dst = mf.DeviceVector(N), mf.DeviceVector(N), mf.DeviceVector(N)
    op.compute_inverse_diagonal(dinv_dev)
    dinv = dinv_dev.to_host()

    def matvec(v):
        src.from_host(v)
        op.vmult(dst, src)
        return dst.to_host()

    b = np.random.default_rng(0).standard_normal(N)
    b[mesh.arrays()["constrained_dofs"]] = 0.0
    cg = mf.CG(op, mf.CG_JACOBI, dinv_dev)
    x = mf.DeviceVector(N)
    cg.begin(x, dv(b), 0.0, 1000)
    for k, (it, status, res, want) in zip(range(4), ref.cg(matvec, b, lambda r: dinv * r, np.float64, 0.0, 1000)):
        if k:
            cg.iterate(1)
            assert rel(x.to_host(), want) <= 1e-12
        info = cg.status()
        assert (info.iterations, info.status) == (k, 0) and abs(info.residual - res) <= 1e-12 * res


# ---- callback
def test_callback_jacobi_matches_builtin():
    P = problem(3, 4, 3)
    b = P.rhs(0)
    op = P.op(np.float64)
    dinv = P.dinv_dev[np.float64]
    calls = []

    def jacobi(z, r, stream):
        calls.append(stream)
        z.equ(1.0, r, stream)
        z.scale(dinv, stream)

    cb = mf.CG(op, mf.CG_CALLBACK, callback=jacobi)
    builtin = P.solver("jacobi", np.float64)
    xc, xb, bd = mf.DeviceVector(P.N), mf.DeviceVector(P.N), dv(b)
    cb.begin(xc, bd, 0.0, 1000)
    builtin.begin(xb, bd, 0.0, 1000)
    for k in range(6):
        cb.iterate(1)
        builtin.iterate(1)
        assert rel(xc.to_host(), xb.to_host()) <= 1e-12
    assert len(calls) == 7 and cb.status().iterations == 6
    assert cb.memory_consumption() == 4 * P.N * 8 + mf.CG_PARTIAL_BYTES + mf.CG_STATE_BYTES


def test_callback_error_code_is_passed_through():
    P = problem(2, 2, 8)
    op = P.op(np.float64)
    rc = [0]
    cg = mf.CG(op, mf.CG_CALLBACK, callback=lambda z, r, stream: z.equ(1.0, r, stream) or rc[0])
    x = mf.DeviceVector(P.N)
    cg.begin(x, dv(P.rhs(0)), 0.0, 1000)
    cg.iterate(1)
    rc[0] = -1
    assert cg.iterate(1, check=False) == -1
    rc[0] = -7
    assert cg.iterate(2, check=False) == -7
    assert cg.begin(x, dv(P.rhs(0)), 0.0, 1000, check=False) == -7


# ---- graph capture
@pytest.mark.parametrize("kind", ["jacobi", "chebyshev"])
@pytest.mark.parametrize("m", [(2, 2, 32), (3, 4, 6)])
def test_begin_and_iterate_are_graph_capturable(m, kind):
    if torch is None:
        pytest.skip("torch is not installed")
    assert torch.cuda.is_available()
    mesh = mf.Mesh.uniform(*m)
    op = mf.Operator(mesh.desc, mesh)
    N = mesh.n_dofs
    dev = torch.device("cuda", 0)
    bh = np.random.default_rng(0).standard_normal(N)
    bh[mesh.arrays()["constrained_dofs"]] = 0.0
    b = torch.from_numpy(bh).to(dev)
    x = torch.zeros(N, device=dev, dtype=torch.float64)
    dinv = torch.zeros(N, device=dev, dtype=torch.float64)
    op.compute_inverse_diagonal(dinv)
    torch.cuda.synchronize()
    # lambda_max of D^-1 A by a few power iterations on the host side of the device operator, enlarged by 20 %
    v, w = torch.ones(N, device=dev, dtype=torch.float64), torch.zeros(N, device=dev, dtype=torch.float64)
    lam = 1.0
    for _ in range(20):
        op.vmult(w, v, torch.cuda.current_stream().cuda_stream)
        w *= dinv
        lam = float(w.norm() / v.norm())
        v = w / w.norm()
    cg = mf.CG(op, KIND[kind], dinv, DEGREE, 1.2 * lam, RANGE)

    def run(stream):
        cg.begin(x, b, 0.0, 1000, stream)
        cg.iterate(8, stream)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run(s.cuda_stream)
    torch.cuda.synchronize()
    want = x.cpu().numpy()
    assert cg.status().as_tuple()[:2] == (8, 0) and np.linalg.norm(want) > 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        x.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert cg.status().as_tuple()[:2] == (8, 0)
        assert np.linalg.norm(x.cpu().numpy() - want) <= 1e-13 * np.linalg.norm(want)


# ---- memory
@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["double", "float"])
@pytest.mark.parametrize("kind,n_vectors", [("none", 3), ("jacobi", 3), ("chebyshev", 7)])
def test_memory_consumption(kind, n_vectors, dt):
    """r, p, q (+ z and the sweep's three vectors for CHEBYSHEV) + 3 x 2048 partial sums + the 128-byte state block"""
    P = problem(3, 4, 3)
    P.op(dt)
    x, b = mf.DeviceVector(P.N, NT[dt]), dv(P.rhs(1), dt)

    def cycle():
        cg = P.solver(kind, dt)
        assert cg.memory_consumption() == n_vectors * P.N * np.dtype(dt).itemsize + mf.CG_PARTIAL_BYTES + mf.CG_STATE_BYTES
        assert cg.solve(x, b, 1e-3 * np.linalg.norm(P.rhs(1)), 100).status == 1
        cg.destroy()
        mf.synchronize()

    cycle()  # (the first use of a kernel loads its code object: not the solver's memory)
    free0, _ = mf.device_memory_info()
    cycle()
    free1, _ = mf.device_memory_info()
    assert free1 == free0, (free0, free1)


# ---- argument checks that need a device
def test_argument_checks():
    P = problem(2, 2, 8)
    op = P.op(np.float64)
    dinv = P.dinv_dev[np.float64]
    for args in [(mf.CG_JACOBI, None, 0, 0.0, 0.0), (mf.CG_CHEBYSHEV, None, 5, 2.0, 15.0),
                 (mf.CG_CHEBYSHEV, dinv, 0, 2.0, 15.0), (mf.CG_CHEBYSHEV, dinv, 5, 0.0, 15.0),
                 (mf.CG_CHEBYSHEV, dinv, 5, -2.0, 15.0), (mf.CG_CHEBYSHEV, dinv, 5, 2.0, 1.0), (4, dinv, 5, 2.0, 15.0),
                 (-1, dinv, 5, 2.0, 15.0)]:
        with pytest.raises(mf.MfgpuError, match="error -1"):
            mf.CG(op, *args)
    x, b = mf.DeviceVector(P.N), dv(P.rhs(0))
    cg = P.solver("jacobi", np.float64)
    assert cg.iterate(1, check=False) == mf.EINVAL  # before begin
    with pytest.raises(mf.MfgpuError, match="error -1.*begin"):
        cg.status()
    x.fill(3.0)
    assert cg.begin(None, b, 1e-10, 10, check=False) == mf.EINVAL
    assert cg.begin(x, None, 1e-10, 10, check=False) == mf.EINVAL
    assert cg.begin(x, x, 1e-10, 10, check=False) == mf.EINVAL
    big = mf.DeviceVector(2 * P.N)
    big.fill(3.0)
    assert cg.begin(big.ptr + 8 * (P.N - 1), big, 1e-10, 10, check=False) == mf.EINVAL  # one element overlaps
    assert cg.iterate(1, check=False) == mf.EINVAL  # none of those began a solve
    assert np.all(x.to_host() == 3.0) and np.all(big.to_host() == 3.0)  # nothing written
    assert cg.begin(big.ptr + 8 * P.N, big, 1e-10, 10, check=False) == mf.OK  # adjacent is fine
    info = mf.CGInfo()
    assert mf.lib().mfgpu_cg_solve(cg._h, x.ptr, b.ptr, 1e-10, 10, 0, None, info) == mf.EINVAL  # check_every 0
    assert mf.lib().mfgpu_cg_status(cg._h, None, None) == mf.EINVAL
    # callback solvers
    cb = mf.CG(op, mf.CG_CALLBACK)
    assert cb.begin(x, b, 1e-10, 10, check=False) == mf.EINVAL  # no callback set
    assert mf.lib().mfgpu_cg_set_callback(cb._h, mf.CG_CALLBACK_TYPE(0), None) == mf.EINVAL
    with pytest.raises(mf.MfgpuError, match="error -1"):
        cg.set_callback(lambda z, r, s: 0)  # not a CALLBACK solver
    assert np.all(x.to_host() == 3.0)


# ---- drivers
def _run(exe, args):
    out = subprocess.run([os.path.join(BIN, exe)] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return [ln.split() for ln in out.stdout.strip().splitlines()]


@pytest.mark.parametrize("exe,args", [("poisson-3d-p4", ["-q", "0", "1"]), ("poisson-2d-p2", ["-q", "0", "2"]),
                                      ("poisson-3d-p2-ball", ["-q", "0", "1"])])
def test_poisson_devcg_drivers(exe, args):
    """dim  degree  n_dofs  iterations  wall_seconds  l2_error: same lines, iteration counts within one, L2 errors to 1e-8"""
    host, device = _run(exe, args), _run(exe + "-devcg", args)
    assert len(host) == len(device) >= 2
    for h, d in zip(host, device):
        assert len(h) == len(d) == 6 and h[:3] == d[:3]
        print(f"{exe} {h[2]} dofs: iterations {h[3]} host loop, {d[3]} device; L2 error {h[5]} / {d[5]}")
        assert abs(int(h[3]) - int(d[3])) <= 1
        assert abs(float(h[5]) - float(d[5])) <= 1e-8 * float(h[5])


def test_poisson_mg_devcg_driver():
    """dim  degree  n_dofs  levels  cg_iterations  wall_seconds  rel_error.  The V-cycle runs through the solver's callback.
    This driver's error column is |x - x*| / |x*| of a solve to 1e-12 |b| -- rounding noise around 1e-13, already relative
    to the solution -- so the two columns agree to 1e-8 of the solution, not of each other."""
    for arg in ("2", "3"):
        (h,), (d,) = _run("poisson-mg-3d-p4", [arg]), _run("poisson-mg-3d-p4-devcg", [arg])
        assert len(h) == len(d) == 7 and h[:4] == d[:4]
        print(f"poisson-mg-3d-p4 {arg}: iterations {h[4]} host loop, {d[4]} device; rel_error {h[6]} / {d[6]}")
        assert abs(int(h[4]) - int(d[4])) <= 1
        assert abs(float(h[6]) - float(d[6])) <= 1e-8
