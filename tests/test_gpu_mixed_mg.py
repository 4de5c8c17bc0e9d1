"""Mixed-precision multigrid and the fused Chebyshev smoother (include/mfgpu.h, csrc/mfgpu_mixed.hip; DESIGN.md
§10) on the GPU:
  - mfgpu_vec_convert bitwise against numpy's astype in both directions (values beyond the float range included) and
    mfgpu_vec_copy_pairs_convert on the copy pairs of a real adaptive hierarchy against numpy fancy indexing;
  - mfgpu_vec_chebyshev_start / _update against a numpy restatement of their formulas, and a degree-5 Chebyshev
    smoothing on a level operator against the BLAS-1 sequence of PreconditionChebyshev::run (host/mfgpu_shim_mg.h);
  - the poisson-mg drivers with float levels under the double CG (-mixed) and with the fused smoother (-fused), at the
    arguments of tests/test_gpu_transfer.py::test_poisson_mg_driver_binaries."""
import os
import subprocess

import numpy as np
import pytest

import pymfgpu as mf

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 3, 64, 65, 1_000_003]


def _dev(a, nt):
    v = mf.DeviceVector(a.size, nt)
    if a.size:
        v.from_host(a)
    return v


def _host(v):
    return v.to_host() if v.n else np.zeros(0, dtype=mf.np_dtype(v.number_type))


def _values(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)
    special = np.array([1e39, -1e39, 1e300, -1e300, 3.4028235677973366e38, 3.4028236e38, 1e-40, -1e-45, 0.0, -0.0,
                        np.inf, -np.inf, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24])
    k = min(n, special.size)
    x[:k] = special[:k]
    return x


@pytest.mark.parametrize("n", SIZES)
def test_vec_convert_is_numpy_astype(n):
    x64 = _values(n, n)
    with np.errstate(over="ignore"):
        want32 = x64.astype(np.float32)
    src = _dev(x64, mf.F64)
    dst = mf.DeviceVector(n, mf.F32)
    mf.vec_convert(dst, mf.F32, src, mf.F64, n)
    mf.synchronize()
    got32 = _host(dst)
    np.testing.assert_array_equal(got32.view(np.uint32), want32.view(np.uint32))
    # float -> double is exact
    back = mf.DeviceVector(n, mf.F64)
    mf.vec_convert(back, mf.F64, dst, mf.F32, n)
    mf.synchronize()
    np.testing.assert_array_equal(_host(back).view(np.uint64), want32.astype(np.float64).view(np.uint64))
    # same type: a copy
    cp = mf.DeviceVector(n, mf.F64)
    mf.vec_convert(cp, mf.F64, src, mf.F64, n)
    mf.synchronize()
    np.testing.assert_array_equal(_host(cp).view(np.uint64), x64.view(np.uint64))
    if n > 4:  # vectors that are not 16-byte aligned take the scalar path
        dst.fill(5.0)
        mf.vec_convert(dst.ptr + 4, mf.F32, src.ptr + 8, mf.F64, n - 1)
        mf.synchronize()
        got = _host(dst)
        assert got[0] == 5.0
        np.testing.assert_array_equal(got[1:].view(np.uint32), want32[1:].view(np.uint32))


def test_vec_convert_rejects_bad_types():
    a, b = mf.DeviceVector(8, mf.F64), mf.DeviceVector(8, mf.F32)
    assert mf.vec_convert(b, 2, a, mf.F64, 8, check=False) == mf.EINVAL
    assert mf.vec_convert(b, mf.F32, a, -1, 8, check=False) == mf.EINVAL


@pytest.mark.parametrize("dim,p,nref", [(2, 2, 4), (3, 2, 3), (3, 4, 3)])
def test_copy_pairs_convert_on_hierarchy_pairs(dim, p, nref):
    mesh = mf.Mesh.adaptive_mg(dim, p, nref)
    H = mf.MgHierarchy(mesh)
    rng = np.random.default_rng(dim * 10 + p)
    act = rng.standard_normal(mesh.n_dofs)
    src = _dev(act, mf.F64)
    back = mf.DeviceVector(mesh.n_dofs, mf.F64)
    back.fill(-3.0)
    seen = np.zeros(mesh.n_dofs, dtype=bool)
    for l in range(H.n_levels):
        a, b = H.copy_pairs(l)
        nl = H.level_mesh(l).n_dofs
        # copy_to_mg: level (float) <- active (double)
        lev = mf.DeviceVector(nl, mf.F32)
        lev.fill(7.0)
        mf.copy_pairs_convert(mf.IndexPairs(b, a), lev, mf.F32, src, mf.F64)
        mf.synchronize()
        want = np.full(nl, 7.0, dtype=np.float32)
        want[b] = act[a].astype(np.float32)
        np.testing.assert_array_equal(lev.to_host(), want)
        # copy_from_mg: active (double) <- level (float), exact
        mf.copy_pairs_convert(mf.IndexPairs(a, b), back, mf.F64, lev, mf.F32)
        seen[a] = True
    mf.synchronize()
    want = np.full(mesh.n_dofs, -3.0)
    want[seen] = act[seen].astype(np.float32).astype(np.float64)
    np.testing.assert_array_equal(back.to_host(), want)


def _cheb_inputs(n, nt, seed):
    rng = np.random.default_rng(seed)
    dt = mf.np_dtype(nt)
    # positive data: no cancellation, so a per-entry relative bound is meaningful
    return {k: rng.uniform(lo, hi, n).astype(dt) for k, lo, hi in
            (("x", 1, 2), ("upd", 0.5, 1), ("r", 1, 2), ("b", 1, 2), ("t", 0, 0.5), ("dinv", 0.1, 1))}


def _close(got, want, tol):
    want = np.asarray(want, dtype=np.float64)
    assert np.all(np.abs(got.astype(np.float64) - want) <= tol * np.abs(want)), np.max(np.abs(got - want) / np.abs(want))


@pytest.mark.parametrize("nt,tol", [(mf.F64, 1e-14), (mf.F32, 1e-6)])
@pytest.mark.parametrize("n", SIZES)
def test_chebyshev_start_and_update_formulas(n, nt, tol):
    dt = mf.np_dtype(nt)
    f, f1, f2 = 0.37, 0.81, 1.23
    for zero_start in (True, False):
        for with_t in (True, False):
            h = _cheb_inputs(n, nt, n + 2 * zero_start + with_t)
            v = {k: _dev(a, nt) for k, a in h.items()}
            mf.chebyshev_start(v["x"], v["upd"], v["r"], v["b"], v["t"] if with_t else None, v["dinv"], f, zero_start,
                               n, nt)
            mf.synchronize()
            H = {k: a.astype(np.float64) for k, a in h.items()}
            r = H["b"] - H["t"] if with_t else H["b"]
            r = r.astype(dt).astype(np.float64)
            u = float(dt(f)) * r * H["dinv"]
            x = u if zero_start else H["x"] + u
            _close(_host(v["r"]), r, tol)
            _close(_host(v["upd"]), u, 4 * tol)
            _close(_host(v["x"]), x, 4 * tol)
    h = _cheb_inputs(n, nt, n + 7)
    v = {k: _dev(a, nt) for k, a in h.items()}
    mf.chebyshev_update(v["x"], v["upd"], v["r"], v["t"], v["dinv"], f1, f2, n, nt)
    mf.synchronize()
    H = {k: a.astype(np.float64) for k, a in h.items()}
    r = (H["r"] - H["t"]).astype(dt).astype(np.float64)
    u = float(dt(f1)) * H["upd"] + float(dt(f2)) * r * H["dinv"]
    _close(_host(v["r"]), r, tol)
    _close(_host(v["upd"]), u, 4 * tol)
    _close(_host(v["x"]), H["x"] + u, 4 * tol)
    if n > 4:  # misaligned by one element: the scalar path
        es = np.dtype(dt).itemsize
        v = {k: _dev(a, nt) for k, a in h.items()}
        mf.chebyshev_update(v["x"].ptr + es, v["upd"].ptr + es, v["r"].ptr + es, v["t"].ptr + es, v["dinv"].ptr + es,
                            f1, f2, n - 1, nt)
        mf.synchronize()
        got = _host(v["x"])
        assert got[0] == h["x"][0]
        _close(got[1:], (H["x"] + u)[1:], 4 * tol)


@pytest.mark.parametrize("nt", [mf.F64, mf.F32])
def test_chebyshev_calls_reject_aliasing(nt):
    n = 100
    x, u, r, b, t, d = (mf.DeviceVector(n, nt) for _ in range(6))
    assert mf.chebyshev_start(x, x, r, b, t, d, 1.0, True, n, nt, check=False) == mf.EINVAL
    assert mf.chebyshev_start(x, u, u, b, t, d, 1.0, True, n, nt, check=False) == mf.EINVAL
    assert mf.chebyshev_start(x, u, r, r, t, d, 1.0, True, n, nt, check=False) == mf.EINVAL
    assert mf.chebyshev_update(x, u, x, t, d, 1.0, 1.0, n, nt, check=False) == mf.EINVAL
    assert mf.chebyshev_update(x, r, r, t, d, 1.0, 1.0, n, nt, check=False) == mf.EINVAL
    assert mf.chebyshev_update(x, u, r, t, d, 1.0, 1.0, n, 5, check=False) == mf.EINVAL
    assert mf.chebyshev_update(x, u, r, t, d, 1.0, 1.0, 0, nt, check=False) == mf.OK


def _sweep(A, x, b, dinv, r, t, upd, lmax, degree, zero_start, fused, nt):
    """PreconditionChebyshev::run (host/mfgpu_shim_mg.h) as BLAS-1 calls or as the two fused calls"""
    n = b.n
    lmin = lmax / 15.0
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    rho = 1.0 / sigma
    if not zero_start:
        A.vmult(t, x)
    if fused:
        mf.chebyshev_start(x, upd, r, b, None if zero_start else t, dinv, 1.0 / theta, zero_start, n, nt)
    else:
        r.equ(1.0, b)
        if not zero_start:
            r.add(-1.0, t)
        upd.equ(1.0 / theta, r)
        upd.scale(dinv)
        if zero_start:
            x.equ(1.0, upd)
        else:
            x.add(1.0, upd)
    for _ in range(1, degree):
        A.vmult(t, upd)
        rho_new = 1.0 / (2.0 * sigma - rho)
        if fused:
            mf.chebyshev_update(x, upd, r, t, dinv, rho_new * rho, 2.0 * rho_new / delta, n, nt)
        else:
            r.add(-1.0, t)
            t.equ(2.0 * rho_new / delta, r)
            t.scale(dinv)
            upd.sadd(rho_new * rho, 1.0, t)
            x.add(1.0, upd)
        rho = rho_new


@pytest.mark.parametrize("nt,tol", [(mf.F64, 1e-13), (mf.F32, 1e-5)])
@pytest.mark.parametrize("kind", ["cube-p4", "ball-p2"])
def test_fused_smoothing_matches_blas1_sequence(kind, nt, tol):
    mesh = mf.Mesh.uniform(3, 4, 4, number_type=nt) if kind == "cube-p4" else mf.Mesh.ball(3, 2, 2, number_type=nt)
    A = mf.Level(mesh.desc, [], mesh)
    n = mesh.n_dofs
    dinv = mf.DeviceVector(n, nt)
    A.compute_inverse_diagonal(dinv)
    # lambda_max of D^-1 A by power iteration (as PreconditionChebyshev::initialize), +20 %
    v, w = _dev(np.sin(0.7 * np.arange(n)) + 0.3, nt), mf.DeviceVector(n, nt)
    lam = 1.0
    for _ in range(30):
        A.vmult(w, v)
        w.scale(dinv)
        nw, nv = w.l2_norm(), v.l2_norm()
        lam = nw / nv
        v.equ(1.0 / nw, w)
    lmax = 1.2 * lam
    rhs = np.random.default_rng(3).standard_normal(n)
    out = []
    for fused in (False, True):
        b = _dev(rhs, nt)
        A.vmult(w, b)  # a right-hand side in the range of A (Dirichlet rows included)
        b.equ(1.0, w)
        x, r, t, upd = (mf.DeviceVector(n, nt) for _ in range(4))
        _sweep(A, x, b, dinv, r, t, upd, lmax, 5, True, fused, nt)   # pre-smoothing from zero
        _sweep(A, x, b, dinv, r, t, upd, lmax, 5, False, fused, nt)  # one more sweep on the iterate
        mf.synchronize()
        out.append(x.to_host().astype(np.float64))
    err = np.linalg.norm(out[1] - out[0]) / np.linalg.norm(out[0])
    print(f"{kind} nt={nt}: fused vs BLAS-1 rel l2 {err:.2e}")
    assert np.all(np.isfinite(out[1])) and err <= tol, err


# ---- drivers
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dealii-cuda_amd", "host", "bin")


def _drive(exe, arg, ncols):
    out = subprocess.run([os.path.join(BIN, exe), arg], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, exe + " " + arg + ": " + out.stdout + out.stderr
    f = out.stdout.split()
    assert len(f) == ncols, out.stdout
    assert float(f[6]) < 1e-8, out.stdout
    return f


def test_mixed_and_fused_poisson_mg_drivers():
    """every -mixed target and -fused at the arguments of test_poisson_mg_driver_binaries: converged to the same
    answer, CG iterations at most 2 above the double target's, the same level-independence bounds"""
    cases = {"poisson-mg-2d-p2": ("5", "7"), "poisson-mg-3d-p4": ("3", "4"), "poisson-mg-3d-p2-ball": ("3",),
             "poisson-mg-2d-p2-adaptive": ("4", "6"), "poisson-mg-3d-p4-adaptive": ("4", "5")}
    its, mg_bytes = {}, {}
    for base, args in cases.items():
        variants = [base + "-mixed"] + (["poisson-mg-3d-p4-fused"] if base == "poisson-mg-3d-p4" else [])
        for arg in args:
            ref = _drive(base, arg, 7)
            for exe in variants:
                f = _drive(exe, arg, 9)
                assert f[:4] == ref[:4], (exe, arg, f, ref)  # dim, degree, n_dofs, levels
                assert int(f[4]) <= int(ref[4]) + 2, (exe, arg, f[4], ref[4])
                assert int(f[7]) > 0 and float(f[8]) > 0
                its[(exe, arg)] = int(f[4])
                mg_bytes[(exe, arg)] = int(f[7])
                print(f"{exe} {arg}: {f[4]} iterations (double levels, unfused: {ref[4]}), mg_bytes {f[7]}, "
                      f"vcycle {f[8]} ms")
    for exe in ("poisson-mg-3d-p4-mixed", "poisson-mg-3d-p4-fused"):
        assert its[(exe, "4")] <= its[(exe, "3")] + 2 <= 16
    assert its[("poisson-mg-2d-p2-mixed", "7")] <= its[("poisson-mg-2d-p2-mixed", "5")] + 2 <= 16
    assert its[("poisson-mg-3d-p2-ball-mixed", "3")] <= 30
    for exe, (a, b) in (("poisson-mg-2d-p2-adaptive-mixed", ("4", "6")), ("poisson-mg-3d-p4-adaptive-mixed", ("4", "5"))):
        assert its[(exe, b)] <= its[(exe, a)] + 3 <= 18
    ratio = mg_bytes[("poisson-mg-3d-p4-mixed", "4")] / mg_bytes[("poisson-mg-3d-p4-fused", "4")]
    print(f"mg_bytes float / double levels, poisson-mg-3d-p4 4: {ratio:.3f}")
    assert ratio < 1.0
