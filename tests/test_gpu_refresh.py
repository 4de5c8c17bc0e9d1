"""mfgpu_vcycle_refresh (pymfgpu.VCycle.refresh) and the enqueue-only set-up calls under it, against
the by-value / host forms they stand in for and against the parent route, a fresh VCycle on the same updated levels.

  1. chebyshev_start_dev / chebyshev_update_dev == the by-value forms, bitwise; chebyshev_scalars_dev against the host's
  2. estimate_lambda_max_enqueue against estimate_lambda_max: status, step count, value
  3. spd_inverse_enqueue against spd_inverse
  4. a refreshed object is the fresh object (estimated and given lambda_max, dense and CG coarse solve, two coefficients)
  5. CG preconditioned by the refreshed V-cycle, hanging nodes included
  6. a graph of {level updates, refresh, apply} replayed on a new coefficient
  7. memory: the documented growth at the first refresh, nothing after it, every byte back
  8. MFGPU_EUNSUPPORTED above the device inverse's cap, a null object, a level-0 matrix that is no longer positive definite

Tolerances that are conditions: the scalars of chebyshev_scalars_dev lie within 4 eps of the host's (the same recurrence in
IEEE double); lambda_max within 64 eps of the level type of the host estimate (the bound of
test_gpu_vcycle.py::test_eigenvalue_estimate for the same iteration run twice).
Tolerances that are measurements (MI355X; the largest value over the cases and two runs of the test; times 10; the
restriction's and the diagonal's atomics land in another order every run):
  device inverse, |inv_dev - inv_host|_F / |inv_host|_F, lda = n and n + 3 alike:
      n = 1: 0, 2: 5.1e-16, 9: 2.1e-15, 63: 1.07e-14, 64: 1.06e-14, 65: 1.62e-14, 125: 1.47e-14, 343: 2.15e-14,
      512: 2.54e-14                                                                          -> 2.6e-13 (cap 1e-9)
  refreshed against fresh V-cycle, relative l2 difference of z, double levels / float levels (estimated and given
  lambda_max, first and second coefficient):
      cube_3d_p4         dense 3.8e-16 / 2.1e-7   CG 3.6e-16 / 1.9e-7
      ball_3d_p2         dense 3.0e-16 / 1.5e-7   CG 3.9e-13 / 1.7e-7
      adaptive_3d_p2_r4  dense 3.7e-16 / 2.3e-7   CG 4.6e-16 / 2.1e-7
      the CG solutions 2.8e-16, the graph replays 2.6e-16                                    -> 4.0e-12 / 2.4e-6 (caps 1e-9 / 1e-4)
  (the ball's coarse CG, 79 dofs, ends by its relative tolerance of 1e-10, the other two at rounding level; presumably
  that is why the rounding-level differences of its right-hand side between the two objects show at this scale)
Measured and not a tolerance: the device estimate differed from the host's by at most 4.8e-16 relative (double and float
levels), with the host's step count on every level."""
import functools

import numpy as np
import pytest
import scipy.sparse.linalg as spla

try:
    import torch  # before the library is loaded: libmfgpu.so binds to the HIP runtime torch brings (as in bench.py)
except ImportError:
    torch = None

import pymfgpu as mf
import vcycle_reference as vr
from oracle import mf_oracle as o
from util import oracle_desc_from_mesh

pytestmark = pytest.mark.gpu

F64, F32 = mf.F64, mf.F32
NTNAME = {F64: "double", F32: "float"}
SPD_TOL = 2.6e-13  # 10 x the largest measured value (docstring); the cap is 1e-9
REFRESH_TOL = {F64: 4.0e-12, F32: 2.4e-6}  # the same; the caps are 1e-9 / 1e-4
assert SPD_TOL <= 1e-9 and REFRESH_TOL[F64] <= 1e-9 and REFRESH_TOL[F32] <= 1e-4
COARSE = {"dense": mf.VCYCLE_COARSE_DENSE, "cg": mf.VCYCLE_COARSE_CG}


def eps(nt):
    return float(np.finfo(mf.np_dtype(nt)).eps)


def typed(a, nt):
    return np.asarray(a).astype(mf.np_dtype(nt)).astype(np.float64)


def dev(a, nt=F64):
    a = np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=mf.np_dtype(nt))
    v = mf.DeviceVector(a.size, nt)
    v.from_host(a)
    return v


def rel(got, want):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / np.linalg.norm(want))


# ---- 1. the _dev Chebyshev forms


def offset_views(arrays, offset, n, nt):
    """device copies of the arrays and views of n elements `offset` elements into them (offset 1: not 16-byte aligned)"""
    es = np.dtype(mf.np_dtype(nt)).itemsize
    store = [dev(a, nt) for a in arrays]
    return store, [mf.DeviceVector.view(v.ptr + offset * es, n, nt) for v in store]


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float"])
@pytest.mark.parametrize("zero_start", [0, 1], ids=["x+=", "x="])
@pytest.mark.parametrize("with_t", [False, True], ids=["b", "b-t"])
@pytest.mark.parametrize("n,offset", [(1, 0), (255, 0), (4097, 0), (1, 1), (255, 1), (4097, 1)])
def test_chebyshev_start_dev_equals_by_value(n, offset, with_t, zero_start, nt):
    rng = np.random.default_rng(n + offset)
    x, upd, r, b, t, dinv = (rng.standard_normal(n + offset) for _ in range(6))
    f = 0.3712345678901234  # not a float
    table = dev([9.0, f], F64)
    got = []
    for form in ("value", "dev"):
        store, (xv, uv, rv, bv, tv, dv) = offset_views([x, upd, r, b, t, dinv], offset, n, nt)
        if form == "value":
            mf.chebyshev_start(xv, uv, rv, bv, tv if with_t else None, dv, f, zero_start, n, nt)
        else:
            mf.chebyshev_start_dev(xv, uv, rv, bv, tv if with_t else None, dv, table.ptr + 8, zero_start, n, nt)
        mf.synchronize()
        got.append([v.to_host() for v in store[:3]])
    for a, b_, first in zip(got[0], got[1], (x, upd, r)):
        np.testing.assert_array_equal(a, b_)
        np.testing.assert_array_equal(b_[:offset], first[:offset].astype(b_.dtype))  # nothing written in front of the view
    assert np.abs(got[1][1][offset:] - upd[offset:].astype(got[1][1].dtype)).max() > 0  # something was computed
    assert mf.chebyshev_start_dev(xv, uv, rv, bv, None, dv, None, 1, n, nt, check=False) == mf.EINVAL
    assert mf.chebyshev_start_dev(xv, xv, rv, bv, None, dv, table, 1, n, nt, check=False) == mf.EINVAL


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float"])
@pytest.mark.parametrize("n,offset", [(1, 0), (255, 0), (4097, 0), (1, 1), (255, 1), (4097, 1)])
def test_chebyshev_update_dev_equals_by_value(n, offset, nt):
    rng = np.random.default_rng(2 * n + offset)
    x, upd, r, t, dinv = (rng.standard_normal(n + offset) for _ in range(5))
    f1, f2 = 0.1234567890123456, 1.8765432109876543
    table = dev([f1, f2], F64)
    got = []
    for form in ("value", "dev"):
        store, (xv, uv, rv, tv, dv) = offset_views([x, upd, r, t, dinv], offset, n, nt)
        if form == "value":
            mf.chebyshev_update(xv, uv, rv, tv, dv, f1, f2, n, nt)
        else:
            mf.chebyshev_update_dev(xv, uv, rv, tv, dv, table, n, nt)
        mf.synchronize()
        got.append([v.to_host() for v in store[:3]])
    for a, b_, first in zip(got[0], got[1], (x, upd, r)):
        np.testing.assert_array_equal(a, b_)
        np.testing.assert_array_equal(b_[:offset], first[:offset].astype(b_.dtype))
    assert np.abs(got[1][0][offset:] - x[offset:].astype(got[1][0].dtype)).max() > 0
    assert mf.chebyshev_update_dev(xv, uv, rv, tv, dv, None, n, nt, check=False) == mf.EINVAL
    assert mf.chebyshev_update_dev(xv, uv, rv, rv, dv, table, n, nt, check=False) == mf.EINVAL


@pytest.mark.parametrize("degree", [1, 2, 5])
def test_chebyshev_scalars_dev(degree):
    lam, rng_ = 1.9876543210123, 15.0
    want = mf.cg_chebyshev_scalars(degree, lam, rng_)
    lam_dev, f_dev = dev([lam]), dev(np.full(2 * degree + 1, np.nan))
    mf.chebyshev_scalars_dev(degree, lam_dev, rng_, f_dev)
    mf.synchronize()
    got = f_dev.to_host()
    assert np.isnan(got[2 * degree - 1:]).all()  # nothing past the table
    err = np.abs(got[:2 * degree - 1] - want) / np.abs(want)
    print(f"chebyshev_scalars_dev degree {degree}: largest relative difference {err.max():.3e}")
    assert err.max() <= 4 * eps(F64)
    assert mf.chebyshev_scalars_dev(0, lam_dev, rng_, f_dev, check=False) == mf.EINVAL
    assert mf.chebyshev_scalars_dev(degree, lam_dev, 1.0, f_dev, check=False) == mf.EINVAL


# ---- 2. the device power iteration


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float"])
@pytest.mark.parametrize("args", [(2, 2, 3), (3, 2, 4)], ids=["adaptive_2d_p2_r3", "adaptive_3d_p2_r4"])
def test_device_power_iteration(args, nt):
    mesh = mf.Mesh.adaptive_mg(*args, number_type=nt)
    levels, keep = mf.VCycle.hierarchy_levels(mesh)
    for l, lev in enumerate(levels):
        n = lev["n_dofs"]
        dinv = mf.DeviceVector(n, nt)
        lev["op"].compute_inverse_diagonal(dinv)
        want, want_steps = mf.estimate_lambda_max(lev["op"], dinv, 15, with_steps=True)
        bytes_ = mf.eig_workspace_bytes(n, nt)
        ws = mf.DeviceVector(bytes_ // 8 + 2)  # two doubles more: nothing may be written past the workspace
        ws.fill(-7.0)
        mf.estimate_lambda_max_enqueue(lev["op"], dinv, 15, 200, ws)
        mf.synchronize()
        r = mf.eig_result(ws)
        print(f"{args} level {l} {NTNAME[nt]}: device {r.lambda_max:.15e} in {r.steps} steps (status {r.status}), host "
              f"{want:.15e} in {want_steps}; relative difference {abs(r.lambda_max - want) / want:.2e}")
        assert r.status == 1 and r.steps == want_steps
        assert r.lambda_max == 1.2 * r.estimate
        np.testing.assert_allclose(r.lambda_max, want, rtol=64 * eps(nt), atol=0.0)
        np.testing.assert_array_equal(ws.to_host()[bytes_ // 8:], [-7.0, -7.0])
        mf.estimate_lambda_max_enqueue(lev["op"], dinv, 15, 3, ws)
        mf.synchronize()
        r3 = mf.eig_result(ws)
        assert (r3.status, r3.steps) == (2, 3) and r3.lambda_max == 1.2 * r3.estimate
    assert mf.estimate_lambda_max_enqueue(levels[0]["op"], dinv, 15, 0, ws, check=False) == mf.EINVAL
    assert mf.estimate_lambda_max_enqueue(levels[0]["op"], dinv, 15, 3, ws.ptr + 8, check=False) == mf.EINVAL


# ---- 3. the device inverse


@functools.lru_cache(maxsize=None)
def spd_case(n):
    """Q diag(d) Q^T with d log-spaced in [1, 1e3], and the host's inverse"""
    rng = np.random.default_rng(n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0.0, 3.0, n)) @ Q.T
    A = 0.5 * (A + A.T)
    return A, mf.spd_inverse(A)


def device_inverse(A, lda, ld, prefill=np.nan):
    n = A.shape[0]
    padded = np.full((n, lda), 123.0)
    padded[:, :n] = A
    a, inv = dev(padded), dev(np.full(n * ld, prefill))
    ws = mf.DeviceVector(mf.spd_inverse_workspace_bytes(n) // 8)
    status = dev([-1.0])
    mf.spd_inverse_enqueue(n, a, lda, inv, ld, ws, status)
    mf.synchronize()
    return inv.to_host().reshape(n, ld), int(status.to_host().view(np.uint32)[0])


@pytest.mark.parametrize("pad", [0, 3], ids=["lda=n", "lda=n+3"])
@pytest.mark.parametrize("n", [1, 2, 9, 63, 64, 65, 125, 343, 512])
def test_device_spd_inverse(n, pad):
    A, want = spd_case(n)
    ld = n + n % 2
    got, status = device_inverse(A, n + pad, ld)
    again, _ = device_inverse(A, n + pad, ld)
    assert status == 0
    np.testing.assert_array_equal(got, again)  # no atomics: equal bits
    if ld > n:
        np.testing.assert_array_equal(got[:, n:], 0.0)
    err = np.linalg.norm(got[:, :n] - want) / np.linalg.norm(want)
    print(f"device SPD inverse n = {n}, lda = {n + pad}: |inv_dev - inv_host|_F / |inv_host|_F = {err:.3e}")
    assert err <= SPD_TOL
    np.testing.assert_array_equal(got[:, :n], got[:, :n].T)


def test_device_spd_inverse_refuses_an_indefinite_matrix():
    n = 65
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.logspace(0.0, 3.0, n)
    d[n // 2] = -1.0
    A = (Q * d) @ Q.T
    got, status = device_inverse(0.5 * (A + A.T), n, n + 1, prefill=-3.25)
    assert status == 1
    np.testing.assert_array_equal(got, -3.25)
    assert mf.spd_inverse(A, check=False)[0] == mf.EINVAL  # (the host refuses it too)
    one = dev([1.0])
    assert mf.spd_inverse_enqueue(0, one, 0, one, 0, one, one, check=False) == mf.EINVAL
    assert mf.spd_inverse_enqueue(513, one, 513, one, 514, one, one, check=False) == mf.EINVAL


# ---- 4. a refreshed object is the fresh object

HIERARCHIES = ["cube_3d_p4", "ball_3d_p2", "adaptive_3d_p2_r4"]
UPD = mf.UPDATABLE_COEFFICIENTS


def field(k):
    """smooth positive coefficients at quadrature points x [..., dim]"""
    def a(x):
        x, y, z = x[..., 0], x[..., 1], x[..., 2]
        if k == 1:
            return 1.0 + x * x + 2.0 * y * y + 3.0 * z * z
        if k == 2:
            return 2.0 + np.sin(3.0 * x) + 0.5 * y * y + np.cos(2.0 * z)
        return 3.0 + x * y - 0.5 * z + np.sin(x + 2.0 * y) ** 2
    return a


def make_levels(name, nt):
    """(levels, keep, level meshes, active mesh) with MFGPU_UPDATABLE_COEFFICIENTS on every level"""
    if name.startswith("adaptive"):
        mesh = mf.Mesh.adaptive_mg(3, 2, 4, number_type=nt)
        levels, keep = mf.VCycle.hierarchy_levels(mesh, flags=UPD)
        return levels, keep, keep[2], mesh
    meshes = vr.cube_meshes(3, 4, (1, 2, 4), nt) if name == "cube_3d_p4" else vr.ball_meshes(3, 2, (0, 1, 2), nt)
    levels = [{"op": mf.Operator(mf.VCycle._flagged(M.desc, UPD), M), "n_dofs": M.n_dofs,
               "transfer": mf.Transfer.from_meshes(meshes[l - 1], M) if l else None} for l, M in enumerate(meshes)]
    return levels, meshes, meshes, meshes[-1]


def set_coefficient(levels, meshes, nt, k, mass=None):
    """the coefficient field k on every level, evaluated in numpy at that level's quadrature points"""
    for lev, M in zip(levels, meshes):
        c = field(k)(M.arrays()["quadrature_points"].astype(np.float64))
        lev["op"].update_coefficients(dev(c, nt), mass)
    mf.synchronize()  # the device arrays are read when the stream gets there


def defects(active, seed):
    """three seeded defects that a float holds, zero on the constrained dofs"""
    N = active.n_dofs
    R = typed(np.random.default_rng(seed).standard_normal((N, 3)), F32)
    R[active.arrays()["constrained_dofs"]] = 0.0
    return R


def apply_all(V, R):
    z = mf.DeviceVector(R.shape[0], F64)
    out = []
    for k in range(R.shape[1]):
        z.fill(np.nan)
        V.apply(z, dev(R[:, k]))
        mf.synchronize()
        out.append(z.to_host())
        assert np.isfinite(out[-1]).all()
    return np.stack(out, axis=1)


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float_levels"])
@pytest.mark.parametrize("mode", ["estimated-dense", "given-dense", "estimated-cg"])
@pytest.mark.parametrize("name", HIERARCHIES)
def test_refreshed_is_fresh(name, mode, nt):
    levels, keep, meshes, active = make_levels(name, nt)
    coarse = COARSE[mode.split("-")[1]]
    N, nl = active.n_dofs, len(levels)
    given = None
    if mode.startswith("given"):
        given = mf.VCycle(levels, F64, N, coarse=coarse, keep=keep).lambda_max()  # valid bounds, those of the first field
    V = mf.VCycle(levels, F64, N, lambda_max=given, coarse=coarse, keep=keep)
    lam0 = V.lambda_max()
    R = defects(active, len(name))
    errs = []
    for k in (1, 2):  # a second refresh after a second coefficient is again the fresh object
        set_coefficient(levels, meshes, nt, k)
        stale = apply_all(V, R)
        V.refresh(eig_steps=200)
        assert np.array_equal(V.lambda_max(), lam0)  # until refresh_status: the previous values
        info = V.refresh_status()
        W = mf.VCycle(levels, F64, N, lambda_max=given, coarse=coarse, keep=keep)  # the parent commit's route
        want = apply_all(W, R)
        got = apply_all(V, R)
        assert info.coarse_status == 0
        if given is None:
            assert info.eig_status_max == 1 and 15 <= info.eig_steps_max <= 200
            # levels above 0: level 0 has no smoother and keeps its creation value
            np.testing.assert_allclose(V.lambda_max()[1:], W.lambda_max()[1:], rtol=64 * eps(nt), atol=0.0)
            assert np.array_equal(V.lambda_max()[:1], lam0[:1])
        else:
            assert (info.eig_status_max, info.eig_steps_max) == (0, 0)
            np.testing.assert_array_equal(V.lambda_max(), given)  # values and scalars are kept
        err = max(rel(got[:, j], want[:, j]) for j in range(3))
        moved = min(rel(stale[:, j], want[:, j]) for j in range(3))
        print(f"refresh {name} {mode} {NTNAME[nt]} levels, field {k}: refreshed against fresh, largest rel l2 of 3: "
              f"{err:.3e}; before the refresh {moved:.3e}")
        errs.append(err)
        assert moved > 100 * REFRESH_TOL[nt]  # otherwise the coefficient change proves nothing
        lam0 = V.lambda_max()
    assert max(errs) <= REFRESH_TOL[nt], errs


# ---- 5. CG with the refreshed V-cycle


def test_cg_with_the_refreshed_vcycle():
    levels, keep, meshes, mesh = make_levels("adaptive_3d_p2_r4", F64)
    N = mesh.n_dofs
    od = oracle_desc_from_mesh(mesh)
    assert od.constraint_mask is not None and od.constraint_mask.any()  # hanging nodes
    a2 = field(1)(mesh.arrays()["quadrature_points"].astype(np.float64))
    od.coefficient = np.ascontiguousarray(a2).reshape(od.coefficient.shape)
    A = o.assemble(od).tocsr()
    op = mf.Operator(mf.VCycle._flagged(mesh.desc, UPD), mesh)
    V = mf.VCycle(levels, F64, N, keep=keep)  # on the first coefficient
    op.update_coefficients(dev(a2))
    set_coefficient(levels, meshes, F64, 1)
    V.refresh(eig_steps=200)
    W = mf.VCycle(levels, F64, N, keep=keep)
    bh = np.random.default_rng(N).standard_normal(N)
    bh[od.constrained] = 0.0
    tol = 1e-10 * np.linalg.norm(bh)
    sols, its = [], []
    for P in (V, W):
        cg = mf.CG(op, mf.CG_CALLBACK)
        cg.set_vcycle(P)
        x = mf.DeviceVector(N)
        info = cg.solve(x, dev(bh), tol, 100)
        assert info.status == 1
        its.append(info.iterations)
        sols.append(x.to_host())
    xr = spla.spsolve(A.tocsc(), bh)
    print(f"CG + refreshed V-cycle: {its[0]} iterations, with the fresh object {its[1]}; |x - x*| / |x*| = "
          f"{rel(sols[0], xr):.3e}; refreshed against fresh {rel(sols[0], sols[1]):.3e}")
    assert its[0] == its[1]
    assert np.linalg.norm(sols[0] - xr) <= 1e-8 * np.linalg.norm(xr)


# ---- 6. graph


def test_update_refresh_apply_in_one_graph():
    if torch is None:
        pytest.skip("torch is not installed")
    assert torch.cuda.is_available()
    nt = F64
    levels, keep, meshes, active = make_levels("adaptive_3d_p2_r4", nt)
    N = active.n_dofs
    d = torch.device("cuda", 0)
    qp = [M.arrays()["quadrature_points"].astype(np.float64) for M in meshes]
    coef = [torch.from_numpy(field(1)(x).reshape(-1)).to(d) for x in qp]  # the fixed device arrays of the graph
    R = defects(active, 6)
    r, z = torch.from_numpy(R[:, 0].copy()).to(d), torch.zeros(N, device=d, dtype=torch.float64)
    V = mf.VCycle(levels, F64, N, keep=keep)

    def run(stream):
        for lev, c in zip(levels, coef):
            lev["op"].update_coefficients(c, None, stream)
        V.refresh(200, stream)
        V.apply(z, r, stream)

    run(None)  # the plain refresh, which allocates; code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(torch.cuda.current_stream().cuda_stream)
    for k in (2, 3):  # overwrite the coefficient arrays in place and replay
        for c, x in zip(coef, qp):
            c.copy_(torch.from_numpy(field(k)(x).reshape(-1)))
        z.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        got = z.cpu().numpy()
        assert V.refresh_status().eig_status_max == 1
        W = mf.VCycle(levels, F64, N, keep=keep)  # fresh, on the levels the replay has updated
        want = apply_all(W, R[:, :1])[:, 0]
        print(f"graph replay on field {k}: refreshed against fresh {rel(got, want):.3e}")
        assert rel(got, want) <= REFRESH_TOL[nt]
        del W
    del g


# ---- 7. memory


def round16(b):
    return (b + 15) // 16 * 16


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float"])
@pytest.mark.parametrize("mode", ["estimated-dense", "given-dense", "estimated-cg"])
def test_refresh_memory(mode, nt):
    mesh = mf.Mesh.adaptive_mg(2, 2, 3, number_type=nt)
    levels, keep = mf.VCycle.hierarchy_levels(mesh, flags=UPD)
    es = np.dtype(mf.np_dtype(nt)).itemsize
    n0, nl, degree = levels[0]["n_dofs"], len(levels), 5
    dense = mode.endswith("dense")
    created = 2 * n0 * es + sum((6 + lev["has_edges"]) * lev["n_dofs"] * es for lev in levels[1:])  # today's value
    created += n0 * (n0 + n0 % 2) * 8 if dense else 3 * n0 * es + mf.CG_PARTIAL_BYTES + mf.CG_STATE_BYTES
    grown = 16 + (nl - 1) * (mf.EIG_STATE_BYTES + round16(8 * (2 * degree - 1)))
    grown += mf.EIG_PARTIAL_BYTES if mode.startswith("estimated") else 0
    grown += 2 * round16(n0 * n0 * es) + round16(8 * n0 * n0) + round16(16 * n0 * n0) if dense else 0
    given = None if mode.startswith("estimated") else [2.0] * nl
    r, z = dev(np.ones(mesh.n_dofs)), mf.DeviceVector(mesh.n_dofs)
    inside = []

    def cycle():
        V = mf.VCycle(levels, F64, mesh.n_dofs, lambda_max=given, coarse=COARSE[mode.split("-")[1]])
        assert V.memory_consumption() == created
        V.apply(z, r)
        V.refresh()
        mf.synchronize()
        assert V.memory_consumption() == created + grown
        inside.append(mf.device_memory_info()[0])
        for _ in range(2):  # further refreshes allocate nothing
            V.refresh()
            V.apply(z, r)
            mf.synchronize()
            assert V.memory_consumption() == created + grown
            assert mf.device_memory_info()[0] == inside[-1]
        V.destroy()
        mf.synchronize()

    cycle()  # (code objects, the first inverse diagonal's tables)
    free0, _ = mf.device_memory_info()
    cycle()
    free1, _ = mf.device_memory_info()
    assert free1 == free0, (free0, free1)


# ---- 8. errors and status


def test_refresh_unsupported_above_the_device_cap():
    mesh = mf.Mesh.uniform(3, 4, 2)
    assert mf.SPD_INVERSE_DEVICE_MAX < mesh.n_dofs == 729 <= mf.VCYCLE_DENSE_MAX
    V = mf.VCycle.from_meshes([mesh], coarse=mf.VCYCLE_COARSE_DENSE, flags=UPD)
    r, z = dev(np.random.default_rng(1).standard_normal(729)), mf.DeviceVector(729)
    V.apply(z, r)
    mf.synchronize()
    before, bytes_before = z.to_host(), V.memory_consumption()
    assert V.refresh(check=False) == mf.EUNSUPPORTED
    z.fill(np.nan)
    V.apply(z, r)
    mf.synchronize()
    np.testing.assert_array_equal(z.to_host(), before)
    assert V.memory_consumption() == bytes_before
    assert mf.lib().mfgpu_vcycle_refresh(None, 0, None) == mf.EINVAL
    with pytest.raises(mf.MfgpuError, match="error -1"):
        V.refresh_status()  # no refresh yet


def test_refresh_reports_an_indefinite_coarse_matrix():
    mesh = mf.Mesh.uniform(2, 2, 2)
    mesh.set_mass_coefficient(np.ones((mesh.n_cells, mesh.nd)))
    V = mf.VCycle.from_meshes([mesh], coarse=mf.VCYCLE_COARSE_DENSE, flags=UPD)
    op = V._keep[0][0]["op"]
    n = mesh.n_dofs
    r, z = dev(np.random.default_rng(2).standard_normal(n)), mf.DeviceVector(n)
    V.refresh()
    assert V.refresh_status().coarse_status == 0
    V.apply(z, r)
    mf.synchronize()
    before = z.to_host()
    op.update_coefficients(None, dev(np.full(mesh.n_cells * mesh.nd, -1e6)))
    mf.synchronize()
    V.refresh()
    info = V.refresh_status()
    assert info.coarse_status == 1
    V.apply(z, r)
    mf.synchronize()
    np.testing.assert_array_equal(z.to_host(), before)  # the old inverse stays
