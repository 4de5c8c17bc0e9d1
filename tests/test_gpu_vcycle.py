"""The V-cycle object (mfgpu_vcycle, pymfgpu.VCycle) and the entry points that came with it, against
tests/mg_reference.py (float64 numpy on the oracle's matrices; tests/vcycle_reference.py fills it for globally refined
hierarchies) and against the two-call forms the new launches replace.

  1. Transfer.prolongate_add  == prolongate into a temporary + add, bitwise
  2. vec_residual             == add + sadd, bitwise, aligned and misaligned
  3. the dense coarse solve through a one-level VCycle
  4. one V-cycle value for value against Hierarchy.vcycle, lambda_max handed to both sides
  5. the eigenvalue estimate against the true largest eigenvalue of D^-1 A
  6. CG preconditioned with the V-cycle through mfgpu_cg_set_vcycle, hanging nodes included
  7. CG.begin_relative against the numpy CG
  8. graph capture of apply and of begin + iterate with the V-cycle
  9. memory_consumption and the return of every byte
 10. the MFGPU_EINVAL cases that need real handles
 11. the -devmg drivers against their counterparts

Tolerances that are measurements (MI355X; the largest value over the cases and two runs of the test, each of which applies
the three defects twice; times 10; the restriction's atomics land in another order every run):
  dense coarse solve, float levels against numpy's solve in double:
      cube 2D p=2 1.9e-8, cube 3D p=4 2.4e-8, cube 3D p=6 7.8e-8, ball 3D p=2 1.05e-7       -> 1.1e-6 (cap 1e-4)
  V-cycle, relative l2 difference of z from the numpy reference, double levels / float levels:
      adaptive_mg(2,2,3)  dense 2.2e-15 / 5.4e-7   CG 1.9e-15 / 6.3e-7
      adaptive_mg(3,2,4)  dense 9.5e-16 / 2.5e-7   CG 6.4e-16 / 1.9e-7
      cube 3D p=4 1-2-4   dense 2.1e-15 / 1.7e-7
      ball 3D p=2 0-1-2   dense 7.5e-16 / 1.4e-7                                             -> 2.3e-14 / 6.3e-6 (caps 1e-9 / 1e-4)
  (the coarse CG on 9 or 27 dofs ends at rounding level, so it needs no tolerance of its own)
Tolerances that are conditions: the dense coarse solve in double leaves |b - A0 x| <= 1e-10 |b|, the accuracy of the
coarse CG it replaces; the eigenvalue estimate lies in [lambda, 1.2 lambda (1 + 1e-10)] (float: 1e-5)."""
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse.linalg as spla

try:
    import torch  # before the library is loaded: libmfgpu.so binds to the HIP runtime torch brings (as in bench.py)
except ImportError:
    torch = None

import cg_reference as cgref
import mg_reference as mg
import pymfgpu as mf
import vcycle_reference as vr
from oracle import mf_oracle as o
from util import oracle_desc_from_mesh

pytestmark = pytest.mark.gpu

F64, F32 = mf.F64, mf.F32
NTNAME = {F64: "double", F32: "float"}
DENSE_FLOAT_TOL = 1.1e-6
VCYCLE_TOL = {F64: 2.3e-14, F32: 6.3e-6}  # 10 x the largest measured value (docstring); the caps are 1e-9 / 1e-4
COARSE = {"dense": mf.VCYCLE_COARSE_DENSE, "cg": mf.VCYCLE_COARSE_CG}
assert VCYCLE_TOL[F64] <= 1e-9 and VCYCLE_TOL[F32] <= 1e-4 and DENSE_FLOAT_TOL <= 1e-4


def typed(a, nt):
    """the values a vector of the number type holds, as doubles"""
    return np.asarray(a).astype(mf.np_dtype(nt)).astype(np.float64)


def dev(a, nt=F64):
    v = mf.DeviceVector(len(a), nt)
    v.from_host(np.ascontiguousarray(a, dtype=mf.np_dtype(nt)))
    return v


def rel(got, want):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / np.linalg.norm(want))


# ---- the hierarchies and their float64 references (host only, shared, never modified)

HIERARCHIES = ["adaptive_2d_p2_r3", "adaptive_3d_p2_r4", "cube_3d_p4", "ball_3d_p2"]


def level_meshes(name, nt):
    if name == "cube_3d_p4":
        return vr.cube_meshes(3, 4, (1, 2, 4), nt)
    if name == "ball_3d_p2":
        return vr.ball_meshes(3, 2, (0, 1, 2), nt)
    raise KeyError(name)


def adaptive_args(name):
    return {"adaptive_2d_p2_r3": (2, 2, 3), "adaptive_2d_p4_r3": (2, 4, 3), "adaptive_3d_p2_r4": (3, 2, 4)}[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 hierarchy with its matrices"""
    if name.startswith("adaptive"):
        return mg.Hierarchy(*adaptive_args(name))
    return vr.global_hierarchy(level_meshes(name, F64))


@functools.lru_cache(maxsize=None)
def vcycle_reference(name):
    """three seeded defects that a float holds, zero on the constrained dofs, and the reference's z for each"""
    ref = reference(name)
    N = ref.mesh.n_dofs
    con = ref.mesh.arrays()["constrained_dofs"]
    R = typed(np.random.default_rng(len(name) * 10 + ref.p).standard_normal((N, 3)), F32)
    R[con] = 0.0
    return ref, R, ref.vcycle(R)


def make_vcycle(name, nt, active_type=F64, **options):
    if name.startswith("adaptive"):
        mesh = mf.Mesh.adaptive_mg(*adaptive_args(name), number_type=nt)
        return mf.VCycle.from_hierarchy(mesh, nt, active_type, **options)
    return mf.VCycle.from_meshes(level_meshes(name, nt), active_type, **options)


# ---- 1. prolongate_add


def transfer_case(what, nt):
    if what == "covers_2d_p3":
        c, f = mf.Mesh.uniform(2, 3, 4, number_type=nt), mf.Mesh.uniform(2, 3, 8, number_type=nt)
        return mf.Transfer.from_meshes(c, f), c.n_dofs, f.n_dofs, True
    if what == "grid_stride_3d_p1":
        c, f = mf.Mesh.uniform(3, 1, 21, number_type=nt), mf.Mesh.uniform(3, 1, 42, number_type=nt)
        assert c.n_cells == 9261 > 8192  # more coarse cells than workgroups
        return mf.Transfer.from_meshes(c, f), c.n_dofs, f.n_dofs, True
    # level 3 of adaptive_mg(3, 2, 4): 36 of the 64 cells of level 2 are parents.  Their children are the whole level 3, so
    # the fine level is still covered; without the last parent it is not (the prolongation's zero pass, which
    # prolongate_add must not need)
    h = mg.Hierarchy(3, 2, 4, matrices=False)
    cd, fd = h.patches[3]
    assert len(cd) == 36 < h.od[2].n_cells
    if what == "uncovered_3d_p2":
        cd, fd = cd[:-1], fd[:-1]
    nc, nf = h.od[2].n_dofs, h.od[3].n_dofs
    return mf.Transfer.from_arrays(3, 2, cd, fd, nc, nf, h.od[2].constrained, nt), nc, nf, len(np.unique(fd)) == nf


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float"])
@pytest.mark.parametrize("what,covers", [("covers_2d_p3", True), ("partial_3d_p2", True), ("uncovered_3d_p2", False),
                                         ("grid_stride_3d_p1", True)])
def test_prolongate_add_equals_prolongate_plus_add(what, covers, nt):
    t, nc, nf, covers_all = transfer_case(what, nt)
    assert covers_all == covers
    rng = np.random.default_rng(nc)
    x, y = rng.standard_normal(nc), rng.standard_normal(nf)
    src, tmp, two_calls, one_call = dev(x, nt), mf.DeviceVector(nf, nt), dev(y, nt), dev(y, nt)
    t.prolongate(tmp, src)
    two_calls.add(1.0, tmp)
    t.prolongate_add(one_call, src)
    mf.synchronize()
    got, want = one_call.to_host(), two_calls.to_host()
    assert np.abs(want - y.astype(want.dtype)).max() > 0  # something was added
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(src.to_host(), x.astype(want.dtype))  # src unchanged


# ---- 2. vec_residual


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float"])
@pytest.mark.parametrize("with_e", [False, True], ids=["b-t", "b-(t+e)"])
@pytest.mark.parametrize("n,offset", [(1, 0), (7, 0), (4097, 0), (4097, 1)], ids=["1", "7", "4097", "4097_misaligned"])
def test_vec_residual_equals_add_plus_sadd(n, offset, with_e, nt):
    dt = mf.np_dtype(nt)
    es = np.dtype(dt).itemsize
    rng = np.random.default_rng(n + offset)
    t, b, e = (rng.standard_normal(n + offset).astype(dt) for _ in range(3))
    store = [dev(t, nt), dev(t, nt), dev(b, nt), dev(e, nt)]  # a view one element into its allocation: not 16-byte aligned
    t1, t2, bv, ev = (mf.DeviceVector.view(v.ptr + offset * es, n, nt) for v in store)
    if with_e:
        t1.add(1.0, ev)
    t1.sadd(-1.0, 1.0, bv)
    mf.vec_residual(t2, bv, ev if with_e else None, n, nt)
    mf.synchronize()
    want = store[0].to_host()
    np.testing.assert_array_equal(store[1].to_host(), want)
    host = b[offset:] - (t[offset:] + e[offset:]) if with_e else b[offset:] - t[offset:]
    np.testing.assert_array_equal(want[offset:], host)  # (both are what the formula says)
    np.testing.assert_array_equal(want[:offset], t[:offset])  # nothing written in front of the view
    assert mf.vec_residual(t2, t2, None, n, nt, check=False) == mf.EINVAL
    assert mf.vec_residual(t2, bv, t2, n, nt, check=False) == mf.EINVAL
    if n > 1:  # one element of overlap is enough
        inside = mf.DeviceVector.view(store[2].ptr + (offset + n - 1) * es, n, nt)  # (never touched: the call is refused)
        assert mf.vec_residual(inside, bv, None, n, nt, check=False) == mf.EINVAL
        assert mf.vec_residual(t2, bv, mf.DeviceVector.view(t2.ptr + es, n - 1, nt), n, nt, check=False) == mf.EINVAL


# ---- 3. the dense coarse solve through a one-level VCycle

COARSE_MESHES = {"cube_2d_p2": lambda nt: mf.Mesh.uniform(2, 2, 1, number_type=nt),
                 "cube_3d_p4": lambda nt: mf.Mesh.uniform(3, 4, 1, number_type=nt),
                 "cube_3d_p6": lambda nt: mf.Mesh.uniform(3, 6, 1, number_type=nt),  # 343 rows: more than one workgroup
                 "ball_3d_p2": lambda nt: mf.Mesh.ball(3, 2, 0, number_type=nt)}


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float"])
@pytest.mark.parametrize("name", list(COARSE_MESHES))
def test_dense_coarse_solve(name, nt):
    mesh = COARSE_MESHES[name](nt)
    mesh64 = COARSE_MESHES[name](F64)  # (the oracle description views the mesh's arrays)
    A0 = o.assemble(oracle_desc_from_mesh(mesh64)).toarray()
    n = mesh.n_dofs
    assert A0.shape == (n, n)
    V = mf.VCycle.from_meshes([mesh], coarse=mf.VCYCLE_COARSE_DENSE)
    assert V.n_levels == 1
    b = typed(np.random.default_rng(n).standard_normal(n), nt)
    r, z = dev(b, nt), mf.DeviceVector(n, nt)
    V.apply(z, r)
    mf.synchronize()
    x = z.to_host()
    V.apply(z, r)
    mf.synchronize()
    np.testing.assert_array_equal(z.to_host(), x)  # no atomics: equal bits
    if nt == F64:
        res = np.linalg.norm(b - A0 @ x) / np.linalg.norm(b)
        print(f"dense coarse solve {name} ({n} dofs) double: |b - A0 x| / |b| = {res:.3e}")
        assert res <= 1e-10
    else:
        err = rel(x, np.linalg.solve(A0, b))
        print(f"dense coarse solve {name} ({n} dofs) float: relative l2 difference from numpy's solve = {err:.3e}")
        assert err <= DENSE_FLOAT_TOL


# ---- 4. one V-cycle, value for value


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float_levels"])
@pytest.mark.parametrize("name,coarse", [(h, "dense") for h in HIERARCHIES] + [(h, "cg") for h in HIERARCHIES[:2]])
def test_one_vcycle_value_for_value(name, coarse, nt):
    ref, R, Z = vcycle_reference(name)
    V = make_vcycle(name, nt, F64, lambda_max=ref.lmax, coarse=COARSE[coarse])
    assert V.n_levels == ref.n_levels
    assert name.startswith("adaptive") == any(len(E) for E in ref.edge)
    np.testing.assert_array_equal(V.lambda_max(), ref.lmax)
    N = R.shape[0]
    z = mf.DeviceVector(N, F64)
    errs = []
    for run in range(2):
        for k in range(R.shape[1]):
            z.fill(np.nan)
            V.apply(z, dev(R[:, k]))
            mf.synchronize()
            got = z.to_host()
            assert np.isfinite(got).all()
            errs.append(rel(got, Z[:, k]))
    print(f"V-cycle {name} ({N} dofs, {V.n_levels} levels) {NTNAME[nt]} levels, {coarse} coarse solve: rel l2 from the "
          f"numpy reference, largest of {len(errs)}: {max(errs):.3e}")
    assert max(errs) <= VCYCLE_TOL[nt], errs


# ---- 5. the eigenvalue estimate


@pytest.mark.parametrize("nt,slack", [(F64, 1e-10), (F32, 1e-5)], ids=["double", "float"])
@pytest.mark.parametrize("name", ["adaptive_2d_p2_r3", "adaptive_2d_p4_r3", "adaptive_3d_p2_r4"])
def test_eigenvalue_estimate(name, nt, slack):
    ref = reference(name)
    mesh = mf.Mesh.adaptive_mg(*adaptive_args(name), number_type=nt)
    levels, keep = mf.VCycle.hierarchy_levels(mesh)
    est = []
    for l, lev in enumerate(levels):
        dinv = mf.DeviceVector(lev["n_dofs"], nt)
        lev["op"].compute_inverse_diagonal(dinv)
        est.append(mf.estimate_lambda_max(lev["op"], dinv, 15))
        lam = ref.lmax[l] / 1.2  # the true largest eigenvalue of D^-1 A
        print(f"{name} level {l} {NTNAME[nt]}: estimate / (1.2 lambda) = {est[-1] / (1.2 * lam):.4f}")
        assert lam <= est[-1] <= 1.2 * lam * (1.0 + slack), (l, lam, est[-1])
    V = mf.VCycle(levels, nt, mesh.n_dofs, keep=keep)  # lambda_max = NULL: the same estimate inside
    # The same iteration on the same operator, but not bit for bit: the level operator's apply sums a dof's cell
    # contributions in an order that can differ between two launches, and one of six double estimates came out 1.3e-16
    # (0.6 eps) apart on the MI355X.  The iteration contracts towards the dominant eigenvector, so such roundings do not
    # accumulate over its steps; 64 eps of the level type is the bound (1.4e-14 / 7.6e-6).  Another start vector or
    # another number of steps moves an estimate that stops at 1 % per step by 1e-4 or more.
    np.testing.assert_allclose(V.lambda_max(), est, rtol=64 * np.finfo(mf.np_dtype(nt)).eps, atol=0.0)


# ---- 6. CG with the V-cycle


@pytest.mark.parametrize("name", ["adaptive_2d_p2_r3", "adaptive_3d_p2_r4"])
def test_cg_with_the_vcycle(name):
    ref = reference(name)
    mesh = mf.Mesh.adaptive_mg(*adaptive_args(name))
    od = oracle_desc_from_mesh(mesh)
    assert od.constraint_mask is not None and od.constraint_mask.any()  # hanging nodes
    A = o.assemble(od).tocsr()
    N = mesh.n_dofs
    bh = np.random.default_rng(N).standard_normal(N)
    bh[od.constrained] = 0.0
    tol = 1e-10 * np.linalg.norm(bh)
    want_it = [it for it, status, _, _ in cgref.cg(lambda v: A @ v, bh, ref.vcycle, np.float64, tol, 100) if status == 1][0]
    op = mf.Operator(mesh.desc, mesh)
    V = mf.VCycle.from_hierarchy(mesh)  # estimated lambda_max
    cg = mf.CG(op, mf.CG_CALLBACK)
    cg.set_vcycle(V)
    x = mf.DeviceVector(N)
    info = cg.solve(x, dev(bh), tol, 100)
    print(f"CG + V-cycle {name} ({N} dofs): {info.iterations} iterations, numpy CG with Hierarchy.vcycle {want_it}")
    assert info.status == 1 and info.iterations <= want_it + 1
    xr = spla.spsolve(A.tocsc(), bh)
    assert np.linalg.norm(x.to_host() - xr) <= 1e-8 * np.linalg.norm(xr)


# ---- 7. begin_relative


@pytest.mark.parametrize("relative", [1e-8, 1e-3])
def test_begin_relative(relative):
    mesh = mf.Mesh.uniform(3, 4, 3)
    od = oracle_desc_from_mesh(mesh)
    A = o.assemble(od).toarray()
    N = mesh.n_dofs
    dinv_h = 1.0 / np.diag(A)
    bh = np.random.default_rng(7).standard_normal(N)
    bh[od.constrained] = 0.0
    steps = list(cgref.cg(lambda v: A @ v, bh, lambda r: dinv_h * r, np.float64, relative * np.linalg.norm(bh), 1000))
    want_it, want_status = steps[-1][0], steps[-1][1]
    assert want_status == 1 and want_it > 3
    op = mf.Operator(mesh.desc, mesh)
    dinv, x, b = dev(dinv_h), mf.DeviceVector(N), dev(bh)
    cg = mf.CG(op, mf.CG_JACOBI, dinv)
    cg.begin_relative(x, b, relative, 1000)
    cg.iterate(want_it + 5)
    info = cg.status()
    print(f"begin_relative {relative:g}: {info.iterations} iterations (numpy {want_it}), residual / initial = "
          f"{info.residual / info.initial_residual:.3e}")
    assert (info.iterations, info.status) == (want_it, 1)
    assert info.residual <= relative * info.initial_residual
    assert abs(info.initial_residual - np.linalg.norm(bh)) <= 1e-12 * np.linalg.norm(bh)
    # an absolute solve afterwards on the same object is not relative any more
    cg.begin(x, b, 0.5 * info.initial_residual, 1000)
    cg.iterate(want_it)
    again = cg.status()
    assert again.status == 1 and again.iterations < want_it and again.residual <= 0.5 * info.initial_residual
    # |b| = 0: converged at once
    b.fill(0.0)
    cg.begin_relative(x, b, relative, 1000)
    cg.iterate(2)
    assert cg.status().as_tuple()[:2] == (0, 1)
    assert cg.begin_relative(x, b, -1.0, 10, check=False) == mf.EINVAL
    assert cg.begin_relative(x, b, float("nan"), 10, check=False) == mf.EINVAL
    assert cg.begin_relative(x, x, 1e-3, 10, check=False) == mf.EINVAL


# ---- 8. graph capture


def capture_and_replay(run, inputs, fill, read, tol):
    """run(stream) eagerly on every input, then captured once and replayed on the refilled inputs"""
    s = torch.cuda.Stream()
    want = []
    for a in inputs:
        fill(a)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            run(s.cuda_stream)
        torch.cuda.synchronize()
        want.append(read())
        assert np.isfinite(want[-1]).all() and np.linalg.norm(want[-1]) > 0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(torch.cuda.current_stream().cuda_stream)
    for a, w in zip(inputs, want):
        fill(a)
        g.replay()
        torch.cuda.synchronize()
        assert np.linalg.norm(read() - w) <= tol * np.linalg.norm(w)


@pytest.mark.parametrize("name,nt,coarse", [("adaptive_2d_p2_r3", F64, "dense"), ("adaptive_2d_p2_r3", F32, "cg"),
                                            ("cube_3d_p4", F64, "dense")])
def test_apply_is_graph_capturable(name, nt, coarse):
    if torch is None:
        pytest.skip("torch is not installed")
    assert torch.cuda.is_available()
    ref, R, _ = vcycle_reference(name)
    V = make_vcycle(name, nt, F64, lambda_max=ref.lmax, coarse=COARSE[coarse])
    N = R.shape[0]
    d = torch.device("cuda", 0)
    r, z = torch.zeros(N, device=d, dtype=torch.float64), torch.zeros(N, device=d, dtype=torch.float64)
    V.apply(z, r)  # the first use of a kernel loads its code object
    torch.cuda.synchronize()

    def fill(a):
        r.copy_(torch.from_numpy(a))
        z.fill_(float("nan"))

    capture_and_replay(lambda stream: V.apply(z, r, stream), [R[:, 0].copy(), R[:, 1].copy()], fill,
                       lambda: z.cpu().numpy(), VCYCLE_TOL[nt])


def test_cg_with_the_vcycle_is_graph_capturable():
    if torch is None:
        pytest.skip("torch is not installed")
    name = "adaptive_2d_p2_r3"
    ref, R, _ = vcycle_reference(name)
    mesh = mf.Mesh.adaptive_mg(*adaptive_args(name))
    op = mf.Operator(mesh.desc, mesh)
    V = mf.VCycle.from_hierarchy(mesh, lambda_max=ref.lmax)
    cg = mf.CG(op, mf.CG_CALLBACK)
    cg.set_vcycle(V)
    N = mesh.n_dofs
    d = torch.device("cuda", 0)
    b, x = torch.zeros(N, device=d, dtype=torch.float64), torch.zeros(N, device=d, dtype=torch.float64)

    def run(stream):
        cg.begin(x, b, 0.0, 1000, stream)
        cg.iterate(4, stream)

    def fill(a):
        b.copy_(torch.from_numpy(a))
        x.fill_(float("nan"))

    fill(R[:, 2].copy())
    run(None)  # code objects
    torch.cuda.synchronize()
    capture_and_replay(run, [R[:, 0].copy(), R[:, 1].copy()], fill, lambda: x.cpu().numpy(), VCYCLE_TOL[F64])
    assert cg.status().as_tuple()[:2] == (4, 0)


# ---- 9. memory


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float"])
@pytest.mark.parametrize("coarse", ["dense", "cg"])
def test_memory_consumption(coarse, nt):
    """levels above 0: defect, solution, t, r, upd, the inverse diagonal (+ edge where the level has edges); level 0:
    defect, solution, and the inverse in double with rows of an even length or the internal CG"""
    mesh = mf.Mesh.adaptive_mg(2, 2, 3, number_type=nt)
    levels, keep = mf.VCycle.hierarchy_levels(mesh)
    es = np.dtype(mf.np_dtype(nt)).itemsize
    n0 = levels[0]["n_dofs"]
    want = 2 * n0 * es + sum((6 + lev["has_edges"]) * lev["n_dofs"] * es for lev in levels[1:])
    assert any(lev["has_edges"] for lev in levels) and not all(lev["has_edges"] for lev in levels[1:])
    want += n0 * (n0 + n0 % 2) * 8 if coarse == "dense" else 3 * n0 * es + mf.CG_PARTIAL_BYTES + mf.CG_STATE_BYTES
    r, z = dev(np.ones(mesh.n_dofs)), mf.DeviceVector(mesh.n_dofs)

    def cycle():
        V = mf.VCycle(levels, F64, mesh.n_dofs, coarse=COARSE[coarse])
        assert V.memory_consumption() == want
        V.apply(z, r)
        mf.synchronize()
        V.destroy()
        mf.synchronize()

    cycle()  # (the first use of a kernel loads its code object, the first inverse diagonal of a handle its tables)
    free0, _ = mf.device_memory_info()
    cycle()
    free1, _ = mf.device_memory_info()
    assert free1 == free0, (free0, free1)


# ---- 10. errors that need real handles


def test_argument_checks():
    m1, m2, m4 = vr.cube_meshes(2, 2, (1, 2, 4))
    ops = [mf.Operator(m.desc, m) for m in (m1, m2, m4)]
    t12, t24 = mf.Transfer.from_meshes(m1, m2), mf.Transfer.from_meshes(m2, m4)
    good = [{"op": ops[0]}, {"op": ops[1], "transfer": t12}, {"op": ops[2], "transfer": t24}]
    N = m4.n_dofs
    V = mf.VCycle(good, F64, N)
    ident = mf.IndexPairs(np.arange(N), np.arange(N))
    m2f = mf.Mesh.uniform(2, 2, 2, number_type=F32)
    lev = mf.Level(m4.desc, np.array([5, 6], dtype=np.uint32), m4)

    def bad(levels, n_active=N, **kw):
        with pytest.raises(mf.MfgpuError, match="error -1"):
            mf.VCycle(levels, kw.pop("active_type", F64), n_active, **kw)

    bad([good[0], {"op": ops[1]}, good[2]])                                     # a missing transfer above level 0
    bad([good[0], good[1], {"op": ops[2], "transfer": t12}])                    # a transfer of two other levels
    bad([good[0], good[1], {"op": ops[2], "edges": lev, "transfer": t24}])      # op is not the operator of the edges
    bad([good[0], good[1], dict(good[2], to_mg=ident, from_mg=ident)])          # pairs on one level only
    bad([dict(g, to_mg=ident) for g in good])                                   # to_mg without from_mg
    bad(good, n_active=N - 1)                                                   # no pairs: the active vector is the finest level's
    bad([good[0], {"op": mf.Operator(m2f.desc, m2f), "transfer": t12}, good[2]])  # levels of two number types
    bad(good, coarse=3)
    bad(good, active_type=2)
    bad(good, lambda_max=[1.0, 2.0, 0.0])
    bad(good, smoothing_range=1.0)
    bad(good[::-1][:1] + good[1:])                                              # (level 0 is not t12's coarse level)
    big = mf.Mesh.uniform(3, 4, 4)                                              # 4913 dofs
    assert big.n_dofs > mf.VCYCLE_DENSE_MAX
    op_big = mf.Operator(big.desc, big)
    bad([{"op": op_big}], n_active=big.n_dofs, coarse=mf.VCYCLE_COARSE_DENSE)   # DENSE above the cap
    auto = mf.VCycle([{"op": op_big}], F64, big.n_dofs)                         # AUTO takes the CG there
    assert auto.memory_consumption() == 5 * big.n_dofs * 8 + mf.CG_PARTIAL_BYTES + mf.CG_STATE_BYTES
    neg = mf.Mesh.uniform(2, 2, 2)
    neg.set_mass_coefficient(np.full((neg.n_cells, neg.nd), -1e3))              # K - 1000 M is indefinite
    with pytest.raises(mf.MfgpuError, match="error -1.*positive definite"):
        mf.VCycle([{"op": mf.Operator(neg.desc, neg)}], F64, neg.n_dofs)
    # apply
    r, z = dev(np.ones(N)), mf.DeviceVector(N)
    assert V.apply(None, r, check=False) == mf.EINVAL and V.apply(z, None, check=False) == mf.EINVAL
    assert V.apply(z, z, check=False) == mf.EINVAL
    # set_vcycle
    jac = mf.CG(ops[2], mf.CG_NONE)
    assert jac.set_vcycle(V, check=False) == mf.EINVAL                          # not a CALLBACK solver
    assert mf.CG(ops[1], mf.CG_CALLBACK).set_vcycle(V, check=False) == mf.EINVAL  # another length
    m4f = mf.Mesh.uniform(2, 2, 4, number_type=F32)
    assert mf.CG(mf.Operator(m4f.desc, m4f), mf.CG_CALLBACK).set_vcycle(V, check=False) == mf.EINVAL  # another type
    cb = mf.CG(ops[2], mf.CG_CALLBACK)
    assert cb.set_vcycle(V, check=False) == mf.OK
    assert cb.solve(z, r, 1e-8 * np.sqrt(N), 50).status == 1


# ---- 11. drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-cuda_amd", "host", "bin")


def _run(exe, args):
    out = subprocess.run([os.path.join(BIN, exe)] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return [ln.split() for ln in out.stdout.strip().splitlines()]


@pytest.mark.parametrize("exe", ["poisson-mg-2d-p2", "poisson-mg-3d-p4", "poisson-mg-3d-p4-adaptive", "poisson-mg-3d-p2-ball",
                                 "poisson-mg-3d-p4-mixed"])
def test_poisson_mg_devmg_drivers(exe):
    """dim  degree  n_dofs  levels  cg_iterations  wall_seconds  rel_error [...]: the same first four columns, iteration
    counts within one, rel_error (|x - x*| / |x*| of a solve to 1e-12 |b|) within 1e-8, the rule of
    test_gpu_cg.py::test_poisson_mg_devcg_driver"""
    for arg in ("2", "3"):
        (h,), (d,) = _run(exe, [arg]), _run(exe + "-devmg", [arg])
        assert len(h) == len(d) >= 7 and h[:4] == d[:4]
        print(f"{exe} {arg}: iterations {h[4]} shim V-cycle, {d[4]} mfgpu_vcycle; rel_error {h[6]} / {d[6]}")
        assert abs(int(h[4]) - int(d[4])) <= 1
        assert abs(float(h[6]) - float(d[6])) <= 1e-8
