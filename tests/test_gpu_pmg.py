"""The p-multigrid transfer (mfgpu_transfer_create_p, pymfgpu.Transfer.p_from_*) and the V-cycles
built on it, against tests/pmg_reference.py (float64 numpy on the oracle's matrices).

  1. prolongate / prolongate_add / restrict_and_add against the numpy P: all 15 degree pairs on small cubes
  2. the same on the ball (unstructured, mixed cell orientations)
  3. a polynomial of the coarse degree prolongates to itself (a known answer that does not go through the numpy P)
  4. more cells than one pass of the capped grid covers
  5. one V-cycle of VCycle.from_level_meshes over hybrid hierarchies, value for value against the numpy model
  6. CG preconditioned with that V-cycle
  7. float levels under a double CG, refresh after update_coefficients, graph capture of apply
  8. errors
  9. the poisson-pmg drivers

Tolerances: the transfer's are those of test_gpu_transfer.py (relative l2 1e-13 double, 1e-5 float); the V-cycle's those
of test_gpu_vcycle.py for the same comparison on h-levels (VCYCLE_TOL); the refresh's those of test_gpu_refresh.py
(REFRESH_TOL); the graph replay's that of test_gpu_graph.py (1e-13, not bit equality: restriction adds atomically)."""
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

import pmg_reference as pr
import pymfgpu as mf
from test_gpu_refresh import REFRESH_TOL, apply_all, defects, set_coefficient
from test_gpu_vcycle import VCYCLE_TOL, capture_and_replay

pytestmark = pytest.mark.gpu

F64, F32 = mf.F64, mf.F32
TRANSFER_TOL = {F64: 1e-13, F32: 1e-5}
GRAPH_TOL = 1e-13
PAIRS = [(pc, pf) for pf in range(2, 7) for pc in range(1, pf)]
TYPES = pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float"])


def typed(a, nt):
    return np.asarray(a).astype(mf.np_dtype(nt)).astype(np.float64)


def dev(a, nt=F64):
    v = mf.DeviceVector(len(a), nt)
    v.from_host(np.ascontiguousarray(a, dtype=mf.np_dtype(nt)))
    return v


def rel(got, want):
    """relative l2 difference; where want is exactly zero (a coarse level whose dofs are all Dirichlet dofs prolongates to
    zero), the norm of got, which must then be zero too"""
    scale = np.linalg.norm(want)
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / (scale if scale > 0 else 1.0))


# ---- 1. / 2. parity of the three calls


def check_parity(t, P, con, nt, what):
    """t against the sparse P [n_fine, n_coarse] (Dirichlet columns zero, owner rule inside)"""
    tol = TRANSFER_TOL[nt]
    nf, nc = P.shape
    rng = np.random.default_rng(nf * 1000 + nc)
    x, y, z = (typed(rng.standard_normal(n), nt) for n in (nc, nf, nc))
    src, fine = dev(x, nt), mf.DeviceVector(nf, nt)
    fine.fill(3.0)
    t.prolongate(fine, src)  # overwrites
    mf.synchronize()
    got_p = fine.to_host()
    e_p = rel(got_p, P @ x)
    one_call, two_calls = dev(y, nt), dev(y, nt)
    t.prolongate_add(one_call, src)
    two_calls.sadd(1.0, 1.0, fine)
    mf.synchronize()
    e_a = rel(one_call.to_host(), two_calls.to_host().astype(np.float64))
    e_a2 = rel(one_call.to_host(), y + P @ x)
    coarse = dev(z, nt)
    t.restrict_and_add(coarse, dev(y, nt))
    mf.synchronize()
    got_r = coarse.to_host()
    e_r = rel(got_r, z + P.T @ y)
    print(f"{what}: prolongate {e_p:.2e}, prolongate_add against prolongate + sadd {e_a:.2e} (numpy {e_a2:.2e}), "
          f"restrict_and_add {e_r:.2e}")
    assert e_p <= tol and e_a <= tol and e_a2 <= tol and e_r <= tol
    np.testing.assert_array_equal(got_r[con], z[con].astype(got_r.dtype))  # Dirichlet entries: not touched
    np.testing.assert_array_equal(src.to_host(), x.astype(got_p.dtype))    # the source is read only
    assert t.memory_consumption() > 0


def mesh_pair(kind, dim, pc, pf, nt):
    if kind == "cube":
        n = (3, 3) if dim == 2 else (3, 2, 1)  # unequal counts: transposed index orders; odd cell counts: the tail of a
        return mf.Mesh.uniform(dim, pc, n, number_type=nt), mf.Mesh.uniform(dim, pf, n, number_type=nt)  # workgroup
    return mf.Mesh.ball(dim, pc, kind, number_type=nt), mf.Mesh.ball(dim, pf, kind, number_type=nt)


def both_constructions(kind, dim, pc, pf, nt):
    c, f = mesh_pair(kind, dim, pc, pf, nt)
    ca, fa = c.arrays(), f.arrays()
    con = ca["constrained_dofs"].astype(np.int64)
    P = pr.p_transfer_matrix(dim, pc, pf, ca["loc2glob"], fa["loc2glob"], c.n_dofs, f.n_dofs, con)
    name = f"{dim}D {kind} ({pc} -> {pf}) {'double' if nt == F64 else 'float'}"
    check_parity(mf.Transfer.p_from_meshes(c, f), P, con, nt, name + " from_meshes")
    t = mf.Transfer.p_from_arrays(dim, pc, pf, ca["loc2glob"], fa["loc2glob"], c.n_dofs, f.n_dofs, con, nt,
                                  prolongation_1d=pr.P1(pc, pf))
    check_parity(t, P, con, nt, name + " from_arrays with an explicit P1")
    # without Dirichlet dofs (on the 3D cube every dof of degree 1 is one, and P above is zero there)
    none = np.zeros(0, dtype=np.int64)
    P = pr.p_transfer_matrix(dim, pc, pf, ca["loc2glob"], fa["loc2glob"], c.n_dofs, f.n_dofs, none)
    t = mf.Transfer.p_from_arrays(dim, pc, pf, ca["loc2glob"], fa["loc2glob"], c.n_dofs, f.n_dofs, none, nt)
    check_parity(t, P, none, nt, name + " from_arrays without Dirichlet dofs")


@TYPES
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("pc,pf", PAIRS)
def test_parity_on_cubes(pc, pf, dim, nt):
    both_constructions("cube", dim, pc, pf, nt)


@TYPES
@pytest.mark.parametrize("dim,n_ref,pc,pf", [(3, 0, 1, 2), (3, 0, 2, 4), (3, 0, 1, 4), (3, 1, 1, 2), (3, 1, 2, 4),
                                             (3, 1, 1, 4), (2, 1, 2, 4)])
def test_parity_on_the_ball(dim, n_ref, pc, pf, nt):
    both_constructions(n_ref, dim, pc, pf, nt)


# ---- 3. a known answer


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("pc,pf", [(1, 2), (2, 4), (3, 6), (4, 5)])
def test_polynomials_of_the_coarse_degree_are_reproduced(pc, pf, dim):
    c, f = mesh_pair("cube", dim, pc, pf, F64)
    t = mf.Transfer.p_from_arrays(dim, pc, pf, c.arrays()["loc2glob"], f.arrays()["loc2glob"], c.n_dofs, f.n_dofs, [])
    coef = np.random.default_rng(10 * pc + pf).uniform(0.5, 1.5, (dim, pc + 1))

    def poly(X):  # degree pc per direction
        return np.prod([np.polyval(coef[d], X[:, d]) for d in range(dim)], axis=0)

    fine = mf.DeviceVector(f.n_dofs)
    fine.fill(3.0)
    t.prolongate(fine, dev(poly(c.dof_coords())))
    mf.synchronize()
    err = rel(fine.to_host(), poly(f.dof_coords()))
    print(f"{dim}D ({pc} -> {pf}): a polynomial of degree {pc} per direction, rel l2 at the fine dofs {err:.2e}")
    assert err <= 1e-13


# ---- 4. more cells than one pass


@TYPES
def test_more_cells_than_one_pass_of_the_grid(nt):
    c, f = mf.Mesh.uniform(3, 1, 21, number_type=nt), mf.Mesh.uniform(3, 2, 21, number_type=nt)
    assert c.n_cells == 9261 > 4 * 2048 and f.n_dofs == 79507  # 4 cells per workgroup, at most 2048 workgroups
    con = c.arrays()["constrained_dofs"].astype(np.int64)
    P = pr.p_transfer_matrix(3, 1, 2, c.arrays()["loc2glob"], f.arrays()["loc2glob"], c.n_dofs, f.n_dofs, con)
    check_parity(mf.Transfer.p_from_meshes(c, f), P, con, nt, "3D 21^3 cells (1 -> 2)")


# ---- 5. / 6. the V-cycle over hybrid hierarchies

HYBRID = {"3d": (3, [(2, 1), (4, 1), (4, 2), (4, 4)]), "2d": (2, [(2, 1), (4, 1), (8, 1), (8, 2), (8, 4)])}


@functools.lru_cache(maxsize=None)
def model(name):
    """the float64 hierarchy with exact smoother bounds (shared, never modified)"""
    dim, spec = HYBRID[name]
    return pr.level_hierarchy(pr.meshes_of(dim, spec))


def hybrid_meshes(name, nt=F64):
    dim, spec = HYBRID[name]
    return pr.meshes_of(dim, spec, nt)


@functools.lru_cache(maxsize=None)
def hybrid_defects(name):
    return defects(model(name).mesh, 7 + len(name))


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float_levels"])
@pytest.mark.parametrize("name", list(HYBRID))
def test_one_vcycle_value_for_value(name, nt):
    V = mf.VCycle.from_level_meshes(hybrid_meshes(name, nt), F64)  # estimated lambda_max
    ref = pr.with_lambda_max(model(name), V.lambda_max())
    assert V.n_levels == ref.n_levels == len(HYBRID[name][1])
    R = hybrid_defects(name)
    got = apply_all(V, R)
    want = ref.vcycle(R)
    errs = [rel(got[:, k], want[:, k]) for k in range(R.shape[1])]
    print(f"V-cycle hybrid {name} ({R.shape[0]} dofs, {V.n_levels} levels) {'double' if nt == F64 else 'float'} levels: rel l2 "
          f"from the numpy model with the object's lambda_max, largest of {len(errs)}: {max(errs):.3e}")
    assert max(errs) <= VCYCLE_TOL[nt], errs


def solve(name, V):
    """CG to 1e-10 relative on the finest level's operator in double with V as preconditioner: (info, x, b, A)"""
    ref = model(name)
    mesh = hybrid_meshes(name)[-1]
    N = mesh.n_dofs
    b = pr.rhs(ref, seed=N)
    op = mf.Operator(mesh.desc, mesh)
    cg = mf.CG(op, mf.CG_CALLBACK)
    cg.set_vcycle(V)
    x = mf.DeviceVector(N)
    info = cg.solve(x, dev(b), 1e-10 * np.linalg.norm(b), 100)
    return info, x.to_host(), b, ref.A[-1]


@pytest.mark.parametrize("name", list(HYBRID))
def test_cg_with_the_vcycle(name):
    ref = model(name)
    V = mf.VCycle.from_level_meshes(hybrid_meshes(name))
    info, x, b, A = solve(name, V)
    want_it, _ = pr.cg_iterations(ref, b)
    print(f"CG + hybrid V-cycle {name} ({len(b)} dofs): {info.iterations} iterations, numpy model {want_it}")
    assert info.status == 1 and info.iterations <= want_it + 2
    assert info.residual <= 1e-10 * np.linalg.norm(b)
    xr = spla.spsolve(A.tocsc(), b)
    assert np.linalg.norm(x - xr) <= 1e-8 * np.linalg.norm(xr)


# ---- 7. what sits on top: float levels, refresh, graph capture


def test_float_levels_under_a_double_cg():
    """the rule of test_gpu_mixed_mg.py: float levels cost at most two iterations over double levels"""
    name = "3d"
    double, _, _, _ = solve(name, mf.VCycle.from_level_meshes(hybrid_meshes(name)))
    info, x, b, A = solve(name, mf.VCycle.from_level_meshes(hybrid_meshes(name, F32), F64))
    print(f"hybrid {name}: {info.iterations} iterations with float levels, {double.iterations} with double levels")
    assert info.status == 1 and double.status == 1 and info.iterations <= double.iterations + 2
    xr = spla.spsolve(A.tocsc(), b)
    assert np.linalg.norm(x - xr) <= 1e-8 * np.linalg.norm(xr)


def test_refreshed_is_fresh():
    """test_gpu_refresh.py::test_refreshed_is_fresh (estimated lambda_max, dense coarse solve, double) on the hybrid levels"""
    nt = F64
    meshes = hybrid_meshes("3d", nt)
    levels = mf.VCycle.level_mesh_levels(meshes, flags=mf.UPDATABLE_COEFFICIENTS)
    N = meshes[-1].n_dofs
    V = mf.VCycle(levels, F64, N, coarse=mf.VCYCLE_COARSE_DENSE, keep=meshes)
    lam0 = V.lambda_max()
    R = hybrid_defects("3d")
    set_coefficient(levels, meshes, nt, 1)
    stale = apply_all(V, R)
    V.refresh(eig_steps=200)
    assert np.array_equal(V.lambda_max(), lam0)  # until refresh_status: the previous values
    info = V.refresh_status()
    W = mf.VCycle(levels, F64, N, coarse=mf.VCYCLE_COARSE_DENSE, keep=meshes)
    want, got = apply_all(W, R), apply_all(V, R)
    assert info.coarse_status == 0 and info.eig_status_max == 1 and 15 <= info.eig_steps_max <= 200
    np.testing.assert_allclose(V.lambda_max()[1:], W.lambda_max()[1:], rtol=64 * np.finfo(np.float64).eps, atol=0.0)
    err = max(rel(got[:, j], want[:, j]) for j in range(3))
    moved = min(rel(stale[:, j], want[:, j]) for j in range(3))
    print(f"refresh hybrid 3d: refreshed against fresh, largest rel l2 of 3: {err:.3e}; before the refresh {moved:.3e}")
    assert moved > 100 * REFRESH_TOL[nt]
    assert err <= REFRESH_TOL[nt]


def test_apply_is_graph_capturable():
    if torch is None:
        pytest.skip("torch is not installed")
    assert torch.cuda.is_available()
    name = "3d"
    V = mf.VCycle.from_level_meshes(hybrid_meshes(name))
    R = hybrid_defects(name)
    N = R.shape[0]
    d = torch.device("cuda", 0)
    r, z = torch.zeros(N, device=d, dtype=torch.float64), torch.zeros(N, device=d, dtype=torch.float64)
    V.apply(z, r)  # the first use of a kernel loads its code object
    torch.cuda.synchronize()

    def fill(a):
        r.copy_(torch.from_numpy(a))
        z.fill_(float("nan"))

    capture_and_replay(lambda stream: V.apply(z, r, stream), [R[:, 0].copy(), R[:, 1].copy()], fill,
                       lambda: z.cpu().numpy(), GRAPH_TOL)


# ---- 8. errors


def test_errors_are_loud_and_create_nothing():
    c, f = mf.Mesh.uniform(2, 2, 3), mf.Mesh.uniform(2, 4, 3)
    cd, fd, con = c.arrays()["loc2glob"], f.arrays()["loc2glob"], c.arrays()["constrained_dofs"]
    mf.Transfer.p_from_meshes(c, f)  # (code objects, tables: what a first call leaves behind)
    mf.synchronize()
    free0, _ = mf.device_memory_info()

    def raises(code, fn, *args, **kw):
        with pytest.raises(mf.MfgpuError) as e:
            fn(*args, **kw)
        assert e.value.code == code, str(e.value)

    def arrays(pc, pf, cd=cd, fd=fd, nc=c.n_dofs, nf=f.n_dofs, con=con):
        return mf.Transfer.p_from_arrays(2, pc, pf, cd, fd, nc, nf, con)

    raises(mf.EINVAL, arrays, 4, 2, cd=fd, fd=cd)      # pc > pf
    raises(mf.EINVAL, arrays, 2, 2, fd=cd)             # pc == pf
    raises(mf.EINVAL, arrays, 0, 2, cd=cd[:, :1])      # degree 0
    raises(mf.EINVAL, arrays, 2, 7)                    # degree 7
    raises(mf.EINVAL, arrays, 2, 4, nc=c.n_dofs - 1)   # a coarse dof out of range
    raises(mf.EINVAL, arrays, 2, 4, nf=f.n_dofs - 1)   # a fine dof out of range
    raises(mf.EINVAL, arrays, 2, 4, con=np.array([c.n_dofs], dtype=np.uint32))
    raises(mf.EINVAL, arrays, 2, 4, nf=1 << 31)        # dof counts >= 2^31
    h = mf.C.c_void_p()
    assert mf.lib().mfgpu_transfer_create_p(2, 2, 4, F64, c.n_cells, None, fd.ctypes.data, c.n_dofs, f.n_dofs, None, 0, None,
                                            mf.C.byref(h)) == mf.EINVAL and not h.value  # a null array
    assert mf.lib().mfgpu_transfer_create_p_from_meshes(c._h, None, mf.C.byref(h)) == mf.EINVAL and not h.value
    raises(mf.EINVAL, mf.Transfer.p_from_meshes, f, c)                             # the degree falls
    raises(mf.EINVAL, mf.Transfer.p_from_meshes, c, mf.Mesh.uniform(2, 2, 3))      # the degree stays
    raises(mf.EINVAL, mf.Transfer.p_from_meshes, c, mf.Mesh.uniform(2, 4, 4))      # other cell counts
    raises(mf.EINVAL, mf.Transfer.p_from_meshes, c, mf.Mesh.uniform(2, 4, (3, 4)))
    raises(mf.EINVAL, mf.Transfer.p_from_meshes, c, mf.Mesh.uniform(3, 4, 3))      # another dimension
    raises(mf.EINVAL, mf.Transfer.p_from_meshes, mf.Mesh.uniform(2, 2, (5, 1)), mf.Mesh.ball(2, 4, 0))  # cube against ball, 5 cells each
    raises(mf.EINVAL, mf.Transfer.p_from_meshes, mf.Mesh.ball(3, 1, 0), mf.Mesh.ball(3, 2, 1))
    raises(mf.EUNSUPPORTED, mf.Transfer.p_from_meshes, mf.Mesh.adaptive(2, 2, 3), mf.Mesh.adaptive(2, 4, 3))
    raises(mf.EUNSUPPORTED, mf.Transfer.from_meshes, c, f)                         # the h-transfer keeps its answer
    mf.synchronize()
    assert mf.device_memory_info()[0] == free0
    # a renumbered mesh works: the current loc2glob is used as it is
    g = mf.Mesh.uniform(2, 4, 3)
    g.renumber(np.random.default_rng(0).permutation(g.n_dofs).astype(np.uint32))
    P = pr.p_transfer_matrix(2, 2, 4, cd, g.arrays()["loc2glob"], c.n_dofs, g.n_dofs, con)
    check_parity(mf.Transfer.p_from_meshes(c, g), P, con.astype(np.int64), F64, "renumbered fine mesh")
    # a p-transfer that does not fit the two levels it is given with
    m1, m2, m4 = mf.Mesh.uniform(2, 1, 3), c, f
    ops = [mf.Operator(m.desc, m) for m in (m1, m2, m4)]
    t12, t24 = mf.Transfer.p_from_meshes(m1, m2), mf.Transfer.p_from_meshes(m2, m4)
    mf.VCycle([{"op": ops[0]}, {"op": ops[1], "transfer": t12}, {"op": ops[2], "transfer": t24}], F64, m4.n_dofs)
    raises(mf.EINVAL, mf.VCycle, [{"op": ops[0]}, {"op": ops[1], "transfer": t12}, {"op": ops[2], "transfer": t12}], F64,
           m4.n_dofs)
    raises(mf.EINVAL, mf.VCycle, [{"op": ops[0]}, {"op": ops[2], "transfer": t24}], F64, m4.n_dofs)
    with pytest.raises(mf.MfgpuError):
        mf.VCycle.from_level_meshes([m4, m2])                                      # the degree falls
    with pytest.raises(mf.MfgpuError):
        mf.VCycle.from_level_meshes([m2, mf.Mesh.uniform(2, 4, 6)])                # refined AND raised in one step


# ---- 9. drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-cuda_amd", "host", "bin")


def _run(exe, arg):
    out = subprocess.run([os.path.join(BIN, exe), arg], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, exe + " " + arg + ": " + out.stdout + out.stderr
    (f,) = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert len(f) == 7 and float(f[6]) < 1e-8, out.stdout
    return f


@pytest.mark.parametrize("exe,args,h_exe", [("poisson-pmg-3d-p4", ("3", "4"), "poisson-mg-3d-p4-devmg"),
                                            ("poisson-pmg-2d-p4", ("5", "6"), None),
                                            ("poisson-pmg-3d-p4-ball", ("2",), None)])
def test_poisson_pmg_drivers(exe, args, h_exe):
    """dim  degree  n_dofs  levels  cg_iterations  wall_seconds  rel_error"""
    its = []
    for arg in args:
        f = _run(exe, arg)
        its.append(int(f[4]))
        ball = exe.endswith("ball")
        assert int(f[0]) == int(exe[12]) and int(f[1]) == 4 and int(f[3]) == int(arg) + (1 if ball else 0) + 2
        line = f"{exe} {arg}: {f[2]} dofs, {f[3]} levels, {f[4]} iterations, rel_error {f[6]}"
        if h_exe:
            h = _run(h_exe, arg)
            assert h[:3] == f[:3]  # the same problem
            line += f"; {h_exe}: {h[3]} levels, {h[4]} iterations"
            assert int(f[4]) <= int(h[4]) + 2
        print(line)
    if len(its) == 2:
        assert its[1] <= its[0] + 2
