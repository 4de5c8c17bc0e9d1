"""The p-multigrid transfer on meshes with hanging nodes (mfgpu_transfer_create_p_hn, pymfgpu.Transfer.p_hn_from_*;
DESIGN.md section 19) and the V-cycles built on it, against tests/pmg_hn_reference.py (float64 numpy on the oracle's
hn_resolve and matrices).

   1. prolongate / prolongate_add / restrict_and_add against the numpy P on small meshes with face, edge and corner masks
   2. <P x, y> = <x, P^T y> without the reference
   3. a polynomial of the coarse degree prolongates to itself at every fine dof some cell lists
   4. conforming meshes through the new entry: bit for bit what the conforming transfer computes
   5. more cells than one pass of the capped grid covers
   6. one V-cycle of VCycle.from_level_meshes over ONE adaptive mesh at degrees 1, 2, 4, value for value against the model
   7. CG preconditioned with that V-cycle, double and float levels
   8. refresh after update_coefficients, graph capture of apply
   9. errors
  10. the poisson-pmg-*-adaptive drivers

Tolerances are those of test_gpu_pmg.py for the same comparisons (TRANSFER_TOL, VCYCLE_TOL, REFRESH_TOL, GRAPH_TOL,
iterations <= the numpy model's + 2).  The adjointness test compares two dot products over N = 6902 fine dofs, each a
sum with a rounding error of about sqrt(N) eps |P x| |y| = 2e-14 |P x| |y|; its bound is 1e-13 |P x| |y|."""
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

import pmg_hn_reference as hr
import pmg_reference as pr
import pymfgpu as mf
from oracle import mf_oracle as o
from test_gpu_pmg import GRAPH_TOL, TRANSFER_TOL, check_parity, dev, rel, typed
from test_gpu_refresh import REFRESH_TOL, apply_all, defects
from test_gpu_vcycle import VCYCLE_TOL, capture_and_replay
from test_hanging_host import CASES, leaves_refine

pytestmark = pytest.mark.gpu

F64, F32 = mf.F64, mf.F32
TYPES = pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float"])
NTNAME = {F64: "double", F32: "float"}


def leaf_meshes(name, pc, pf, nt=F64):
    dim, leaves = CASES[name]
    return dim, mf.Mesh.from_leaves(dim, pc, leaves, number_type=nt), mf.Mesh.from_leaves(dim, pf, leaves, number_type=nt)


def unlisted(mesh):
    """the dofs no cell lists: the hanging ones"""
    seen = np.zeros(mesh.n_dofs, dtype=bool)
    seen[mesh.arrays()["loc2glob"].reshape(-1)] = True
    return ~seen


def check_parity_hn(t, P, con, nt, what, hanging):
    """check_parity of test_gpu_pmg.py, and on the fine dofs no cell lists: prolongate stores exact zeros,
    prolongate_add leaves them as they were"""
    check_parity(t, P, con, nt, what)
    nf, nc = P.shape
    rng = np.random.default_rng(nf + nc)
    x, y = typed(rng.standard_normal(nc), nt), typed(rng.standard_normal(nf), nt)
    fine, acc = mf.DeviceVector(nf, nt), dev(y, nt)
    fine.fill(3.0)
    t.prolongate(fine, dev(x, nt))
    t.prolongate_add(acc, dev(x, nt))
    mf.synchronize()
    assert hanging.any() and not fine.to_host()[hanging].any()
    np.testing.assert_array_equal(acc.to_host()[hanging], y[hanging].astype(mf.np_dtype(nt)))


# ---- 1. parity of the three calls


@TYPES
@pytest.mark.parametrize("pc,pf", [(1, 2), (2, 4), (1, 4), (3, 6), (4, 5)])
@pytest.mark.parametrize("name", ["2d_corner", "2d_L", "3d_corner", "3d_edge", "3d_slab"])
def test_parity_on_meshes_with_hanging_nodes(name, pc, pf, nt):
    dim, c, f = leaf_meshes(name, pc, pf, nt)
    ca, fa = c.arrays(), f.arrays()
    mask = ca["constraint_mask"]
    assert c.n_cells == {"2d_corner": 7, "3d_corner": 15}.get(name, c.n_cells) and (mask != 0).any()
    if name == "3d_edge":  # cells whose only constraint is an edge
        assert ((mask != 0) & ((mask & (0b111 << 3)) == 0) & ((mask & (0b111 << 6)) != 0)).any()
    np.testing.assert_array_equal(mask, fa["constraint_mask"])
    con = ca["constrained_dofs"].astype(np.int64)
    hanging = unlisted(f)
    what = f"{name} ({pc} -> {pf}) {NTNAME[nt]}"
    P = hr.mesh_pair_matrix_hn(c, f)
    check_parity_hn(mf.Transfer.p_hn_from_meshes(c, f), P, con, nt, what + " from_meshes", hanging)
    args = (dim, pc, pf, ca["loc2glob"], fa["loc2glob"], c.n_dofs, f.n_dofs)
    t = mf.Transfer.p_hn_from_arrays(*args, con, nt, prolongation_1d=pr.P1(pc, pf), constraint_mask=mask,
                                     coarse_constraint_weights=o.constraint_weights(pc))
    check_parity_hn(t, P, con, nt, what + " from_arrays with an explicit P1 and weights", hanging)
    none = np.zeros(0, dtype=np.int64)
    P = hr.mesh_pair_matrix_hn(c, f, dirichlet=none)
    t = mf.Transfer.p_hn_from_arrays(*args, none, nt, constraint_mask=mask)
    check_parity_hn(t, P, none, nt, what + " from_arrays without Dirichlet dofs", hanging)


# ---- 2. adjointness


def test_restriction_is_the_transpose_of_prolongation():
    dim, c, f = leaf_meshes("3d_two", 2, 4)
    t = mf.Transfer.p_hn_from_arrays(dim, 2, 4, c.arrays()["loc2glob"], f.arrays()["loc2glob"], c.n_dofs, f.n_dofs, [],
                                     constraint_mask=c.arrays()["constraint_mask"])
    rng = np.random.default_rng(24)
    x, y = rng.standard_normal(c.n_dofs), rng.standard_normal(f.n_dofs)
    Px, PTy = mf.DeviceVector(f.n_dofs), mf.DeviceVector(c.n_dofs)
    PTy.fill(0.0)
    t.prolongate(Px, dev(x))
    t.restrict_and_add(PTy, dev(y))
    mf.synchronize()
    Px, PTy = Px.to_host(), PTy.to_host()
    lhs, rhs = float(Px @ y), float(x @ PTy)
    scale = np.linalg.norm(Px) * np.linalg.norm(y)
    print(f"3d_two (2 -> 4), {f.n_dofs} fine dofs: <P x, y> = {lhs:.15e}, <x, P^T y> = {rhs:.15e}, difference / (|P x| |y|) "
          f"{abs(lhs - rhs) / scale:.2e}")
    assert scale > 0 and abs(lhs - rhs) <= 1e-13 * scale


# ---- 3. a known answer


@pytest.mark.parametrize("pc,pf", [(1, 2), (2, 4), (3, 6), (4, 5)])
@pytest.mark.parametrize("name", ["3d_edge", "2d_L"])
def test_polynomials_of_the_coarse_degree_are_reproduced(name, pc, pf):
    dim, c, f = leaf_meshes(name, pc, pf)
    t = mf.Transfer.p_hn_from_arrays(dim, pc, pf, c.arrays()["loc2glob"], f.arrays()["loc2glob"], c.n_dofs, f.n_dofs, [],
                                     constraint_mask=c.arrays()["constraint_mask"])
    coef = np.random.default_rng(10 * pc + pf).uniform(0.5, 1.5, (dim, pc + 1))

    def poly(X):  # degree pc per direction
        return np.prod([np.polyval(coef[d], X[:, d]) for d in range(dim)], axis=0)

    fine = mf.DeviceVector(f.n_dofs)
    fine.fill(3.0)
    t.prolongate(fine, dev(poly(c.dof_coords())))
    mf.synchronize()
    sel = ~unlisted(f)
    err = rel(fine.to_host()[sel], poly(f.dof_coords())[sel])
    print(f"{name} ({pc} -> {pf}): a polynomial of degree {pc} per direction, rel l2 at the {sel.sum()} fine dofs that are "
          f"not hanging {err:.2e}")
    assert err <= 1e-13


# ---- 4. conforming meshes through the new entry


@TYPES
@pytest.mark.parametrize("pc,pf", [(1, 2), (2, 4)])
@pytest.mark.parametrize("kind", ["cube", "ball"])
def test_conforming_meshes_compute_what_the_conforming_transfer_computes(kind, pc, pf, nt):
    if kind == "cube":
        c, f = (mf.Mesh.uniform(3, p, (3, 2, 1), number_type=nt) for p in (pc, pf))
    else:
        c, f = (mf.Mesh.ball(3, p, 1, number_type=nt) for p in (pc, pf))
    ca, fa = c.arrays(), f.arrays()
    assert ca["constraint_mask"] is None
    con = ca["constrained_dofs"]
    args = (3, pc, pf, ca["loc2glob"], fa["loc2glob"], c.n_dofs, f.n_dofs, con, nt)
    want_t = mf.Transfer.p_from_meshes(c, f)
    rng = np.random.default_rng(pc + 10 * pf)
    x, y, z = (typed(rng.standard_normal(n), nt) for n in (c.n_dofs, f.n_dofs, c.n_dofs))

    def three(t):
        fine, acc, coarse = mf.DeviceVector(f.n_dofs, nt), dev(y, nt), dev(z, nt)
        fine.fill(3.0)
        t.prolongate(fine, dev(x, nt))
        t.prolongate_add(acc, dev(x, nt))
        t.restrict_and_add(coarse, dev(y, nt))
        mf.synchronize()
        return fine.to_host(), acc.to_host(), coarse.to_host()

    want = three(want_t)
    zero = np.zeros(c.n_cells, dtype=np.uint32)
    for what, t, null in (("from_meshes", mf.Transfer.p_hn_from_meshes(c, f), True),
                          ("a NULL mask", mf.Transfer.p_hn_from_arrays(*args), True),
                          ("an all-zero mask", mf.Transfer.p_hn_from_arrays(*args, constraint_mask=zero), False)):
        got = three(t)
        np.testing.assert_array_equal(got[0], want[0])  # prolongate, bit for bit
        np.testing.assert_array_equal(got[1], want[1])  # prolongate_add
        e_r = rel(got[2], want[2].astype(np.float64))   # restrict_and_add adds atomically
        print(f"{kind} ({pc} -> {pf}) {NTNAME[nt]}, {what}: prolongate and prolongate_add bit-equal, restrict_and_add {e_r:.2e}")
        assert e_r <= TRANSFER_TOL[nt]
        if null:
            assert t.memory_consumption() == want_t.memory_consumption()
        else:
            assert t.memory_consumption() > want_t.memory_consumption()


# ---- 5. more cells than one pass


@functools.lru_cache(maxsize=None)
def large_pair_matrix():
    c, f = mf.Mesh.adaptive(3, 1, 5), mf.Mesh.adaptive(3, 2, 5)
    return hr.mesh_pair_matrix_hn(c, f)


@TYPES
def test_more_cells_than_one_pass_of_the_grid(nt):
    c, f = mf.Mesh.adaptive(3, 1, 5, number_type=nt), mf.Mesh.adaptive(3, 2, 5, number_type=nt)
    mask = c.arrays()["constraint_mask"]
    assert c.n_cells == 33797 > 4 * 2048 and int((mask != 0).sum()) == 21301 and f.n_dofs == 328847
    con = c.arrays()["constrained_dofs"].astype(np.int64)
    check_parity_hn(mf.Transfer.p_hn_from_meshes(c, f), large_pair_matrix(), con, nt,
                    f"3D adaptive n_ref 5, 33797 cells (1 -> 2) {NTNAME[nt]}", unlisted(f))


# ---- 6. / 7. the V-cycle over one adaptive mesh at degrees 1, 2, 4

ADAPTIVE = {"2d": (2, 3), "3d": (3, 4)}  # (dim, n_ref); level 0 has 176 / 1210 dofs: the coarse solve is dense
DEGREES = (1, 2, 4)


def level_meshes(name, nt=F64):
    dim, n_ref = ADAPTIVE[name]
    return [mf.Mesh.adaptive(dim, p, n_ref, number_type=nt) for p in DEGREES]


@functools.lru_cache(maxsize=None)
def model(name):
    """the float64 hierarchy with exact smoother bounds (shared, never modified)"""
    return hr.level_hierarchy_hn(level_meshes(name))


@functools.lru_cache(maxsize=None)
def level_defects(name):
    return defects(model(name).mesh, 11 + len(name))


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float_levels"])
@pytest.mark.parametrize("name", list(ADAPTIVE))
def test_one_vcycle_value_for_value(name, nt):
    V = mf.VCycle.from_level_meshes(level_meshes(name, nt), F64)  # estimated lambda_max
    ref = pr.with_lambda_max(model(name), V.lambda_max())
    assert V.n_levels == ref.n_levels == 3
    assert [M.n_dofs for M in ref.meshes] == {"2d": [176, 678, 2498], "3d": [1210, 8302, 57142]}[name]
    R = level_defects(name)
    got = apply_all(V, R)
    want = ref.vcycle(R)
    errs = [rel(got[:, k], want[:, k]) for k in range(R.shape[1])]
    print(f"V-cycle adaptive {name} degrees 1, 2, 4 ({R.shape[0]} dofs) {NTNAME[nt]} levels: rel l2 from the numpy model with "
          f"the object's lambda_max, largest of {len(errs)}: {max(errs):.3e}")
    assert max(errs) <= VCYCLE_TOL[nt], errs


def solve(name, V):
    """CG to 1e-10 relative on the finest level's operator in double with V as preconditioner: (info, x, b, A)"""
    ref = model(name)
    mesh = level_meshes(name)[-1]
    N = mesh.n_dofs
    b = pr.rhs(ref, seed=N)
    op = mf.Operator(mesh.desc, mesh)
    cg = mf.CG(op, mf.CG_CALLBACK)
    cg.set_vcycle(V)
    x = mf.DeviceVector(N)
    info = cg.solve(x, dev(b), 1e-10 * np.linalg.norm(b), 100)
    return info, x.to_host(), b, ref.A[-1]


@functools.lru_cache(maxsize=None)
def direct_solution(name):
    ref = model(name)
    # (the minimum-degree ordering of A^T + A: the matrix is symmetric, and the default ordering takes 20 times as long)
    return spla.spsolve(ref.A[-1].tocsc(), pr.rhs(ref, seed=ref.mesh.n_dofs), permc_spec="MMD_AT_PLUS_A")


@pytest.mark.parametrize("name", list(ADAPTIVE))
def test_cg_with_the_vcycle(name):
    ref = model(name)
    double, x, b, _ = solve(name, mf.VCycle.from_level_meshes(level_meshes(name)))
    want_it, _ = pr.cg_iterations(ref, b)
    single, xs, _, _ = solve(name, mf.VCycle.from_level_meshes(level_meshes(name, F32), F64))
    print(f"CG + p-V-cycle adaptive {name} ({len(b)} dofs): {double.iterations} iterations with double levels, "
          f"{single.iterations} with float levels, numpy model {want_it}")
    assert double.status == 1 and double.iterations <= want_it + 2
    assert double.residual <= 1e-10 * np.linalg.norm(b)
    assert single.status == 1 and single.iterations <= double.iterations + 2
    xr = direct_solution(name)
    assert np.linalg.norm(x - xr) <= 1e-8 * np.linalg.norm(xr)
    assert np.linalg.norm(xs - xr) <= 1e-8 * np.linalg.norm(xr)


# ---- 8. refresh, graph capture


def field2(x):
    """a smooth positive coefficient at quadrature points x [..., 2]"""
    return 1.0 + x[..., 0] ** 2 + 2.0 * x[..., 1] ** 2


def test_refreshed_is_fresh():
    """test_gpu_pmg.py::test_refreshed_is_fresh on the 2D adaptive mesh (176 dofs on level 0: within the device cap of the
    dense refresh)"""
    nt = F64
    meshes = level_meshes("2d", nt)
    levels = mf.VCycle.level_mesh_levels(meshes, flags=mf.UPDATABLE_COEFFICIENTS)
    N = meshes[-1].n_dofs
    V = mf.VCycle(levels, F64, N, coarse=mf.VCYCLE_COARSE_DENSE, keep=meshes)
    lam0 = V.lambda_max()
    R = level_defects("2d")
    for lev, M in zip(levels, meshes):
        c = field2(M.arrays()["quadrature_points"].astype(np.float64))
        lev["op"].update_coefficients(dev(c.reshape(-1), nt), None)
    mf.synchronize()
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
    print(f"refresh adaptive 2d degrees 1, 2, 4: refreshed against fresh, largest rel l2 of 3: {err:.3e}; before the refresh "
          f"{moved:.3e}")
    assert moved > 100 * REFRESH_TOL[nt]
    assert err <= REFRESH_TOL[nt]


def test_apply_is_graph_capturable():
    if torch is None:
        pytest.skip("torch is not installed")
    assert torch.cuda.is_available()
    name = "3d"
    V = mf.VCycle.from_level_meshes(level_meshes(name))
    R = level_defects(name)
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


# ---- 9. errors


def test_errors_are_loud_and_create_nothing():
    dim, c, f = leaf_meshes("2d_corner", 2, 4)
    ca, fa = c.arrays(), f.arrays()
    cd, fd, con, mask = ca["loc2glob"], fa["loc2glob"], ca["constrained_dofs"], ca["constraint_mask"]
    mf.Transfer.p_hn_from_meshes(c, f)  # (code objects, tables: what a first call leaves behind)
    mf.synchronize()
    free0, _ = mf.device_memory_info()

    def raises(code, fn, *args, **kw):
        with pytest.raises(mf.MfgpuError) as e:
            fn(*args, **kw)
        assert e.value.code == code, str(e.value)

    def arrays(pc=2, pf=4, cd=cd, fd=fd, nc=c.n_dofs, nf=f.n_dofs, con=con, mask=mask, dim=2):
        return mf.Transfer.p_hn_from_arrays(dim, pc, pf, cd, fd, nc, nf, con, constraint_mask=mask)

    def with_bit(bit):
        m = mask.copy()
        m[0] |= np.uint32(1 << bit)
        return m

    arrays()
    raises(mf.EINVAL, arrays, mask=with_bit(9))                      # a bit outside the 9 defined ones
    raises(mf.EINVAL, arrays, mask=with_bit(31))
    for bit in (2, 5, 6, 7, 8):                                      # 3D bits in 2D
        raises(mf.EINVAL, arrays, mask=with_bit(bit))
    # two cells that share a face and both flag it: the dofs inside the face are listed, and nobody owns them
    u2, u4 = mf.Mesh.uniform(2, 2, (2, 1)), mf.Mesh.uniform(2, 4, (2, 1))
    pair = dict(cd=u2.arrays()["loc2glob"], fd=u4.arrays()["loc2glob"], nc=u2.n_dofs, nf=u4.n_dofs,
                con=u2.arrays()["constrained_dofs"])
    raises(mf.EINVAL, arrays, mask=np.array([1 << 3, (1 << 3) | 1], dtype=np.uint32), **pair)
    arrays(mask=np.array([1 << 3, 0], dtype=np.uint32), **pair)      # (flagged on one side only: the neighbour owns them)
    # what mfgpu_transfer_create_p refuses
    raises(mf.EINVAL, arrays, 4, 2, cd=fd, fd=cd)                    # the degree falls
    raises(mf.EINVAL, arrays, 2, 2, fd=cd)                           # the degree stays
    raises(mf.EINVAL, arrays, 2, 7)
    raises(mf.EINVAL, arrays, nc=c.n_dofs - 1)                       # a coarse dof out of range
    raises(mf.EINVAL, arrays, nf=f.n_dofs - 1)
    raises(mf.EINVAL, arrays, con=np.array([c.n_dofs], dtype=np.uint32))
    raises(mf.EINVAL, arrays, nf=1 << 31)
    h = mf.C.c_void_p()
    L = mf.lib()
    assert L.mfgpu_transfer_create_p_hn(2, 2, 4, F64, c.n_cells, None, fd.ctypes.data, c.n_dofs, f.n_dofs, None, 0, None,
                                        mask.ctypes.data, None, mf.C.byref(h)) == mf.EINVAL and not h.value  # null arrays
    assert L.mfgpu_transfer_create_p_hn(2, 2, 4, F64, c.n_cells, cd.ctypes.data, None, c.n_dofs, f.n_dofs, None, 0, None,
                                        mask.ctypes.data, None, mf.C.byref(h)) == mf.EINVAL and not h.value
    assert L.mfgpu_transfer_create_p_hn(2, 2, 4, F64, c.n_cells, cd.ctypes.data, fd.ctypes.data, c.n_dofs, f.n_dofs, None, 0,
                                        None, mask.ctypes.data, None, None) == mf.EINVAL
    assert L.mfgpu_transfer_create_p_hn_from_meshes(c._h, None, mf.C.byref(h)) == mf.EINVAL and not h.value
    assert L.mfgpu_transfer_create_p_hn_from_meshes(None, f._h, mf.C.byref(h)) == mf.EINVAL and not h.value
    raises(mf.EINVAL, mf.Transfer.p_hn_from_meshes, f, c)                                          # the degree falls
    raises(mf.EINVAL, mf.Transfer.p_hn_from_meshes, c, mf.Mesh.from_leaves(2, 2, CASES["2d_corner"][1]))  # ... stays
    other = mf.Mesh.from_leaves(2, 4, leaves_refine(2, 1, [(1, 1)]))                               # 7 cells, another corner
    assert other.n_cells == c.n_cells
    raises(mf.EINVAL, mf.Transfer.p_hn_from_meshes, c, other)
    raises(mf.EINVAL, mf.Transfer.p_hn_from_meshes, c, mf.Mesh.adaptive(2, 4, 3))                  # other cell counts
    raises(mf.EINVAL, mf.Transfer.p_hn_from_meshes, mf.Mesh.adaptive(2, 2, 3), mf.Mesh.adaptive(3, 4, 3))
    raises(mf.EINVAL, mf.Transfer.p_hn_from_meshes, mf.Mesh.uniform(2, 2, (7, 1)), f)              # a cube against leaves
    raises(mf.EINVAL, mf.Transfer.p_hn_from_meshes, mf.Mesh.uniform(2, 2, 3), mf.Mesh.uniform(2, 4, 4))
    raises(mf.EUNSUPPORTED, mf.Transfer.p_from_meshes, c, f)                                       # the old entry keeps its answer
    mf.synchronize()
    assert mf.device_memory_info()[0] == free0
    # the accepted pairs: conforming ones, adaptive against from_leaves of the same leaves
    mf.Transfer.p_hn_from_meshes(mf.Mesh.uniform(2, 2, 3), mf.Mesh.uniform(2, 4, 3))
    a2 = mf.Mesh.adaptive(2, 2, 3)
    mf.Transfer.p_hn_from_meshes(a2, mf.Mesh.from_leaves(2, 4, a2.cell_levels()))


# ---- 10. drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-cuda_amd", "host", "bin")


@pytest.mark.parametrize("exe,arg,name", [("poisson-pmg-2d-p4-adaptive", "3", "2d"), ("poisson-pmg-3d-p4-adaptive", "4", "3d")])
def test_poisson_pmg_adaptive_drivers(exe, arg, name):
    """dim  degree  n_dofs  levels  cg_iterations  wall_seconds  rel_error; the driver solves to 1e-12 |b|"""
    out = subprocess.run([os.path.join(BIN, exe), arg], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, exe + " " + arg + ": " + out.stdout + out.stderr
    (f,) = [ln.split() for ln in out.stdout.strip().splitlines()]
    ref = model(name)
    want_it, _ = pr.cg_iterations(ref, pr.rhs(ref), relative=1e-12)
    print(f"{exe} {arg}: {f[2]} dofs, {f[3]} levels, {f[4]} iterations (numpy model {want_it}), rel_error {f[6]}")
    assert len(f) == 7 and int(f[0]) == ADAPTIVE[name][0] and int(f[1]) == 4 and int(f[2]) == ref.mesh.n_dofs
    assert int(f[3]) == 3 and float(f[6]) < 1e-8
    assert int(f[4]) <= want_it + 2
