"""Global-coarsening multigrid: the h-transfer between two leaf meshes with hanging nodes
(mfgpu_transfer_create_h_hn, pymfgpu.Transfer.h_hn_from_*) and the V-cycles built on it, against tests/gc_reference.py
(float64 numpy on the oracle's hn_resolve, 1D h-matrix and assembled matrices).

   1. prolongate / prolongate_add / restrict_and_add against the numpy P on (coarsened, mesh) pairs of small leaf meshes
   2. <P x, y> = <x, P^T y> without the reference
   3. a polynomial of degree p per direction is reproduced at every fine dof that is not hanging
   4. a mesh against itself (all child = 0): prolongate is the identity on listed dofs, bit for bit
   5. uniform cubes n -> 2n written as leaf meshes agree with Transfer.from_meshes
   6. more cells than one pass of the capped grid covers
   7. one V-cycle of VCycle.from_global_coarsening, value for value against the numpy model
   8. CG preconditioned with it against a direct solve
   9. refresh after update_coefficients equals a fresh object
  10. apply is graph-capturable
  11. errors, with the free device memory unchanged
  12. the poisson-gc-*-adaptive drivers

Tolerances are those of the existing tests for the same comparisons (TRANSFER_TOL, VCYCLE_TOL, REFRESH_TOL, GRAPH_TOL,
iterations <= the numpy model's + 2).  The adjointness test compares two dot products over N = 6902 fine dofs, each a sum
with a rounding error of about sqrt(N) eps |P x| |y| = 2e-14 |P x| |y|; its bound is 1e-13 |P x| |y|."""
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

import gc_reference as gr
import pmg_reference as pr
import pymfgpu as mf
from hn_reference import match_by_position
from oracle import mf_oracle as o
from test_gpu_pmg import GRAPH_TOL, TRANSFER_TOL, dev, rel, typed
from test_gpu_pmg_hn import check_parity_hn, unlisted
from test_gpu_refresh import REFRESH_TOL, apply_all, defects
from test_gpu_vcycle import VCYCLE_TOL, capture_and_replay
from test_hanging_host import CASES

pytestmark = pytest.mark.gpu

F64, F32 = mf.F64, mf.F32
TYPES = pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float"])
NTNAME = {F64: "double", F32: "float"}


def pair(name, p, nt=F64):
    """(dim, coarsened mesh, mesh) of a small case at degree p"""
    dim, leaves = CASES[name]
    return (dim, mf.Mesh.from_leaves(dim, p, mf.Mesh.coarsen_leaves(dim, leaves), number_type=nt),
            mf.Mesh.from_leaves(dim, p, leaves, number_type=nt))


def array_args(dim, p, c, f):
    ca, fa = c.arrays(), f.arrays()
    parent, child = mf.coarsening_map(c, f)
    return (dim, p, ca["loc2glob"], fa["loc2glob"], parent, child, c.n_dofs, f.n_dofs), \
        dict(coarse_mask=ca["constraint_mask"], fine_mask=fa["constraint_mask"])


# ---- 1. parity of the three calls

# what makes the cases hard: fine cells -> coarse cells, unchanged cells, refined parents, refined parents with a coarse mask
HARD = {"3d_two": (85, 29, 21, 8, 3), "2d_center": (22, 10, 6, 4, 2)}


@TYPES
@pytest.mark.parametrize("p", [1, 2, 4, 6])
@pytest.mark.parametrize("name", ["3d_two", "2d_center", "2d_L", "3d_edge", "3d_slab"])
def test_parity_on_coarsened_pairs(name, p, nt):
    dim, c, f = pair(name, p, nt)
    ca, fa = c.arrays(), f.arrays()
    parent, child = mf.coarsening_map(c, f)
    refined = np.unique(parent[child != 0])
    cm = ca["constraint_mask"]
    if name in HARD:
        masked = int((cm[refined] != 0).sum())
        assert (f.n_cells, c.n_cells, int((child == 0).sum()), len(refined), masked) == HARD[name]
        # unchanged cells that carry a coarse mask they do not have in the fine mesh
        same = child == 0
        assert (cm[parent[same]] != fa["constraint_mask"][same]).any()
    assert (fa["constraint_mask"] != 0).any() and len(refined) and (child == 0).any()
    con = ca["constrained_dofs"].astype(np.int64)
    hanging = unlisted(f)
    what = f"{name} p = {p} ({c.n_cells} -> {f.n_cells} cells) {NTNAME[nt]}"
    P = gr.mesh_pair_matrix_gc(c, f)
    check_parity_hn(mf.Transfer.h_hn_from_meshes(c, f), P, con, nt, what + " from_meshes", hanging)
    args, masks = array_args(dim, p, c, f)
    t = mf.Transfer.h_hn_from_arrays(*args, con, nt, prolongation_1d=o.mg_prolongation_1d(p),
                                     constraint_weights=o.constraint_weights(p), **masks)
    check_parity_hn(t, P, con, nt, what + " from_arrays with an explicit P1 and weights", hanging)
    none = np.zeros(0, dtype=np.int64)
    P = gr.mesh_pair_matrix_gc(c, f, dirichlet=none)
    check_parity_hn(mf.Transfer.h_hn_from_arrays(*args, none, nt, **masks), P, none, nt,
                    what + " from_arrays without Dirichlet dofs", hanging)


# ---- 2. adjointness


def test_restriction_is_the_transpose_of_prolongation():
    dim, c, f = pair("3d_two", 4)
    args, masks = array_args(dim, 4, c, f)
    t = mf.Transfer.h_hn_from_arrays(*args, [], **masks)
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
    print(f"3d_two p = 4, {f.n_dofs} fine dofs: <P x, y> = {lhs:.15e}, <x, P^T y> = {rhs:.15e}, difference / (|P x| |y|) "
          f"{abs(lhs - rhs) / scale:.2e}")
    assert f.n_dofs == 6902 and scale > 0 and abs(lhs - rhs) <= 1e-13 * scale


# ---- 3. a known answer


@pytest.mark.parametrize("p", [1, 2, 4, 6])
@pytest.mark.parametrize("name", ["3d_two", "2d_L", "3d_edge"])
def test_polynomials_of_degree_p_are_reproduced(name, p):
    dim, c, f = pair(name, p)
    args, masks = array_args(dim, p, c, f)
    t = mf.Transfer.h_hn_from_arrays(*args, [], **masks)
    coef = np.random.default_rng(10 * p + dim).uniform(0.5, 1.5, (dim, p + 1))

    def poly(X):  # degree p per direction
        return np.prod([np.polyval(coef[d], X[:, d]) for d in range(dim)], axis=0)

    fine = mf.DeviceVector(f.n_dofs)
    fine.fill(3.0)
    t.prolongate(fine, dev(poly(c.dof_coords())))
    mf.synchronize()
    sel = ~unlisted(f)
    err = rel(fine.to_host()[sel], poly(f.dof_coords())[sel])
    print(f"{name} p = {p}: a polynomial of degree {p} per direction, rel l2 at the {sel.sum()} fine dofs that are not "
          f"hanging {err:.2e}")
    assert err <= 1e-13


# ---- 4. a mesh against itself


@TYPES
@pytest.mark.parametrize("p", [1, 4])
@pytest.mark.parametrize("name", ["3d_two", "2d_L"])
def test_a_mesh_against_itself_is_the_identity(name, p, nt):
    dim, leaves = CASES[name]
    f = mf.Mesh.from_leaves(dim, p, leaves, number_type=nt)
    parent, child = mf.coarsening_map(f, f)
    assert not child.any()
    a = f.arrays()
    t = mf.Transfer.h_hn_from_arrays(dim, p, a["loc2glob"], a["loc2glob"], parent, child, f.n_dofs, f.n_dofs, [], nt,
                                     coarse_mask=a["constraint_mask"], fine_mask=a["constraint_mask"])
    x = np.random.default_rng(p).standard_normal(f.n_dofs).astype(mf.np_dtype(nt))
    fine = mf.DeviceVector(f.n_dofs, nt)
    fine.fill(3.0)
    t.prolongate(fine, dev(x, nt))
    mf.synchronize()
    got, hanging = fine.to_host(), unlisted(f)
    assert hanging.any() and not got[hanging].any()
    np.testing.assert_array_equal(got[~hanging], x[~hanging])  # bit for bit


# ---- 5. uniform cubes as leaf meshes


@TYPES
@pytest.mark.parametrize("dim,p,level", [(2, 3, 1), (3, 2, 1), (3, 4, 0), (2, 1, 2)])
def test_uniform_leaf_meshes_agree_with_the_level_transfer(dim, p, level, nt):
    def uniform_leaves(l):
        r = range(1 << l)
        return [[l, x, y, z] for z in (r if dim == 3 else [0]) for y in r for x in r]

    lc, lf = (mf.Mesh.from_leaves(dim, p, uniform_leaves(l), number_type=nt) for l in (level, level + 1))
    uc, uf = (mf.Mesh.uniform(dim, p, 1 << l, number_type=nt) for l in (level, level + 1))
    assert lc.arrays()["constraint_mask"] is None and lf.arrays()["constraint_mask"] is None
    ic, jf = match_by_position(lc.dof_coords(), uc.dof_coords()), match_by_position(lf.dof_coords(), uf.dof_coords())
    rng = np.random.default_rng(dim + 10 * p)
    x, y, z = (typed(rng.standard_normal(n), nt) for n in (uc.n_dofs, uf.n_dofs, uc.n_dofs))

    def three(t, x, y, z):
        fine, acc, coarse = mf.DeviceVector(len(y), nt), dev(y, nt), dev(z, nt)
        fine.fill(3.0)
        t.prolongate(fine, dev(x, nt))
        t.prolongate_add(acc, dev(x, nt))
        t.restrict_and_add(coarse, dev(y, nt))
        mf.synchronize()
        return [v.to_host().astype(np.float64) for v in (fine, acc, coarse)]

    want = three(mf.Transfer.from_meshes(uc, uf), x, y, z)
    got = three(mf.Transfer.h_hn_from_meshes(lc, lf), x[ic], y[jf], z[ic])  # leaf numbering: v_leaf[i] = v_uniform[index[i]]
    errs = [rel(got[0], want[0][jf]), rel(got[1], want[1][jf]), rel(got[2], want[2][ic])]
    print(f"{dim}D p = {p}, {uc.n_cells} -> {uf.n_cells} cells {NTNAME[nt]}: leaf meshes against the level transfer, "
          f"prolongate {errs[0]:.2e}, prolongate_add {errs[1]:.2e}, restrict_and_add {errs[2]:.2e}")
    assert max(errs) <= TRANSFER_TOL[nt]


# ---- 6. more cells than one pass


@functools.lru_cache(maxsize=None)
def large_pair_matrix():
    f = mf.Mesh.adaptive(3, 1, 5)
    return gr.mesh_pair_matrix_gc(mf.Mesh.coarsening_sequence(f)[-2], f)


@TYPES
def test_more_cells_than_one_pass_of_the_grid(nt):
    f = mf.Mesh.adaptive(3, 1, 5, number_type=nt)
    c = mf.Mesh.coarsening_sequence(f)[-2]
    assert f.n_cells == 33797 > 4 * 2048 and c.n_cells == 7099
    con = c.arrays()["constrained_dofs"].astype(np.int64)
    check_parity_hn(mf.Transfer.h_hn_from_meshes(c, f), large_pair_matrix(), con, nt,
                    f"3D adaptive n_ref 5, 7099 -> 33797 cells p = 1 {NTNAME[nt]}", unlisted(f))


# ---- 7. / 8. the V-cycle

ADAPTIVE = {"2d": (2, 3), "3d": (3, 4)}  # (dim, n_ref)
KINDS = {"h": (4,), "p": (1, 2, 4)}      # the degrees of from_global_coarsening


def gc_meshes(name, kind, nt=F64):
    """what from_global_coarsening builds: the coarsening sequence at the lowest degree, then the rising degrees"""
    dim, n_ref = ADAPTIVE[name]
    degrees = KINDS[kind]
    mesh = mf.Mesh.adaptive(dim, 4, n_ref, number_type=nt)
    meshes = mf.Mesh.coarsening_sequence(mesh, degrees[0])
    meshes += [mf.Mesh.from_leaves(dim, d, mesh.cell_levels(), number_type=nt) for d in degrees[1:-1]]
    return meshes + ([mesh] if len(degrees) > 1 else []), mesh


@functools.lru_cache(maxsize=None)
def model(name, kind):
    """the float64 hierarchy with exact smoother bounds (shared, never modified)"""
    return gr.level_hierarchy_gc(gc_meshes(name, kind)[0])


@functools.lru_cache(maxsize=None)
def level_defects(name):
    return defects(gc_meshes(name, "h")[1], 11 + len(name))


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float_levels"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", list(ADAPTIVE))
def test_one_vcycle_value_for_value(name, kind, nt):
    dim, n_ref = ADAPTIVE[name]
    V = mf.VCycle.from_global_coarsening(mf.Mesh.adaptive(dim, 4, n_ref, number_type=nt), KINDS[kind], F64)
    ref = pr.with_lambda_max(model(name, kind), V.lambda_max())  # estimated lambda_max
    cells = [M.n_cells for M in ref.meshes]
    want_cells = {"2d": [4, 16, 28, 61, 136], "3d": [8, 22, 78, 253, 736]}[name]
    assert cells == want_cells + [want_cells[-1]] * (len(KINDS[kind]) - 1) and V.n_levels == ref.n_levels == len(cells)
    assert [int(M.desc.degree) for M in ref.meshes][-len(KINDS[kind]):] == list(KINDS[kind])
    R = level_defects(name)
    got = apply_all(V, R)
    want = ref.vcycle(R)
    errs = [rel(got[:, k], want[:, k]) for k in range(R.shape[1])]
    print(f"V-cycle global coarsening {name} degrees {KINDS[kind]} ({R.shape[0]} dofs, {V.n_levels} levels, level 0 "
          f"{ref.meshes[0].n_dofs} dofs) {NTNAME[nt]} levels: rel l2 from the numpy model with the object's lambda_max, "
          f"largest of {len(errs)}: {max(errs):.3e}")
    assert max(errs) <= VCYCLE_TOL[nt], errs


def test_from_global_coarsening_is_from_level_meshes_over_the_sequence():
    meshes, mesh = gc_meshes("2d", "p")
    V, W = mf.VCycle.from_global_coarsening(mesh, KINDS["p"]), mf.VCycle.from_level_meshes(meshes)
    assert V.n_levels == W.n_levels == len(meshes)
    R = level_defects("2d")
    # (two estimates of the same operators: their reductions add atomically, so equal up to rounding, as in refresh)
    np.testing.assert_allclose(V.lambda_max(), W.lambda_max(), rtol=64 * np.finfo(np.float64).eps, atol=0.0)
    assert max(rel(a, b) for a, b in zip(apply_all(V, R).T, apply_all(W, R).T)) <= VCYCLE_TOL[F64]
    with pytest.raises(mf.MfgpuError):
        mf.VCycle.from_global_coarsening(mesh, (1, 2))  # does not end at the mesh's degree
    with pytest.raises(mf.MfgpuError):
        mf.VCycle.from_global_coarsening(mesh, (2, 1, 4))


@functools.lru_cache(maxsize=None)
def direct_solution(name, kind):
    ref = model(name, kind)
    # (the minimum-degree ordering of A^T + A: the matrix is symmetric, and the default ordering takes 20 times as long)
    return spla.spsolve(ref.A[-1].tocsc(), pr.rhs(ref, seed=ref.mesh.n_dofs), permc_spec="MMD_AT_PLUS_A")


@pytest.mark.parametrize("name,kind", [("2d", "h"), ("2d", "p"), ("3d", "p")])
def test_cg_with_the_vcycle(name, kind):
    """CG to 1e-10 relative on the active mesh's operator in double with the V-cycle as preconditioner"""
    dim, n_ref = ADAPTIVE[name]
    ref = model(name, kind)
    mesh = ref.mesh
    b = pr.rhs(ref, seed=mesh.n_dofs)
    want_it, _ = pr.cg_iterations(ref, b)
    xr = direct_solution(name, kind)
    its = {}
    for nt in (F64, F32):
        V = mf.VCycle.from_global_coarsening(mf.Mesh.adaptive(dim, 4, n_ref, number_type=nt), KINDS[kind], F64)
        cg = mf.CG(mf.Operator(mesh.desc, mesh), mf.CG_CALLBACK)
        cg.set_vcycle(V)
        x = mf.DeviceVector(mesh.n_dofs)
        info = cg.solve(x, dev(b), 1e-10 * np.linalg.norm(b), 100)
        its[nt] = info.iterations
        assert info.status == 1 and info.residual <= 1e-10 * np.linalg.norm(b)
        assert np.linalg.norm(x.to_host() - xr) <= 1e-8 * np.linalg.norm(xr)
    print(f"CG + global-coarsening V-cycle {name} degrees {KINDS[kind]} ({len(b)} dofs): {its[F64]} iterations with double "
          f"levels, {its[F32]} with float levels, numpy model {want_it}")
    assert its[F64] <= want_it + 2 and its[F32] <= its[F64] + 2


# ---- 9. / 10. refresh, graph capture


def field2(x):
    """a smooth positive coefficient at quadrature points x [..., 2]"""
    return 1.0 + x[..., 0] ** 2 + 2.0 * x[..., 1] ** 2


@pytest.mark.parametrize("kind", list(KINDS))
def test_refreshed_is_fresh(kind):
    """test_gpu_pmg_hn.py::test_refreshed_is_fresh over the coarsened 2D meshes (level 0: 4 cells)"""
    nt = F64
    meshes, mesh = gc_meshes("2d", kind, nt)
    levels = mf.VCycle.level_mesh_levels(meshes, flags=mf.UPDATABLE_COEFFICIENTS)
    N = mesh.n_dofs
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
    assert info.coarse_status == 0 and info.eig_steps_max <= 200
    np.testing.assert_allclose(V.lambda_max()[1:], W.lambda_max()[1:], rtol=64 * np.finfo(np.float64).eps, atol=0.0)
    err = max(rel(got[:, j], want[:, j]) for j in range(3))
    moved = min(rel(stale[:, j], want[:, j]) for j in range(3))
    print(f"refresh global coarsening 2d degrees {KINDS[kind]}: refreshed against fresh, largest rel l2 of 3: {err:.3e}; "
          f"before the refresh {moved:.3e}")
    assert moved > 100 * REFRESH_TOL[nt]
    assert err <= REFRESH_TOL[nt]


def test_apply_is_graph_capturable():
    if torch is None:
        pytest.skip("torch is not installed")
    assert torch.cuda.is_available()
    V = mf.VCycle.from_global_coarsening(gc_meshes("3d", "p")[1], KINDS["p"])
    R = level_defects("3d")
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


# ---- 11. errors


def test_errors_are_loud_and_create_nothing():
    dim, c, f = pair("2d_center", 2)
    ca, fa = c.arrays(), f.arrays()
    cd, fd, con = ca["loc2glob"], fa["loc2glob"], ca["constrained_dofs"]
    cmask, fmask = ca["constraint_mask"], fa["constraint_mask"]
    parent, child = mf.coarsening_map(c, f)
    mf.Transfer.h_hn_from_meshes(c, f)  # (code objects, tables: what a first call leaves behind)
    mf.synchronize()
    free0, _ = mf.device_memory_info()

    def raises(code, fn, *args, **kw):
        with pytest.raises(mf.MfgpuError) as e:
            fn(*args, **kw)
        assert e.value.code == code, str(e.value)

    def arrays(p=2, cd=cd, fd=fd, parent=parent, child=child, nc=c.n_dofs, nf=f.n_dofs, con=con, cmask=cmask, fmask=fmask,
               dim=2):
        return mf.Transfer.h_hn_from_arrays(dim, p, cd, fd, parent, child, nc, nf, con, coarse_mask=cmask, fine_mask=fmask)

    def changed(a, i, v):
        a = a.copy()
        a[i] = v
        return a

    arrays()
    raises(mf.EINVAL, arrays, parent=changed(parent, 3, c.n_cells))            # a parent out of range
    raises(mf.EINVAL, arrays, child=changed(child, 0, 5))                      # a child > 2^dim
    for mask in ("cmask", "fmask"):
        m = cmask if mask == "cmask" else fmask
        raises(mf.EINVAL, arrays, **{mask: changed(m, 0, m[0] | np.uint32(1 << 9))})   # a bit outside the 9 defined ones
        raises(mf.EINVAL, arrays, **{mask: changed(m, 0, m[0] | np.uint32(1 << 31))})
        for bit in (2, 5, 6, 7, 8):                                            # 3D bits in 2D
            raises(mf.EINVAL, arrays, **{mask: changed(m, 0, m[0] | np.uint32(1 << bit))})
    # two cells that share a face and both flag it: the dofs inside the face are listed, and nobody owns them
    u = mf.Mesh.uniform(2, 2, (2, 1))
    ul, two = u.arrays()["loc2glob"], np.arange(2, dtype=np.uint32)
    same = dict(cd=ul, fd=ul, parent=two, child=0 * two, nc=u.n_dofs, nf=u.n_dofs, con=u.arrays()["constrained_dofs"], cmask=None)
    raises(mf.EINVAL, arrays, fmask=np.array([1 << 3, (1 << 3) | 1], dtype=np.uint32), **same)
    arrays(fmask=np.array([1 << 3, 0], dtype=np.uint32), **same)               # (flagged on one side only)
    raises(mf.EINVAL, arrays, 0)                                               # degrees outside 1..6
    raises(mf.EINVAL, arrays, 7)
    raises(mf.EINVAL, arrays, dim=4)
    raises(mf.EINVAL, arrays, nc=c.n_dofs - 1)                                 # a coarse dof out of range
    raises(mf.EINVAL, arrays, nf=f.n_dofs - 1)
    raises(mf.EINVAL, arrays, con=np.array([c.n_dofs], dtype=np.uint32))
    raises(mf.EINVAL, arrays, nf=1 << 31)
    h = mf.C.c_void_p()
    L = mf.lib()

    def raw(cd=cd.ctypes.data, fd=fd.ctypes.data, pa=parent.ctypes.data, ch=child.ctypes.data, out=mf.C.byref(h)):
        return L.mfgpu_transfer_create_h_hn(2, 2, F64, c.n_cells, f.n_cells, cd, fd, pa, ch, c.n_dofs, f.n_dofs, None, 0, None,
                                            cmask.ctypes.data, fmask.ctypes.data, None, out)

    for null in ("cd", "fd", "pa", "ch"):                                      # null arrays
        assert raw(**{null: None}) == mf.EINVAL and not h.value
    assert raw(out=None) == mf.EINVAL
    assert L.mfgpu_transfer_create_h_hn_from_meshes(c._h, None, mf.C.byref(h)) == mf.EINVAL and not h.value
    assert L.mfgpu_transfer_create_h_hn_from_meshes(None, f._h, mf.C.byref(h)) == mf.EINVAL and not h.value
    raises(mf.EINVAL, mf.Transfer.h_hn_from_meshes, f, c)                                       # the fine mesh first
    raises(mf.EINVAL, mf.Transfer.h_hn_from_meshes, c, mf.Mesh.from_leaves(2, 4, CASES["2d_center"][1]))  # two degrees
    raises(mf.EINVAL, mf.Transfer.h_hn_from_meshes, c, mf.Mesh.from_leaves(2, 2, CASES["2d_L"][1]))       # other leaves
    raises(mf.EINVAL, mf.Transfer.h_hn_from_meshes, c, mf.Mesh.from_leaves(3, 2, CASES["3d_corner"][1]))  # two dimensions
    raises(mf.EINVAL, mf.Transfer.h_hn_from_meshes, mf.Mesh.uniform(2, 2, 2), mf.Mesh.uniform(2, 2, 4))   # cubes
    raises(mf.EINVAL, mf.Transfer.h_hn_from_meshes, mf.Mesh.uniform(2, 2, 2), f)
    mf.synchronize()
    assert mf.device_memory_info()[0] == free0
    # the conforming cubes and balls keep their transfer in level_mesh_levels; leaf meshes get the new one
    mf.VCycle.level_mesh_levels([mf.Mesh.uniform(2, 2, 2), mf.Mesh.uniform(2, 2, 4)])
    assert mf.VCycle.level_mesh_levels([c, f])[1]["transfer"].memory_consumption() == mf.Transfer.h_hn_from_meshes(c, f).memory_consumption()


# ---- 12. drivers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-cuda_amd", "host", "bin")


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("exe,arg,name", [("poisson-gc-2d-p4-adaptive", "3", "2d"), ("poisson-gc-3d-p4-adaptive", "4", "3d")])
def test_poisson_gc_drivers(exe, arg, name, kind):
    """dim  degree  n_dofs  levels  cg_iterations  wall_seconds  rel_error; the driver solves to 1e-12 |b|"""
    args = [arg] + (["p"] if kind == "p" else [])
    out = subprocess.run([os.path.join(BIN, exe), *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, exe + " " + " ".join(args) + ": " + out.stdout + out.stderr
    (f,) = [ln.split() for ln in out.stdout.strip().splitlines()]
    ref = model(name, kind)
    want_it, _ = pr.cg_iterations(ref, pr.rhs(ref), relative=1e-12)
    print(f"{exe} {' '.join(args)}: {f[2]} dofs, {f[3]} levels, {f[4]} iterations (numpy model {want_it}), rel_error {f[6]}")
    assert len(f) == 7 and int(f[0]) == ADAPTIVE[name][0] and int(f[1]) == 4 and int(f[2]) == ref.mesh.n_dofs
    assert int(f[3]) == ref.n_levels and float(f[6]) < 1e-8
    assert int(f[4]) <= want_it + 2
