"""Piece-wise GPU parity of multigrid on ADAPTIVE hierarchies: the product's own hierarchy (mf.Mesh.adaptive_mg +
mf.MgHierarchy: non-box cell sets in octree numbering, refinement edges with corners that reach the boundary) together
with the GPU pieces, every piece against oracle/mf_oracle.py on util.oracle_desc_from_mesh(level_mesh, float64).
The convergence tests (test_gpu_mg_adaptive.py, the poisson-mg drivers) cannot see a subtly wrong piece: a V-cycle with a
wrong level matrix, interface matrix or transfer is still a usable preconditioner.

  a. every level of every hierarchy: Level.vmult, its inverse diagonal (edge and Dirichlet rows exactly 1),
     vmult_interface_down / _up, dst prefilled, src unchanged, <down x, y> = <x, up y> on the GPU results;
  b. the same four checks on general geometry (balls, a deformed cube: a full J^-1 per point) with the edge of a cell
     subset, and with a mass term against tests/helmholtz_reference.py;
  c. mfgpu_transfer_* on the hierarchy's transfer arrays of every level pair, also where only some coarse cells are
     parents;
  d. the transfer kernel's grid-stride loop: more coarse cells than the 8192 workgroups of its grid, per entry;
  e. ONE V-cycle, value for value, in the schedule of test_gpu_mg_adaptive.py::v_step against tests/mg_reference.py
     (float64 numpy, kept honest by tests/test_mg_reference_host.py), lambda_max of every level handed to both sides.

n_ref of the 2D cases: Mesh.adaptive_mg(2, p, n_ref) is the same 145-cell mesh for n_ref <= 3, and the only 2D one whose
refinement edge reaches the boundary (level 3); from n_ref = 4 on the refined region stays inside.  The 2D cases
therefore run at n_ref = 3 with both assertions (an edge that meets Dirichlet dofs, an edge that does not) and again at
the larger n_ref = 5 / 4 (12 - 13 levels, up to 40000 level dofs) where only interior edges exist.

Tolerances are the project's: operator and interface products relative l2 1e-12 / 1e-5 (test_gpu.TOL), transfers
1e-13 / 1e-5 (test_gpu_transfer.py), inverse diagonal rtol 1e-12 / 1e-5; a float reference sees the inputs rounded to
float first.

The V-cycle of (e) is a composition of about 40 applies per level.  Measured on the MI355X, relative l2 difference of z
from the numpy reference, largest of three defects and two runs (the atomics of restrict_and_add land in another order
every run):
    adaptive_mg(2, 2, 5): double 1.62e-15, float levels 3.45e-07
    adaptive_mg(3, 2, 4): double 7.07e-16, float levels 1.70e-07
The test asserts 10 times the larger value of a type, rounded up to one digit: 2e-14 and 4e-6 (the margin covers the
order in which the atomics of restrict_and_add land and another host's BLAS).  Both are far below the caps 1e-9 / 1e-4,
which are conditions, not measurements: a wrong piece moves z by percent, and lambda_max times 1.01 on one side alone
moves it by 2e-4 to 6e-4."""
import functools

import numpy as np
import pytest

import helmholtz_reference as hr
import mg_reference as mg
import pymfgpu as mf
from oracle import mf_oracle as o
from test_gpu import TOL, rel
from util import deform, desc_from_oracle, oracle_desc_from_mesh

pytestmark = pytest.mark.gpu

F64, F32 = mf.F64, mf.F32
TRANSFER_TOL = {F64: 1e-13, F32: 1e-5}
DIAG_RTOL = {F64: 1e-12, F32: 1e-5}
VCYCLE_TOL = {F64: 2e-14, F32: 4e-6}  # 10 x the largest measured value (docstring); the caps are 1e-9 / 1e-4
NTNAME = {F64: "double", F32: "float"}

# (dim, p, n_ref, number type, the case has a refinement edge that reaches the boundary)
HIERARCHIES = [(2, 2, 3, F64, True), (2, 4, 3, F64, True), (3, 1, 5, F64, True), (3, 2, 4, F64, True), (3, 3, 4, F64, True),
               (3, 4, 4, F64, True), (2, 2, 3, F32, True), (3, 4, 4, F32, True),
               (2, 2, 5, F64, False), (2, 4, 4, F64, False), (2, 2, 5, F32, False)]
HIERARCHY_IDS = [f"{d}d_p{p}_r{r}_{NTNAME[nt]}" for d, p, r, nt, _ in HIERARCHIES]


@functools.lru_cache(maxsize=None)
def hierarchy(dim, p, n_ref, nt):
    """host only: the hierarchy and the oracle descriptions of its levels, shared by the tests (never modified)"""
    return mg.Hierarchy(dim, p, n_ref, number_type=nt, matrices=False)


def typed(a, nt):
    """the values a vector of the number type holds, as doubles"""
    return np.asarray(a).astype(mf.np_dtype(nt)).astype(np.float64)


def dev(a, nt):
    v = mf.DeviceVector(len(a), nt)
    v.from_host(a)
    return v


def random_c(od, nt, seed):
    """mass coefficient in [0.5, 1.5] per quadrature point, as test_gpu_helmholtz.random_c"""
    return typed(np.random.default_rng(seed).uniform(0.5, 1.5, (od.n_cells, od.nd)), nt)


def check_level(desc, keep, od, E, nt, seed, c=None):
    """The four checks on one level.  od: float64 oracle description with the Dirichlet dofs constrained; E: edge dofs;
    c: mass coefficient already in desc (the reference is then tests/helmholtz_reference.py)"""
    n, dt = od.n_dofs, mf.np_dtype(nt)
    E = np.asarray(E, dtype=np.uint32)
    C = np.union1d(od.constrained, E).astype(np.uint32)
    odc = mg.with_constrained(od, C)
    if c is None:
        ref_vmult = lambda x: o.vmult(odc, x)
        ref_diag = lambda: o.compute_inverse_diagonal(odc)
        ref_down = lambda x: o.vmult_interface_down(od, E, x)
        ref_up = lambda x: o.vmult_interface_up(od, E, x)
    else:
        ref_vmult = lambda x: hr.vmult(odc, c, x)
        ref_diag = lambda: hr.inverse_diagonal(odc, c)
        ref_down = lambda x: hr.vmult_interface_down(od, c, E, x)
        ref_up = lambda x: hr.vmult_interface_up(od, c, E, x)
    lev = mf.Level(desc, E, keep)
    rng = np.random.default_rng(seed)
    x, y = typed(rng.standard_normal(n), nt), typed(rng.standard_normal(n), nt)
    a, b = dev(x, nt), mf.DeviceVector(n, nt)

    def run(fn, src, src_host):
        b.fill(5.0)
        fn(b, src)
        mf.synchronize()
        np.testing.assert_array_equal(src.to_host(), src_host.astype(dt))  # src unchanged
        return b.to_host().astype(np.float64)

    # level matrix: identity rows on Dirichlet AND edge dofs
    e = rel(run(lev.vmult, a, x), ref_vmult(x))
    assert e <= TOL[nt], ("vmult", e)
    # inverse diagonal: rows of Dirichlet and edge dofs exactly 1
    d = mf.DeviceVector(n, nt)
    d.fill(5.0)
    lev.compute_inverse_diagonal(d)
    mf.synchronize()
    got = d.to_host().astype(np.float64)
    np.testing.assert_array_equal(got[C], 1.0)
    np.testing.assert_allclose(got, ref_diag(), rtol=DIAG_RTOL[nt])
    # interface matrices
    if len(E) == 0:
        assert not run(lev.vmult_interface_down, a, x).any() and not run(lev.vmult_interface_up, a, x).any()
        return
    down, want = run(lev.vmult_interface_down, a, x), ref_down(x)
    assert np.linalg.norm(want) > 0 and np.linalg.norm(down - want) <= TOL[nt] * np.linalg.norm(want), "interface_down"
    up, want = run(lev.vmult_interface_up, a, x), ref_up(x)
    assert np.linalg.norm(want) > 0 and np.linalg.norm(up - want) <= TOL[nt] * np.linalg.norm(want), "interface_up"
    if nt == F64:
        # transposes of each other, on the GPU results: each side is within TOL of an exact pair of equal numbers, and
        # the host's two dot products round by less than that (n 2^-53 << 1e-12)
        a.from_host(y)
        up_y = run(lev.vmult_interface_up, a, y)
        bound = 2.0 * TOL[nt] * (np.linalg.norm(down) * np.linalg.norm(y) + np.linalg.norm(x) * np.linalg.norm(up_y))
        assert abs(down @ y - x @ up_y) <= bound


# ---- a. level pieces on every hierarchy level


@pytest.mark.parametrize("dim,p,n_ref,nt,reaches_boundary", HIERARCHIES, ids=HIERARCHY_IDS)
def test_level_pieces_on_every_hierarchy_level(dim, p, n_ref, nt, reaches_boundary):
    h = hierarchy(dim, p, n_ref, nt)
    touching = [l for l in range(h.n_levels) if len(np.intersect1d(h.edge[l], h.od[l].constrained))]
    inside = [l for l in range(h.n_levels) if len(h.edge[l]) and l not in touching]
    assert inside and bool(touching) == reaches_boundary, (touching, inside)
    for l in range(h.n_levels):
        M = h.meshes[l]
        check_level(M.desc, (M, h), h.od[l], h.edge[l], nt, seed=100 * dim + 10 * p + l)


# ---- b. interface matrices on general geometry and with a mass term


def subset_edge(od):
    """what a refinement edge is: the dofs referenced both by a cell of S and by a cell outside S; S = the first third
    of the cells in mesh order"""
    k = od.n_cells // 3
    E = np.intersect1d(od.loc2glob[:k], od.loc2glob[k:]).astype(np.uint32)
    assert 0 < len(E) < od.n_dofs
    return E


@pytest.mark.parametrize("what,nt", [("ball_3d_p2", F64), ("ball_2d_p4", F64), ("deformed_3d_p3", F64), ("ball_3d_p2", F32)],
                         ids=lambda v: NTNAME.get(v, v) if isinstance(v, int) else v)
def test_level_pieces_on_general_geometry(what, nt):
    if what.startswith("ball"):
        mesh = mf.Mesh.ball(3, 2, 2, number_type=nt) if what == "ball_3d_p2" else mf.Mesh.ball(2, 4, 2, number_type=nt)
        od = oracle_desc_from_mesh(mesh, dtype=np.float64)
        desc, keep = mesh.desc, mesh
        E = subset_edge(od)
        assert len(np.intersect1d(E, od.constrained)) > 0  # the edge reaches the boundary of the ball
    else:
        od = deform(o.uniform_mesh_desc(3, 3, 4))
        desc, keep = desc_from_oracle(od, number_type=nt)
        E = subset_edge(od)
    assert not (desc.flags & mf.UNIFORM_J0)  # a full J^-1 per quadrature point
    check_level(desc, keep, od, E, nt, seed=7)


@pytest.mark.parametrize("what", ["ball_3d_p2", "adaptive_mg_3d_p2_r4"])
def test_level_pieces_with_a_mass_term(what):
    if what == "ball_3d_p2":
        mesh = mf.Mesh.ball(3, 2, 2)
        od = oracle_desc_from_mesh(mesh, dtype=np.float64)
        E, keep = subset_edge(od), mesh
    else:
        h = hierarchy(3, 2, 4, F64)
        l = max(l for l in range(h.n_levels) if len(np.intersect1d(h.edge[l], h.od[l].constrained)))
        mesh = h.H.level_mesh(l)  # a description of its own: the shared one stays without the term
        od, E, keep = h.od[l], h.edge[l], (mesh, h)
    c = random_c(od, F64, seed=11)
    mesh.set_mass_coefficient(c)
    check_level(mesh.desc, keep, od, E, F64, seed=8, c=c)
    # (the term is there)
    x = np.random.default_rng(9).standard_normal(od.n_dofs)
    want = hr.vmult_interface_down(od, c, E, x)
    assert np.linalg.norm(want - o.vmult_interface_down(od, E, x)) > 1e-6 * np.linalg.norm(want)


# ---- c. transfers of the hierarchy


@pytest.mark.parametrize("dim,p,n_ref,nt,reaches_boundary", HIERARCHIES, ids=HIERARCHY_IDS)
def test_transfers_of_the_hierarchy(dim, p, n_ref, nt, reaches_boundary):
    h = hierarchy(dim, p, n_ref, nt)
    dt, tol = mf.np_dtype(nt), TRANSFER_TOL[nt]
    rng = np.random.default_rng(1000 * dim + 10 * p + n_ref)
    partial = 0
    for l in range(1, h.n_levels):
        cd, fd = h.patches[l]
        C, F = h.od[l - 1], h.od[l]
        nc, nf, con = C.n_dofs, F.n_dofs, C.constrained
        t = mf.Transfer.from_arrays(dim, p, cd, fd, nc, nf, con, nt)
        x, y, z = (typed(rng.random(k), nt) for k in (nc, nf, nc))
        a, b = dev(x, nt), mf.DeviceVector(nf, nt)
        b.fill(3.0)  # prolongate overwrites
        t.prolongate(b, a)
        mf.synchronize()
        # (not rel(): the coarsest level of a p = 1 hierarchy has Dirichlet dofs only, and P of it is exactly zero)
        got, want = b.to_host().astype(np.float64), o.mg_prolongate(dim, p, cd, fd, nf, con, x)
        assert np.linalg.norm(got - want) <= tol * np.linalg.norm(want), (l, "prolongate")
        a.from_host(z)
        b.from_host(y)
        t.restrict_and_add(a, b)
        mf.synchronize()
        got, want = a.to_host(), o.mg_restrict_and_add(dim, p, cd, fd, nc, con, z, y)
        assert np.linalg.norm(got - want) <= tol * np.linalg.norm(want), (l, "restrict_and_add")
        np.testing.assert_array_equal(got[con], z.astype(dt)[con])  # coarse Dirichlet entries: bitwise unchanged
        if len(cd) < C.n_cells:  # the parents are a strict subset of the coarse level's cells
            orphan = np.setdiff1d(np.arange(nc), cd)  # coarse dofs of no parent cell
            if len(orphan):
                partial += 1
                np.testing.assert_array_equal(got[orphan], z.astype(dt)[orphan])
    assert partial > 0


# ---- d. the transfer kernel's grid-stride loop


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float"])
@pytest.mark.parametrize("dim,p,n", [(3, 1, 21), (2, 3, 91)])
def test_transfer_grid_stride_loop(dim, p, n, nt):
    """transfer_kernel walks the coarse cells with cell += gridDim.x on at most 8192 workgroups: a workgroup's second
    trip reuses its LDS arrays behind one barrier.  A race there corrupts a few patches, hence per entry."""
    mc, mfine = mf.Mesh.uniform(dim, p, n, number_type=nt), mf.Mesh.uniform(dim, p, 2 * n, number_type=nt)
    C, F = o.uniform_mesh_desc(dim, p, n), o.uniform_mesh_desc(dim, p, 2 * n)
    cd, fd = o.mg_patches_uniform(dim, p, n, C, F)
    n_coarse_cells = len(cd)
    assert n_coarse_cells == mc.n_cells and n_coarse_cells > 8192
    tol = TRANSFER_TOL[nt]
    rng = np.random.default_rng(dim * 100 + p * 10)
    x, y, z = (typed(rng.random(k), nt) for k in (C.n_dofs, F.n_dofs, C.n_dofs))
    t = mf.Transfer.from_meshes(mc, mfine)
    a, b = dev(x, nt), mf.DeviceVector(F.n_dofs, nt)
    b.fill(3.0)
    t.prolongate(b, a)
    mf.synchronize()
    want = o.mg_prolongate(dim, p, cd, fd, F.n_dofs, C.constrained, x)
    np.testing.assert_allclose(b.to_host().astype(np.float64), want, rtol=tol, atol=tol * np.abs(want).max())
    a.from_host(z)
    b.from_host(y)
    t.restrict_and_add(a, b)
    mf.synchronize()
    want = o.mg_restrict_and_add(dim, p, cd, fd, C.n_dofs, C.constrained, z, y)
    np.testing.assert_allclose(a.to_host().astype(np.float64), want, rtol=tol, atol=tol * np.abs(want).max())


# ---- e. one V-cycle, value for value


@functools.lru_cache(maxsize=None)
def vcycle_reference(dim, p, n_ref):
    """the float64 reference with its matrices and three seeded defects, zero on the constrained dofs, with values a
    float holds (both variants get the same ones), and the reference's z for each"""
    ref = mg.Hierarchy(dim, p, n_ref)
    N = ref.mesh.n_dofs
    con = ref.mesh.arrays()["constrained_dofs"]
    R = typed(np.random.default_rng(dim * 10 + p).standard_normal((N, 3)), F32)
    R[con] = 0.0
    return ref, R, ref.vcycle(R)


class _LevelOperator:
    """the level matrix of an mf.Level as the operator mf.CG takes (the handle stays the level's)"""

    def __init__(self, lev, n):
        self._lev, self._n, self.number_type = lev, n, lev.number_type
        self._h = mf.lib().mfgpu_level_operator(lev._h)

    def n(self):
        return self._n


class GpuVcycle:
    """the schedule of test_gpu_mg_adaptive.py::v_step through mf.Level, mf.Transfer and the hierarchy's copy pairs;
    nt: number type of the levels (the active vectors are double)"""

    def __init__(self, dim, p, n_ref, nt, lmax):
        self.h = h = hierarchy(dim, p, n_ref, nt)
        self.nt, self.nl, self.lmax = nt, h.n_levels, lmax
        self.n = [M.n_dofs for M in h.meshes]
        self.levs = [mf.Level(M.desc, E, (M, h)) for M, E in zip(h.meshes, h.edge)]
        vec = lambda: [mf.DeviceVector(n, nt) for n in self.n]
        self.defect, self.defect2, self.sol, self.tv, self.dinv, self.r, self.t, self.d = (vec() for _ in range(8))
        for lev, dinv in zip(self.levs, self.dinv):
            lev.compute_inverse_diagonal(dinv)
        self.tr = [None] + [mf.Transfer.from_arrays(dim, p, *h.patches[l], self.n[l - 1], self.n[l],
                                                    h.od[l - 1].constrained, nt) for l in range(1, self.nl)]
        self.to_mg = [mf.IndexPairs(b, a) for a, b in h.pairs]    # level <- active
        self.from_mg = [mf.IndexPairs(a, b) for a, b in h.pairs]  # active <- level
        self.sol64 = [mf.DeviceVector(n, F64) for n in self.n] if nt == F32 else None
        self.cg = mf.CG(_LevelOperator(self.levs[0], self.n[0]), mf.CG_NONE)
        self.coarse_status = []

    def smooth(self, l, x, b, zero_start):
        lev, dinv, r, d, t = self.levs[l], self.dinv[l], self.r[l], self.d[l], self.t[l]
        lmax = self.lmax[l]
        lmin = lmax / mg.SMOOTHING_RANGE
        theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
        sigma = theta / delta
        rho = 1.0 / sigma
        r.equ(1.0, b)
        if not zero_start:
            lev.vmult(t, x)
            r.add(-1.0, t)
        d.equ(1.0 / theta, r)
        d.scale(dinv)
        if zero_start:
            x.equ(1.0, d)
        else:
            x.add(1.0, d)
        for _ in range(mg.DEGREE - 1):
            lev.vmult(t, d)
            r.add(-1.0, t)
            rho_new = 1.0 / (2.0 * sigma - rho)
            t.equ(2.0 * rho_new / delta, r)
            t.scale(dinv)
            d.sadd(rho_new * rho, 1.0, t)
            x.add(1.0, d)
            rho = rho_new

    def v_step(self, l):
        defect, defect2, sol, tv, levs = self.defect, self.defect2, self.sol, self.tv, self.levs
        if l == 0:
            info = self.cg.solve(sol[0], defect[0], 1e-13 * defect[0].l2_norm(), 1000)
            self.coarse_status.append(int(info.status))
            return
        self.smooth(l, sol[l], defect[l], True)
        levs[l].vmult(tv[l], sol[l])                        # t = A x
        defect2[l].fill(0.0)
        levs[l].vmult_interface_down(defect2[l], sol[l])    # + the rows of the edge dofs
        tv[l].add(1.0, defect2[l])
        tv[l].sadd(-1.0, 1.0, defect[l])                    # t = defect - t
        self.tr[l].restrict_and_add(defect[l - 1], tv[l])
        sol[l - 1].fill(0.0)
        self.v_step(l - 1)
        self.tr[l].prolongate(tv[l], sol[l - 1])
        sol[l].add(1.0, tv[l])
        levs[l].vmult_interface_up(tv[l], sol[l])           # the edge values' action on the interior rows
        defect2[l].equ(1.0, defect[l])
        defect2[l].add(-1.0, tv[l])
        self.smooth(l, sol[l], defect2[l], False)

    def apply(self, r_host):
        r, z = dev(r_host, F64), mf.DeviceVector(len(r_host), F64)
        for l in range(self.nl):  # copy_to_mg
            self.defect[l].fill(0.0)
            if self.nt == F64:
                self.to_mg[l].copy(self.defect[l], r, F64)
            else:
                mf.copy_pairs_convert(self.to_mg[l], self.defect[l], F32, r, F64)
        self.sol[self.nl - 1].fill(0.0)
        self.v_step(self.nl - 1)
        z.fill(0.0)
        for l in range(self.nl):  # copy_from_mg
            if self.nt == F64:
                self.from_mg[l].copy(z, self.sol[l], F64)
            else:
                mf.vec_convert(self.sol64[l], F64, self.sol[l], F32, self.n[l])
                self.from_mg[l].copy(z, self.sol64[l], F64)
        mf.synchronize()
        return z.to_host()


@pytest.mark.parametrize("nt", [F64, F32], ids=["double", "float_levels"])
@pytest.mark.parametrize("dim,p,n_ref", [(2, 2, 5), (3, 2, 4)])
def test_one_vcycle_value_for_value(dim, p, n_ref, nt):
    ref, R, Z = vcycle_reference(dim, p, n_ref)
    V = GpuVcycle(dim, p, n_ref, nt, ref.lmax)
    assert V.nl == ref.n_levels and any(len(E) for E in ref.edge)
    errs = []
    for k in range(R.shape[1]):
        z = V.apply(R[:, k])
        assert np.isfinite(z).all()
        errs.append(rel(z, Z[:, k]))
    print(f"V-cycle adaptive_mg({dim}, {p}, {n_ref}) {NTNAME[nt]} levels: rel l2 from the numpy reference {errs}, "
          f"coarse CG status {sorted(set(V.coarse_status))}")
    if nt == F64:
        assert set(V.coarse_status) == {1}  # the coarsest level's CG reached 1e-13 |b|
    assert max(errs) <= VCYCLE_TOL[nt], errs
