"""The vector-valued quadrature-point operator mfgpu_vqop_* on the GPU against the numpy reference in
tests/vqop_reference.py, against the scalar path (QpOperator) and a known answer solved by the device BiCGStab.

Meshes: those of test_gpu_qop -- cube 4^2 / 3^3 cells, Mesh.adaptive(dim, p, 3 | 4), Mesh.ball(dim, p, 1 | 0); the
kind x dim grid at p = 2 and p = 4, and p = 1, 3, 5, 6 on the hanging-node meshes, where the masked path and the ND > 64
loops run.  Tolerance: the suite's double tolerance, relative l2 <= test_gpu.TOL[F64] = 1e-12, unless said otherwise.
Fields are in blocks: u[a * n_dofs + i]."""
import os
import subprocess

import numpy as np
import pytest

import torch  # noqa: F401  before the library is loaded: libmfgpu.so binds to the HIP runtime torch brings

import poisson_reference as pr
import pymfgpu as mf
import qop_reference as qr
import vqop_reference as vr
from test_gpu import TOL, rel
from test_gpu_evaluate import integrator
from test_gpu_poisson import dv
from test_gpu_qop import CASES, GRID, mesh_of
from test_vqop_host import TERM_SETS, pick, rigid_body_modes, vfields
from util import desc_from_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL64 = TOL[mf.F64]
BIT = {"lam": mf.VQOP_ISOTROPIC, "mu": mf.VQOP_ISOTROPIC, "tensor": mf.VQOP_TENSOR4, "mass": mf.VQOP_MASS}


class Setup:
    """mesh, reference cells, integrator, seeded coefficients and a source that is nonzero on constrained entries.
    dirichlet=False: the description rebuilt through make_desc without Dirichlet dofs (every dof free)"""

    def __init__(self, kind, dim, p, dirichlet=True):
        self.mesh = mesh_of(kind, dim, p)
        if dirichlet:
            self.cells = pr.Cells(self.mesh)
            self.it = integrator(self.mesh)
        else:
            self.mesh.desc.n_constrained = 0
            self.cells = pr.Cells(self.mesh)
            desc, keep = desc_from_oracle(self.cells.od, quadrature_points=self.cells.qpts)
            desc.flags |= mf.UPDATABLE_COEFFICIENTS
            self.it = mf.Integrator(desc, keep)
        od = self.cells.od
        self.dim, self.n_dofs, self.n, self.npts = dim, od.n_dofs, dim * od.n_dofs, od.n_cells * od.nd
        self.f = vfields(self.cells, 10 * dim + p)
        self.x = np.random.default_rng(p).standard_normal(self.n)
        self.con = vr.constrained_flags(self.cells)
        for a in list(self.f.values()) + [self.x, self.con]:
            a.setflags(write=False)
        self._ref = {}

    def ref(self, names, constrained=None):
        """the reference apply to self.x, computed once per term set"""
        key = (names, None if constrained is None else tuple(constrained))
        if key not in self._ref:
            self._ref[key] = vr.apply(self.cells, self.x, constrained=constrained, **pick(self.f, *names))
            self._ref[key].setflags(write=False)
        return self._ref[key]


_setups = {}


def setup(kind, dim, p, dirichlet=True):
    key = (kind, dim, p, dirichlet)
    if key not in _setups:
        _setups[key] = Setup(*key)
    return _setups[key]


def terms_of(names):
    t = 0
    for k in names:
        t |= BIT[k]
    return t


def make_vqop(s, names, constrained=None, coefs=None):
    q = mf.VectorQpOperator(s.it, terms_of(names), constrained)
    q.set_coefficients(**{k: dv(np.asarray((coefs or s.f)[k]).reshape(-1)) for k in names})
    return q


def gpu_apply(q, x):
    src, dst = dv(x), mf.DeviceVector(len(x))
    dst.fill(np.nan)  # every entry is written
    q.vmult(dst, src)
    mf.synchronize()
    np.testing.assert_array_equal(src.to_host(), x)  # src untouched
    return dst.to_host()


# ---- 1. vmult against the reference


@pytest.mark.parametrize("kind,dim,p", CASES)
def test_vmult_matches_reference(kind, dim, p):
    s = setup(kind, dim, p)
    for names in TERM_SETS:
        q = make_vqop(s, names)
        got, ref = gpu_apply(q, s.x), s.ref(names)
        err = rel(got, ref)
        print(f"{'+'.join(names)}: rel l2 {err:.3e}")
        assert err <= TOL64
        np.testing.assert_array_equal(got[s.con], s.x[s.con])  # identity rows
        np.testing.assert_array_equal(gpu_apply(q, s.x), got)  # bitwise repeatable
        v = dv(s.x)
        q.vmult(v, v)  # dst == src: the same bits in place
        np.testing.assert_array_equal(v.to_host(), got)


# ---- 2. the two folds of the isotropic law


@pytest.mark.parametrize("kind,dim,p", GRID)
def test_isotropic_equals_tensor4_of_the_isotropic_tensor(kind, dim, p):
    s = setup(kind, dim, p)
    iso = gpu_apply(make_vqop(s, ("lam", "mu")), s.x)
    C4 = vr.isotropic_tensor(s.f["lam"], s.f["mu"], dim)
    ten = gpu_apply(make_vqop(s, ("tensor",), coefs={"tensor": C4}), s.x)
    err = rel(ten, iso)
    print(f"TENSOR4(isotropic_tensor) against ISOTROPIC: rel l2 {err:.3e}")
    assert err <= TOL64


# ---- 3. the existing scalar path


@pytest.mark.parametrize("kind,dim,p", GRID)
def test_decoupled_tensor_equals_scalar_qop_per_component(kind, dim, p):
    s = setup(kind, dim, p)
    a = s.f["lam"]
    d = np.eye(dim)
    C4 = a[..., None, None, None, None] * np.einsum("ab,kl->akbl", d, d)
    got = gpu_apply(make_vqop(s, ("tensor",), coefs={"tensor": C4}), s.x).reshape(dim, s.n_dofs)
    sq = mf.QpOperator(s.it, mf.QOP_DIFFUSION_SCALAR)
    sq.set_coefficients(diffusion=dv(a.reshape(-1)))
    for c in range(dim):
        src, dst = dv(s.x.reshape(dim, s.n_dofs)[c]), mf.DeviceVector(s.n_dofs)
        sq.vmult(dst, src)
        mf.synchronize()
        err = rel(got[c], dst.to_host())
        print(f"component {c} against QpOperator(DIFFUSION_SCALAR): rel l2 {err:.3e}")
        assert err <= TOL64


# ---- 4. rigid-body modes


@pytest.mark.parametrize("kind,dim,p", [c for c in GRID if c[0] != "hanging"])
def test_rigid_body_modes(kind, dim, p):
    s = setup(kind, dim, p, dirichlet=False)
    assert not s.con.any()
    q = make_vqop(s, ("lam", "mu"))
    scale = np.linalg.norm(gpu_apply(q, s.x)) / np.linalg.norm(s.x)
    modes = rigid_body_modes(s.cells)
    assert len(modes) == dim * (dim + 1) // 2
    for r in modes:
        res = np.linalg.norm(gpu_apply(q, r))
        print(f"|A r| = {res:.3e}, allowed {1e-12 * scale * np.linalg.norm(r):.3e}")
        assert res <= 1e-12 * scale * np.linalg.norm(r)


# ---- 5. symmetry


@pytest.mark.parametrize("kind,dim,p", GRID)
def test_isotropic_plus_mass_is_symmetric(kind, dim, p):
    s = setup(kind, dim, p)
    q = make_vqop(s, ("lam", "mu", "mass"))
    x = np.where(s.con, 0.0, s.x)
    y = np.where(s.con, 0.0, np.random.default_rng(77).standard_normal(s.n))
    Ax, Ay = gpu_apply(q, x), gpu_apply(q, y)
    assert abs(y @ Ax - x @ Ay) <= 1e-12 * (np.abs(y) @ np.abs(Ax))


# ---- 6. per-component constraints


@pytest.mark.parametrize("dim", [2, 3])
def test_per_component_constraints(dim):
    s = setup("cube", dim, 2, dirichlet=False)
    xc = s.cells.dof_coords[:, 0]
    lo, hi = np.isclose(xc, xc.min()), np.isclose(xc, xc.max())
    assert lo.any() and hi.any()
    con = np.zeros((dim, s.n_dofs), bool)
    con[0] = lo  # component 0 fixed on x = lo (a sliding face), every component on x = hi, the rest free
    con[:, hi] = True
    con = con.reshape(-1)
    lst = np.nonzero(con)[0]
    names = ("lam", "mu", "mass")
    q = make_vqop(s, names, constrained=lst)
    got, ref = gpu_apply(q, s.x), s.ref(names, constrained=lst)
    assert rel(got, ref) <= TOL64
    np.testing.assert_array_equal(got[con], s.x[con])
    d = mf.DeviceVector(s.n)
    d.fill(np.nan)
    q.inverse_diagonal(d)
    dh = d.to_host()
    assert rel(dh, vr.inverse_diagonal(s.cells, constrained=lst, **pick(s.f, *names))) <= TOL64
    assert np.all(dh[con] == 1.0)
    v = dv(s.x)
    q.set_constrained_values(v, -2.5)
    np.testing.assert_array_equal(v.to_host(), np.where(con, -2.5, s.x))
    # the default list is the description's (here empty): nothing is set
    v = dv(s.x)
    make_vqop(s, ("mass",)).set_constrained_values(v, -2.5)
    np.testing.assert_array_equal(v.to_host(), s.x)


# ---- 7. inverse diagonal


@pytest.mark.parametrize("kind,dim,p", CASES)
def test_inverse_diagonal_matches_reference(kind, dim, p):
    """The tensor here is tensor_pos, whose diagonal sums have positive terms only.  1 / A_jj carries the rounding of A_jj
    times sum |terms| / |sum terms|, which the indefinite random tensor of the vmult tests does not bound: on hanging 3D
    p = 6 it gave 7.2e-12 against 4.2e-15 for lam + mu + mass on the same mesh (measured on the MI355X)."""
    s = setup(kind, dim, p)
    for names in (("lam", "mu", "mass"), ("tensor",)):
        coefs = pick(s.f, *names) if names != ("tensor",) else {"tensor": s.f["tensor_pos"]}
        q = make_vqop(s, names, coefs=coefs)
        d = mf.DeviceVector(s.n)
        d.fill(np.nan)
        q.inverse_diagonal(d)
        mf.synchronize()
        got, ref = d.to_host(), vr.inverse_diagonal(s.cells, **coefs)
        err = rel(got, ref)
        print(f"inverse diagonal {'+'.join(names)}: rel l2 {err:.3e}")
        assert err <= TOL64
        assert np.all(got[s.con] == 1.0)


def test_inverse_diagonal_matches_unit_vectors():
    s = setup("hanging", 2, 2)
    q = make_vqop(s, ("tensor", "mass"))
    d = mf.DeviceVector(s.n)
    q.inverse_diagonal(d)
    got = d.to_host()
    referenced = np.tile(np.isin(np.arange(s.n_dofs), s.cells.od.loc2glob.reshape(-1)), s.dim)
    assert (~referenced).any()
    diag = np.ones(s.n)
    for i in np.nonzero(~s.con & referenced)[0]:
        e = np.zeros(s.n)
        e[i] = 1.0
        diag[i] = gpu_apply(q, e)[i]
    assert rel(got, 1.0 / diag) <= TOL64
    assert np.all(got[~referenced] == 1.0)


# ---- 8. a partial update keeps the other terms


@pytest.mark.parametrize("kind,dim,p", [("hanging", 3, 2), ("ball", 2, 4), ("cube", 3, 4)])
def test_setting_the_mass_alone_keeps_lambda_and_mu(kind, dim, p):
    s = setup(kind, dim, p)
    names = ("lam", "mu", "mass")
    q = make_vqop(s, names)
    first = gpu_apply(q, s.x)
    m2 = 2.0 + s.f["mass"]
    q.set_coefficients(mass=dv(m2.reshape(-1)))
    ref = vr.apply(s.cells, s.x, lam=s.f["lam"], mu=s.f["mu"], mass=m2)
    assert rel(gpu_apply(q, s.x), ref) <= TOL64
    q.set_coefficients(mass=dv(s.f["mass"].reshape(-1)))
    np.testing.assert_array_equal(gpu_apply(q, s.x), first)  # and back: bitwise the first result


# ---- 9. memory


@pytest.mark.parametrize("kind,dim", [("cube", 2), ("cube", 3), ("ball", 2), ("ball", 3)])
def test_memory_consumption_is_the_documented_bytes_per_point(kind, dim):
    s = setup(kind, dim, 2)
    assert bool(s.mesh.desc.flags & mf.UNIFORM_J0) == (kind == "cube")
    sets = {mf.VQOP_ISOTROPIC: 16, mf.VQOP_TENSOR4: 8 * dim ** 4, mf.VQOP_MASS: 8, mf.VQOP_ISOTROPIC | mf.VQOP_MASS: 24,
            mf.VQOP_TENSOR4 | mf.VQOP_MASS: 8 * dim ** 4 + 8}
    for terms, per_point in sets.items():
        assert mf.VectorQpOperator(s.it, terms).memory_consumption() == per_point * s.npts + dim * s.n_dofs


# ---- 10. errors


def test_error_cases():
    s = setup("cube", 2, 2)
    plain = integrator(s.mesh, updatable=False)
    n, npts = s.n, s.npts
    one, c4 = dv(np.ones(npts)), dv(np.ones(npts * 16))
    src, dst = dv(s.x), mf.DeviceVector(n)
    dst.fill(np.nan)
    # create: terms
    for terms in (0, 1 << 3, mf.VQOP_ISOTROPIC | mf.VQOP_TENSOR4, mf.VQOP_ISOTROPIC | mf.VQOP_TENSOR4 | mf.VQOP_MASS,
                  mf.VQOP_MASS | (1 << 9)):
        with pytest.raises(mf.MfgpuError, match="error -1"):
            mf.VectorQpOperator(s.it, terms)
    for terms in (mf.VQOP_ISOTROPIC, mf.VQOP_TENSOR4, mf.VQOP_ISOTROPIC | mf.VQOP_MASS):
        with pytest.raises(mf.MfgpuError, match="error -1.*MFGPU_UPDATABLE_COEFFICIENTS"):
            mf.VectorQpOperator(plain, terms)
    # create: the list
    base = np.nonzero(s.con)[0]
    for bad in (base[::-1], np.concatenate([base[:1], base]), np.concatenate([base, [n]]), base[1:], base[:-1]):
        with pytest.raises(mf.MfgpuError, match="error -1"):  # descending, repeated, out of range, not covering
            mf.VectorQpOperator(s.it, mf.VQOP_MASS, bad)
    assert rel(gpu_apply(make_vqop(s, ("mass",), constrained=base), s.x), s.ref(("mass",))) <= TOL64
    # a mass-only operator works on any integrator
    q = mf.VectorQpOperator(plain, mf.VQOP_MASS)
    q.set_coefficients(mass=dv(s.f["mass"].reshape(-1)))
    assert rel(gpu_apply(q, s.x), s.ref(("mass",))) <= TOL64
    # set_coefficients / vmult / diagonal
    q = mf.VectorQpOperator(s.it, mf.VQOP_ISOTROPIC | mf.VQOP_MASS)
    with pytest.raises(mf.MfgpuError, match="error -1"):
        q.vmult(dst, src)  # nothing set
    with pytest.raises(mf.MfgpuError, match="error -1"):
        q.set_coefficients(tensor=c4)  # not in terms
    with pytest.raises(mf.MfgpuError, match="error -1"):
        q.set_coefficients()
    with pytest.raises(mf.MfgpuError, match="error -1"):
        q.set_coefficients(lam=one)  # without mu
    with pytest.raises(mf.MfgpuError, match="error -1"):
        q.set_coefficients(mu=one, mass=one)  # without lambda: nothing is folded, the mass stays unset
    q.set_coefficients(lam=one, mu=one)
    with pytest.raises(mf.MfgpuError, match="error -1"):
        q.vmult(dst, src)  # mass never set
    with pytest.raises(mf.MfgpuError, match="error -1"):
        q.inverse_diagonal(dst)
    mf.synchronize()
    assert np.all(np.isnan(dst.to_host()))  # a refused call writes nothing
    q.set_coefficients(mass=one)
    q.vmult(dst, src)
    assert np.all(np.isfinite(dst.to_host()))
    qt = mf.VectorQpOperator(s.it, mf.VQOP_TENSOR4)
    with pytest.raises(mf.MfgpuError, match="error -1"):
        qt.set_coefficients(lam=one, mu=one)
    # BiCGStab: the solver's length is dim * n_dofs, its type double
    L = mf.lib()
    for length, nt in ((s.n_dofs, mf.F64), (n, mf.F32)):
        b = mf.BiCGStab(lambda d, x, st: None, n=length, number_type=nt)
        assert L.mfgpu_bicgstab_set_operator_vqop(b._h, q._h) == mf.EINVAL
    assert mf.BiCGStab(q).n == n


# ---- 11. known answer

# Relative l2 distance of qop_reference.bicgstab (Jacobi, 1e-12 |b|) on the assembled matrix from x*, and its iteration
# count, measured on the CPU (isotropic + mass, seeds as below): the summation-order drift the GPU is allowed 10x of.
BICGSTAB_DRIFT = {(2, 2, 8): (5.062e-11, 72), (3, 2, 4): (1.078e-11, 39)}


def known_answer(dim, p, n):
    mesh = mf.Mesh.uniform(dim, p, n)
    cells = pr.Cells(mesh)
    f = pick(vfields(cells, 40 + dim), "lam", "mu", "mass")
    con = vr.constrained_flags(cells)
    xs = np.where(con, 0.0, np.random.default_rng(41).standard_normal(con.size))
    A = vr.assemble(cells, **f)
    return mesh, cells, f, xs, A, A @ xs


@pytest.mark.parametrize("dim,p,n", list(BICGSTAB_DRIFT))
def test_known_answer_by_device_bicgstab(dim, p, n):
    mesh, cells, f, xs, A, b = known_answer(dim, p, n)
    ref, ref_its = qr.bicgstab(lambda v: A @ v, b, vr.inverse_diagonal(cells, **f))
    drift, _ = BICGSTAB_DRIFT[(dim, p, n)]
    q = mf.VectorQpOperator(integrator(mesh), mf.VQOP_ISOTROPIC | mf.VQOP_MASS)
    q.set_coefficients(**{k: dv(v.reshape(-1)) for k, v in f.items()})
    dinv, x, bd = mf.DeviceVector(len(b)), mf.DeviceVector(len(b)), dv(b)
    q.inverse_diagonal(dinv)
    solver = mf.BiCGStab(q, mf.CG_JACOBI, dinv)
    info = solver.solve(x, bd, 1e-12 * np.linalg.norm(b), 10000)
    err = rel(x.to_host(), xs)
    print(f"{dim}D p={p} n={n}: {info.iterations} iterations (numpy loop {ref_its}), |x - x*| / |x*| = {err:.3e} "
          f"(numpy loop {rel(ref, xs):.3e}, allowed {10 * drift:.3e})")
    assert info.status == 1
    assert abs(int(info.iterations) - ref_its) <= 2
    assert err <= 10 * drift


# ---- 12. the driver


@pytest.mark.parametrize("dim,p", [(2, 2), (2, 4), (3, 2), (3, 4)])
def test_elasticity_driver_errors_decrease(dim, p):
    """the two lowest refinements of elasticity-*: one line per cycle, every component's L2 error falls.  The observed
    orders are recorded in profiles/r25_notes.md, not asserted."""
    out = subprocess.run([os.path.join(ROOT, "dealii-cuda_amd", "host", "bin", f"elasticity-{dim}d-p{p}"), "-q", "0", "1"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    print(out.stdout)
    assert len(rows) == 2 and all(len(r) == 5 + dim for r in rows), out.stdout
    assert [int(r[0]) for r in rows] == [dim, dim] and [int(r[1]) for r in rows] == [p, p]
    assert int(rows[0][2]) < int(rows[1][2])
    for a in range(dim):
        coarse, fine = float(rows[0][5 + a]), float(rows[1][5 + a])
        assert 0.0 < fine < coarse, (a, coarse, fine)
