"""mfgpu_integrator_integrate and the quadrature-point operator mfgpu_qop_* on the GPU against the numpy reference in
tests/qop_reference.py, against the existing paths (Integrator.evaluate, Operator.vmult), and two known answers: a
convection-diffusion solve and Newton's method for nonlinear_reference's problem.

Meshes: the three kinds of test_gpu_poisson.small_mesh at 4^2 / 3^3 cells (cube) and the lowest n_ref (hanging, ball);
the full kind x dim grid at p = 2 and p = 4; p = 1, 3, 5, 6 on the hanging-node meshes, where the masked path and the
ND > 64 loops run.  Tolerance: the suite's double tolerance, relative l2 <= test_gpu.TOL[F64] = 1e-12, unless said
otherwise.  Point-wise arithmetic on the device is done with torch tensors handed to the library by pointer."""
import os
import subprocess

import numpy as np
import pytest

import torch  # before the library is loaded: libmfgpu.so binds to the HIP runtime torch brings (as in bench.py)

import nonlinear_reference as nr
import poisson_reference as pr
import pymfgpu as mf
import qop_reference as qr
from test_gpu import TOL, rel
from test_gpu_evaluate import integrator
from test_gpu_nonlinear import CG_DRIFT
from test_gpu_poisson import dv
from test_qop_host import NEWTON_MESHES, NEWTON_STEPS, PICARD_STEPS, fields

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL64 = TOL[mf.F64]
KINDS = ("cube", "hanging", "ball")
CASES = [(k, d, p) for p in (2, 4) for d in (2, 3) for k in KINDS] + \
        [("hanging", d, p) for p in (1, 3, 5, 6) for d in (2, 3)]
GRID = [c for c in CASES if c[2] in (2, 4)]
ALL = mf.QOP_DIFFUSION_TENSOR | mf.QOP_CONVECTION | mf.QOP_FLUX | mf.QOP_REACTION
BIT = {"diffusion": None, "convection": mf.QOP_CONVECTION, "flux": mf.QOP_FLUX, "reaction": mf.QOP_REACTION}


def mesh_of(kind, dim, p):
    if kind == "cube":
        return mf.Mesh.uniform(dim, p, 4 if dim == 2 else 3)
    if kind == "hanging":
        return mf.Mesh.adaptive(dim, p, 3 if dim == 2 else 4)
    return mf.Mesh.ball(dim, p, 1 if dim == 2 else 0)


class Setup:
    def __init__(self, kind, dim, p):
        self.mesh = mesh_of(kind, dim, p)
        self.cells = pr.Cells(self.mesh)
        self.it = integrator(self.mesh)
        od = self.cells.od
        self.n, self.npts, self.dim = od.n_dofs, od.n_cells * od.nd, dim
        self.tensor, self.scalar = fields(self.cells, 10 * dim + p), fields(self.cells, 10 * dim + p, tensor=False)
        self.x = np.random.default_rng(p).standard_normal(self.n)  # nonzero on the constrained dofs
        self.free = np.ones(self.n, bool)
        self.free[od.constrained] = False
        for a in list(self.tensor.values()) + list(self.scalar.values()) + [self.x]:
            a.setflags(write=False)


_setups = {}


def setup(kind, dim, p):
    if (kind, dim, p) not in _setups:
        _setups[(kind, dim, p)] = Setup(kind, dim, p)
    return _setups[(kind, dim, p)]


def terms_of(coefs, tensor):
    t = 0
    for name in coefs:
        t |= BIT[name] if BIT[name] else (mf.QOP_DIFFUSION_TENSOR if tensor else mf.QOP_DIFFUSION_SCALAR)
    return t


def make_qop(s, coefs, tensor=True):
    q = mf.QpOperator(s.it, terms_of(coefs, tensor))
    q.set_coefficients(**{k: dv(v.reshape(-1)) for k, v in coefs.items()})
    return q


def gpu_apply(q, x, transpose=False):
    src, dst = dv(x), mf.DeviceVector(len(x))
    dst.fill(np.nan)  # every entry is written
    q.vmult(dst, src, transpose=transpose)
    mf.synchronize()
    np.testing.assert_array_equal(src.to_host(), x)  # src untouched
    return dst.to_host()


@pytest.mark.parametrize("kind,dim,p", CASES)
def test_integrate_matches_reference(kind, dim, p):
    s = setup(kind, dim, p)
    od = s.cells.od
    rng = np.random.default_rng(7)
    v, g = rng.standard_normal(s.npts), rng.standard_normal(s.npts * dim)
    dvv, dg = dv(v), dv(g)
    for vals, grads in ((v, None), (None, g), (v, g)):
        dst, dst2 = mf.DeviceVector(s.n), mf.DeviceVector(s.n)
        dst.fill(np.nan)
        s.it.integrate(dst, None if vals is None else dvv, None if grads is None else dg)
        s.it.integrate(dst2, None if vals is None else dvv, None if grads is None else dg)
        got, ref = dst.to_host(), qr.integrate(s.cells, vals, grads)
        err = rel(got, ref)
        print(f"integrate values={vals is not None} gradients={grads is not None}: rel l2 {err:.3e}")
        assert err <= TOL64
        assert np.all(got[od.constrained] == 0.0)
        np.testing.assert_array_equal(dst2.to_host(), got)  # bitwise repeatable
    # <integrate(v, g), u> = sum JxW (v val(u) + g . grad u), u zero on the constrained dofs, evaluate on the GPU
    u = np.where(s.free, s.x, 0.0)
    u[~np.isin(np.arange(s.n), od.loc2glob.reshape(-1))] = 0.0
    val, grad = mf.DeviceVector(s.npts), mf.DeviceVector(s.npts * dim)
    s.it.evaluate(dv(u), val, grad)
    w = od.JxW.astype(np.float64).reshape(-1)
    pv, pg = w * v * val.to_host(), np.repeat(w, dim) * g * grad.to_host()
    lhs, rhs = got @ u, pv.sum() + pg.sum()
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(pv).sum() + np.abs(pg).sum())


@pytest.mark.parametrize("kind,dim,p", CASES)
def test_vmult_term_by_term(kind, dim, p):
    s = setup(kind, dim, p)
    sets = [({"diffusion": s.scalar["diffusion"]}, False), (s.tensor, True)]  # (all five terms with a non-symmetric D)
    sets += [({name: s.tensor[name]}, True) for name in s.tensor]  # each term alone
    for coefs, tensor in sets:
        q = make_qop(s, coefs, tensor)
        for tr in ((False, True) if len(coefs) > 1 else (False,)):
            got, ref = gpu_apply(q, s.x, tr), qr.apply(s.cells, s.x, transpose=tr, **coefs)
            err = rel(got, ref)
            print(f"{'+'.join(coefs)} tensor={tensor} transpose={tr}: rel l2 {err:.3e}")
            assert err <= TOL64
            np.testing.assert_array_equal(got[~s.free], s.x[~s.free])  # identity rows
    # transpose of the single non-symmetric terms
    for coefs in ({"diffusion": s.tensor["diffusion"]}, {"convection": s.tensor["convection"]}):
        got = gpu_apply(make_qop(s, coefs), s.x, True)
        assert rel(got, qr.apply(s.cells, s.x, transpose=True, **coefs)) <= TOL64


@pytest.mark.parametrize("kind,dim,p", GRID + [("hanging", 3, 6)])
def test_vmult_equals_evaluate_arithmetic_integrate(kind, dim, p):
    s = setup(kind, dim, p)
    q = make_qop(s, s.tensor)
    got = gpu_apply(q, s.x)
    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(v.copy()).to(dev) for k, v in s.tensor.items()}
    u = torch.from_numpy(np.where(s.free, s.x, 0.0)).to(dev)
    val = torch.empty(s.npts, dtype=torch.float64, device=dev)
    grad = torch.empty(s.npts * dim, dtype=torch.float64, device=dev)
    s.it.evaluate(u, val, grad)
    gq = grad.view(-1, dim)
    fl = torch.einsum("qkl,ql->qk", t["diffusion"].view(-1, dim, dim), gq) + t["flux"].view(-1, dim) * val[:, None]
    vo = (t["convection"].view(-1, dim) * gq).sum(dim=1) + t["reaction"].view(-1) * val
    dst = torch.empty(s.n, dtype=torch.float64, device=dev)
    s.it.integrate(dst, vo.contiguous(), fl.contiguous())
    torch.cuda.synchronize()
    two_call = dst.cpu().numpy()
    two_call[~s.free] = s.x[~s.free]
    err = rel(got, two_call)
    print(f"fused against evaluate + arithmetic + integrate: rel l2 {err:.3e}")
    assert err <= TOL64


@pytest.mark.parametrize("mass", [False, True])
@pytest.mark.parametrize("kind,dim,p", GRID)
def test_scalar_diffusion_matches_operator_vmult(kind, dim, p, mass):
    s = setup(kind, dim, p)
    mesh = mesh_of(kind, dim, p)
    a = s.cells.od.coefficient.astype(np.float64)
    coefs = {"diffusion": a}
    if mass:
        coefs["reaction"] = s.scalar["reaction"]
        mesh.set_mass_coefficient(s.scalar["reaction"])
    op = mf.Operator(mesh.desc, mesh)
    src, dst = dv(s.x), mf.DeviceVector(s.n)
    op.vmult(dst, src)
    mf.synchronize()
    ref = dst.to_host()
    got = gpu_apply(make_qop(s, coefs, tensor=False), s.x)
    err = rel(got, ref)
    print(f"QpOperator against Operator.vmult (mass={mass}): rel l2 {err:.3e}")
    assert err <= TOL64


@pytest.mark.parametrize("kind,dim,p", [("hanging", 3, 2), ("ball", 2, 4), ("cube", 3, 4)])
def test_vmult_is_repeatable_and_null_keeps_a_term(kind, dim, p):
    s = setup(kind, dim, p)
    q = make_qop(s, s.tensor)
    a, b = gpu_apply(q, s.x), gpu_apply(q, s.x)
    np.testing.assert_array_equal(a, b)
    # dst == src is allowed: the same bits in place
    v = dv(s.x)
    q.vmult(v, v)
    np.testing.assert_array_equal(v.to_host(), a)
    # replace the reaction only: the other three terms keep their values
    c2 = 2.0 + s.tensor["reaction"]
    q.set_coefficients(reaction=dv(c2.reshape(-1)))
    ref = qr.apply(s.cells, s.x, **dict(s.tensor, reaction=c2))
    assert rel(gpu_apply(q, s.x), ref) <= TOL64
    # and back: bitwise the first result
    q.set_coefficients(reaction=dv(s.tensor["reaction"].reshape(-1)))
    np.testing.assert_array_equal(gpu_apply(q, s.x), a)


@pytest.mark.parametrize("kind,dim,p", CASES)
def test_inverse_diagonal_matches_reference(kind, dim, p):
    s = setup(kind, dim, p)
    coefs = dict(s.tensor)
    q = make_qop(s, coefs)
    d = mf.DeviceVector(s.n)
    d.fill(np.nan)
    q.inverse_diagonal(d)
    mf.synchronize()
    got, ref = d.to_host(), qr.inverse_diagonal(s.cells, **coefs)
    err = rel(got, ref)
    print(f"inverse diagonal: rel l2 {err:.3e}")
    assert err <= TOL64
    assert np.all(got[~s.free] == 1.0)


def test_inverse_diagonal_matches_unit_vectors():
    s = setup("hanging", 2, 2)
    q = make_qop(s, s.tensor)
    d = mf.DeviceVector(s.n)
    q.inverse_diagonal(d)
    got = d.to_host()
    referenced = np.isin(np.arange(s.n), s.cells.od.loc2glob.reshape(-1))
    assert (~referenced).any()
    diag = np.ones(s.n)
    for i in np.nonzero(s.free & referenced)[0]:
        e = np.zeros(s.n)
        e[i] = 1.0
        diag[i] = gpu_apply(q, e)[i]
    assert rel(got, 1.0 / diag) <= TOL64
    assert np.all(got[~referenced] == 1.0)


@pytest.mark.parametrize("kind,dim", [("cube", 2), ("cube", 3), ("ball", 2), ("ball", 3)])
def test_memory_consumption_is_the_documented_bytes_per_point(kind, dim):
    s = setup(kind, dim, 2)
    general = kind == "ball"
    assert bool(s.mesh.desc.flags & mf.UNIFORM_J0) == (not general)
    sets = {mf.QOP_DIFFUSION_SCALAR | mf.QOP_REACTION: (8 * dim * dim if general else 8) + 8,
            ALL: 8 * (dim * dim + 2 * dim + 1),
            mf.QOP_CONVECTION | mf.QOP_REACTION: 8 * dim + 8}
    for terms, per_point in sets.items():
        assert mf.QpOperator(s.it, terms).memory_consumption() == per_point * s.npts


def test_error_cases():
    s = setup("cube", 2, 2)
    plain = integrator(s.mesh, updatable=False)
    n, npts = s.n, s.npts
    v, g, dst = dv(np.ones(npts)), dv(np.ones(npts * 2)), mf.DeviceVector(n)
    dst.fill(np.nan)
    # integrate
    with pytest.raises(mf.MfgpuError, match="error -1.*both NULL"):
        s.it.integrate(dst)
    with pytest.raises(mf.MfgpuError, match="error -1.*MFGPU_UPDATABLE_COEFFICIENTS"):
        plain.integrate(dst, v, g)
    with pytest.raises(mf.MfgpuError, match="error -1.*MFGPU_UPDATABLE_COEFFICIENTS"):
        plain.integrate(dst, gradients=g)
    mf.synchronize()
    assert np.all(np.isnan(dst.to_host()))  # a refused call writes nothing
    plain.integrate(dst, v)  # values work on every integrator
    assert rel(dst.to_host(), qr.integrate(s.cells, np.ones(npts))) <= TOL64
    # create
    for terms in (0, 1 << 5, mf.QOP_DIFFUSION_SCALAR | mf.QOP_DIFFUSION_TENSOR, mf.QOP_REACTION | (1 << 9)):
        with pytest.raises(mf.MfgpuError, match="error -1"):
            mf.QpOperator(s.it, terms)
    for terms in (mf.QOP_DIFFUSION_SCALAR, mf.QOP_DIFFUSION_TENSOR, mf.QOP_CONVECTION, mf.QOP_FLUX,
                  mf.QOP_FLUX | mf.QOP_REACTION):
        with pytest.raises(mf.MfgpuError, match="error -1.*MFGPU_UPDATABLE_COEFFICIENTS"):
            mf.QpOperator(plain, terms)
    # a reaction-only operator works on any integrator
    c = s.scalar["reaction"]
    q = mf.QpOperator(plain, mf.QOP_REACTION)
    q.set_coefficients(reaction=dv(c.reshape(-1)))
    assert rel(gpu_apply(q, s.x), qr.apply(s.cells, s.x, reaction=c)) <= TOL64
    # set_coefficients / vmult
    q = mf.QpOperator(s.it, mf.QOP_DIFFUSION_SCALAR | mf.QOP_REACTION)
    src = dv(s.x)
    with pytest.raises(mf.MfgpuError, match="error -1"):
        q.vmult(dst, src)  # nothing set
    with pytest.raises(mf.MfgpuError, match="error -1"):
        q.set_coefficients(flux=g)  # not in terms
    with pytest.raises(mf.MfgpuError, match="error -1"):
        q.set_coefficients()
    q.set_coefficients(diffusion=v)
    with pytest.raises(mf.MfgpuError, match="error -1"):
        q.vmult(dst, src)  # reaction never set
    with pytest.raises(mf.MfgpuError, match="error -1"):
        q.inverse_diagonal(dst)
    q.set_coefficients(reaction=v)
    q.vmult(dst, src)
    assert mf.lib().mfgpu_qop_vmult(q._h, dst.ptr, src.ptr, 2, None) == mf.EINVAL  # unknown flag
    # MFGPU_F32: no integrator, so no operator
    m32 = mf.Mesh.uniform(2, 2, 2, number_type=mf.F32)
    with pytest.raises(mf.MfgpuError, match="error -4"):
        mf.Integrator(m32.desc, m32)


# ---- known answers


def bicgstab(apply, b, dinv, rtol=1e-12, max_it=20000):
    """qop_reference.bicgstab over DeviceVector operations: right-preconditioned, zero start, until |r| <= rtol |b|"""
    n = b.n
    x, r, r0, p, v, y, s, z, t = (mf.DeviceVector(n) for _ in range(9))
    for w in (x, p, v):
        w.fill(0.0)
    r.equ(1.0, b)
    r0.equ(1.0, b)
    tol = rtol * b.l2_norm()
    rho = alpha = omega = 1.0
    for it in range(1, max_it + 1):
        rho_new = r0.dot(r)
        beta = (rho_new / rho) * (alpha / omega)
        rho = rho_new
        p.add(-omega, v)
        p.sadd(beta, 1.0, r)
        y.equ(1.0, p)
        y.scale(dinv)
        apply(v, y)
        alpha = rho / r0.dot(v)
        s.equ(1.0, r)
        s.add(-alpha, v)
        if s.l2_norm() <= tol:
            x.add(alpha, y)
            return x, it
        z.equ(1.0, s)
        z.scale(dinv)
        apply(t, z)
        omega = t.dot(s) / t.dot(t)
        x.add(alpha, y)
        x.add(omega, z)
        r.equ(1.0, s)
        r.add(-omega, t)
        if r.l2_norm() <= tol:
            return x, it
    raise AssertionError("BiCGStab did not converge")


BETA = {2: np.array([1.5, -0.75]), 3: np.array([1.5, -0.75, 0.5])}


def convection_diffusion_error(mesh):
    """-lap u + beta . grad u = f with u = Solution<dim>: the lift by integrate on the evaluated boundary field, BiCGStab
    with the inverse diagonal, L2 error"""
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
    b, dinv = mf.DeviceVector(N), mf.DeviceVector(N)
    it.integrate(b, dv(f - g_h @ BETA[dim]), dv(-g_h.reshape(-1)))  # int phi_i (f - beta . grad u_b) - grad phi_i . grad u_b
    q.inverse_diagonal(dinv)
    x, its = bicgstab(lambda dst, src: q.vmult(dst, src), b, dinv)
    x.add(1.0, ub)
    return it.l2_error(x), its


@pytest.mark.parametrize("dim,p", [(2, 2), (3, 2)])
def test_convection_diffusion_known_answer(dim, p):
    errs = []
    for level in range(3):
        err, its = convection_diffusion_error(pr.family("cube", dim, p, level))
        print(f"{dim}D p={p} level {level}: L2 error {err:.4e}, {its} BiCGStab iterations")
        errs.append(err)
    assert pr.orders(errs)[-1] >= p + 0.7, errs  # the order test_gpu_poisson asserts for the cube family


def gpu_newton(mesh, tol=1e-10, max_steps=50):
    """qop_reference.newton on the GPU: residual by integrate, Jacobian a QpOperator with scalar diffusion 1 + u^2 and
    flux 2 u grad u formed on the device, BiCGStab with the inverse diagonal to 1e-12 |R|.  Only norms and dot products
    come back to the host."""
    dim = int(mesh.desc.dim)
    it = integrator(mesh)
    N, npts = mesh.n_dofs, mesh.n_cells * mesh.nd
    dev = torch.device("cuda", 0)
    con = mesh.arrays()["constrained_dofs"]
    u_h = np.zeros(N)
    u_h[con] = pr.solution(mesh.dof_coords()[con])
    u = dv(u_h)
    mf_f = torch.from_numpy(-nr.load(mesh.arrays()["quadrature_points"].astype(np.float64)).reshape(-1)).to(dev)
    val = torch.empty(npts, dtype=torch.float64, device=dev)
    grad = torch.empty(npts * dim, dtype=torch.float64, device=dev)
    q = mf.QpOperator(it, mf.QOP_DIFFUSION_SCALAR | mf.QOP_FLUX)
    R, dinv = mf.DeviceVector(N), mf.DeviceVector(N)
    hist = []
    for _ in range(max_steps):
        it.evaluate(u, val, grad)
        a = 1.0 + val * val
        it.integrate(R, mf_f, (a[:, None] * grad.view(-1, dim)).contiguous())
        q.set_coefficients(diffusion=a, flux=(2.0 * val[:, None] * grad.view(-1, dim)).contiguous())
        q.inverse_diagonal(dinv)
        R.mul(-1.0)
        d, _ = bicgstab(lambda dst, src: q.vmult(dst, src), R, dinv)
        u.add(1.0, d)
        hist.append(d.l2_norm() / u.l2_norm())
        if hist[-1] <= tol:
            break
    return u.to_host(), hist


@pytest.mark.parametrize("dim,p,n", NEWTON_MESHES)
def test_newton_matches_reference(dim, p, n):
    """The reference's step count, and its final iterate within the tolerance of GPU Picard against the reference
    (test_gpu_nonlinear: 10 x CG_DRIFT).  Newton's limit does not depend on the linear solver: the reference with
    BiCGStab to 1e-12 |R| in place of the direct solve moves by 1.7e-16 (2D p=2 n=8), 1.9e-16 (2D p=4 n=8), 8.5e-17 (3D
    p=2 n=4), measured on the CPU, so the two 2D meshes share the 2D figure."""
    mesh = mf.Mesh.uniform(dim, p, n)
    ref, ref_hist = qr.newton(pr.Cells(mesh))
    got, hist = gpu_newton(mesh)
    allowed = 10 * CG_DRIFT[(dim, 2, n)]
    err = rel(got, ref)
    print(f"{dim}D p={p} n={n}: {len(hist)} Newton steps (reference {len(ref_hist)}, Picard {PICARD_STEPS[(dim, p, n)]}), "
          f"GPU vs reference {err:.3e} (allowed {allowed:.3e}); update norms {hist}")
    assert len(hist) == len(ref_hist) == NEWTON_STEPS[(dim, p, n)]
    assert err <= allowed


def _driver(exe):
    out = subprocess.run([os.path.join(ROOT, "dealii-cuda_amd", "host", "bin", exe), "-q", "0", "0"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert len(rows) == 1 and len(rows[0]) == 7, out.stdout
    return rows[0]


@pytest.mark.parametrize("dim,p,n", [(2, 2, 8), (3, 2, 4)])
def test_newton_driver_against_nonlinear_driver(dim, p, n):
    """First cycle of newton-* and nonlinear-* (the meshes of NEWTON_MESHES).  Both stop at a relative update of 1e-10;
    Picard contracts by at least 5x per step, so its iterate is within 1.25e-10 |u| of the discrete solution and Newton's
    far closer.  The L2 errors (1.4e-2 in 2D, 9.1e-2 in 3D, |u|_L2 below 1) then differ by at most 1.25e-10 / 1.4e-2 =
    9e-9 relative, plus 5e-9 for the 8 printed digits: 2e-8 allowed."""
    newton, picard = _driver(f"newton-{dim}d-p{p}"), _driver(f"nonlinear-{dim}d-p{p}")
    print(newton, picard)
    assert [int(v) for v in newton[:3]] == [int(v) for v in picard[:3]] == [dim, p, (p * n + 1) ** dim]
    assert int(newton[3]) == NEWTON_STEPS[(dim, p, n)] < int(picard[3])
    assert int(newton[3]) <= int(newton[4]) < 10000 * int(newton[3])
    e_newton, e_picard = float(newton[6]), float(picard[6])
    assert abs(e_newton - e_picard) <= 2e-8 * e_picard, (e_newton, e_picard)
