"""GPU: adaptive refinement.

mfgpu_integrator_recovery_indicator against the numpy restatement of tests/amr_reference.py (written from the definition
in include/mfgpu.h), by a known answer that does not go through it, by where it localises a kink, bitwise repeatable,
captured in a graph, inside red zones, and its refusals; then the loop solve -> estimate -> mark -> refine -> transfer ->
solve through pymfgpu, and the poisson-amr driver against that loop.

Bounds.  Parity: |got - want| <= 1e-12 max_K want, the project's double parity bound.  Known answer: u the interpolant of
a polynomial of degree <= p per variable on an affine mesh, so that G = grad u_h exactly and
sum eta_K^2 <= (1e4 * 2.2e-16)^2 sum_K int |grad u_h|^2; the factor 1e4 covers the amplification by the inverse table
and the derivative matrices, and the numpy reference stays 100x inside it at p = 6
(tests/test_amr_host.py::test_the_reference_vanishes_on_polynomials_100x_inside_the_gpu_bound measures 2e-16 .. 8e-16).
Localisation: threshold 1e-3 max; the reference puts 5e-29 max outside the three columns
(tests/test_amr_host.py::test_the_reference_localises_a_kink).  Loop: the GPU solves stop at a residual of 1e-12 |b| and
the CPU model solves directly; with a condition number below 1e4 on these meshes the L2 error and eta agree to 1e-8."""
import functools
import os
import subprocess

import numpy as np
import pytest

try:  # before the library is loaded, as in the other graph tests: both then share one HIP runtime
    import torch
except ImportError:
    torch = None

import amr_reference as ar
import gc_reference as gr
import poisson_reference as pr
import pymfgpu as mf
from oracle import mf_oracle as o
from redzone import Zoned
from test_amr_host import KNOWN_ANSWER_FACTOR, known_answer_ratio, polynomial, small_mesh
from test_gpu_evaluate import integrator, nan_vector
from test_gpu_poisson import dv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "dealii-cuda_amd", "host", "bin")

PARITY = [(kind, dim, p) for kind in ("uniform", "leaves", "ball0", "ball1") for dim in (2, 3) for p in (1, 2, 4, 6)] + [
    ("leaves", 2, 3), ("leaves", 2, 5)]


@functools.lru_cache(maxsize=None)
def case(kind, dim, p):
    """(mesh, cells, u, weight, eta, eta with the weight): the reference is computed once per case"""
    mesh = small_mesh(kind, dim, p)
    cells = pr.Cells(mesh)
    rng = np.random.default_rng(100 * dim + 10 * p + len(kind))
    u = rng.standard_normal(mesh.n_dofs)
    unread = np.ones(mesh.n_dofs, bool)
    unread[cells.od.loc2glob.reshape(-1)] = False
    assert (kind == "leaves") == bool(unread.any())
    weight = rng.uniform(0.5, 2.0, (mesh.n_cells, mesh.nd))
    eta = ar.recovery_indicator(cells, np.where(unread, 0.0, u))
    eta_w = ar.recovery_indicator(cells, np.where(unread, 0.0, u), weight)
    u[unread] = np.nan  # the entries of hanging dofs are not read
    for a in (u, weight, eta, eta_w):
        a.setflags(write=False)
    return mesh, cells, u, weight, eta, eta_w


def indicator(it, u, weight=None):
    out = nan_vector(it.n_cells)  # every entry is written
    assert it.recovery_indicator(dv(u), out, None if weight is None else dv(np.asarray(weight).reshape(-1))) is out
    mf.synchronize()
    return out.to_host()


@pytest.mark.parametrize("kind,dim,p", PARITY)
def test_indicator_matches_the_reference(kind, dim, p):
    mesh, cells, u, weight, eta, eta_w = case(kind, dim, p)
    it = integrator(mesh)
    for w, want in ((None, eta), (weight, eta_w)):
        got = indicator(it, u, w)
        err = np.abs(got - want).max() / want.max()
        print(f"{kind} {dim}D p = {p} ({mesh.n_cells} cells){' weighted' if w is not None else ''}: "
              f"max |got - want| / max want = {err:.2e}")
        assert err <= 1e-12
    assert eta.min() > 0 and np.abs(eta_w - eta).max() > 1e-3 * eta.max()  # (the weight matters)


@pytest.mark.parametrize("kind,dim,p", [(kind, dim, p) for kind in ("uniform", "leaves") for dim in (2, 3) for p in (1, 2, 4, 6)])
def test_indicator_vanishes_on_polynomials(kind, dim, p):
    mesh = small_mesh(kind, dim, p)
    it = integrator(mesh)
    u = polynomial(dim, p, 7 * p + dim)(mesh.dof_coords())
    got = indicator(it, u)
    g = nan_vector(mesh.n_cells * mesh.nd * dim)
    it.evaluate(dv(u), gradients=g)
    mf.synchronize()
    r = known_answer_ratio(pr.Cells(mesh), got, g.to_host().reshape(mesh.n_cells, mesh.nd, dim))
    print(f"{kind} {dim}D p = {p}: sqrt(sum eta^2 / sum int |grad u_h|^2) = {r:.2e}, bound {KNOWN_ANSWER_FACTOR * 2.2e-16:.1e}")
    assert (got >= 0).all() and r <= KNOWN_ANSWER_FACTOR * 2.2e-16


def test_indicator_localises_a_kink():
    mesh = mf.Mesh.uniform(2, 2, 8)
    eta = indicator(integrator(mesh), np.abs(mesh.dof_coords()[:, 0] - 0.3))
    x = mesh.arrays()["quadrature_points"][:, :, 0].mean(axis=1)
    col = np.floor((x + 1.0) / 0.25).astype(int)
    kink = int(np.floor(1.3 / 0.25))
    big = eta > 1e-3 * eta.max()
    assert big[col == kink].all() and (np.abs(col[big] - kink) <= 1).all()


@pytest.mark.parametrize("kind,dim,p", [("leaves", 3, 2), ("ball1", 2, 4), ("uniform", 3, 6)])
def test_two_calls_are_bitwise_equal(kind, dim, p):
    mesh, _, u, weight, _, _ = case(kind, dim, p)
    it = integrator(mesh)
    a, b = indicator(it, u, weight), indicator(it, u, weight)
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    c = indicator(integrator(mesh), u, weight)  # and of another object
    np.testing.assert_array_equal(a.view(np.uint64), c.view(np.uint64))


def test_refusals():
    mesh, _, u, _, _, _ = case("leaves", 2, 2)
    out = nan_vector(mesh.n_cells)
    with pytest.raises(mf.MfgpuError, match="error -1.*MFGPU_UPDATABLE_COEFFICIENTS"):
        integrator(mesh, updatable=False).recovery_indicator(dv(u), out)
    it = integrator(mesh)
    L = mf.lib()
    d = dv(u)
    assert L.mfgpu_integrator_recovery_indicator(it._h, None, None, out.ptr, None) == mf.EINVAL
    assert L.mfgpu_integrator_recovery_indicator(it._h, d.ptr, None, None, None) == mf.EINVAL
    assert L.mfgpu_integrator_recovery_indicator(None, d.ptr, None, out.ptr, None) == mf.EINVAL
    mf.synchronize()
    assert np.all(np.isnan(out.to_host()))  # a refused call writes nothing


@pytest.mark.parametrize("kind,dim,p", [("leaves", 3, 2), ("ball1", 2, 4)])
def test_indicator_is_graph_capturable(kind, dim, p):
    if torch is None:
        pytest.skip("torch is not installed")
    assert torch.cuda.is_available()
    mesh, _, u, weight, _, _ = case(kind, dim, p)
    it = integrator(mesh)
    want = indicator(it, u, weight)  # (the first call allocates the scratch: before the capture)
    dev = torch.device("cuda", 0)
    ut = torch.tensor(np.where(np.isnan(u), 0.0, u), device=dev, dtype=torch.float64)
    wt = torch.tensor(weight.reshape(-1), device=dev, dtype=torch.float64)
    out = torch.full((mesh.n_cells,), float("nan"), device=dev, dtype=torch.float64)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        it.recovery_indicator(ut, out, wt, torch.cuda.current_stream().cuda_stream)
    for _ in range(2):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64), want.view(np.uint64))  # no atomics: the same bits


@pytest.mark.parametrize("offset_one", [False, True], ids=["aligned16", "one_off"])
@pytest.mark.parametrize("kind,dim,p", [("leaves", 3, 2), ("ball1", 3, 4), ("uniform", 2, 6)])
def test_indicator_inside_red_zones(kind, dim, p, offset_one):
    mesh, _, u, weight, _, eta_w = case(kind, dim, p)
    it = integrator(mesh)
    zu = Zoned(np.where(np.isnan(u), 0.0, u), mf.F64, offset_one)
    zw = Zoned(weight, mf.F64, offset_one)
    zo = Zoned(mesh.n_cells, mf.F64, offset_one)
    it.recovery_indicator(zu.vec, zo.vec, zw.vec)
    got = zo.result()
    zu.unchanged()
    zw.unchanged()
    assert np.abs(got - eta_w).max() <= 1e-12 * eta_w.max()


# ---- the loop


def lagrange_at(nodes, x):
    """[len(x), len(nodes)] values of the Lagrange basis on `nodes`"""
    return o.lagrange_eval(np.asarray(nodes), np.asarray(x))[0].T


def solve_on(mesh, start=None):
    """the reference's Poisson problem on the mesh through pymfgpu: u = lift + x with A x = rhs(f, lift), CG under the
    global-coarsening V-cycle to 1e-12 |b|; with `start` (a homogeneous field) the CG solves for the correction of it.
    Returns (u, x, iterations, l2 error, eta_K^2, integrator)"""
    cells = pr.Cells(mesh)
    N = mesh.n_dofs
    it = integrator(mesh)
    op = mf.Operator(mesh.desc, mesh)
    lift, b = dv(cells.lift()), mf.DeviceVector(N)
    it.rhs(b, None, lift)
    bnorm = b.l2_norm()
    x = mf.DeviceVector(N)
    x.fill(0.0)
    if start is not None:
        x.equ(1.0, start)
        op.set_constrained_values(x, 0.0)
        t = mf.DeviceVector(N)
        op.vmult(t, x)
        b.add(-1.0, t)  # b - A x~ (0 on the constrained rows: x~ is 0 there)
    cg = mf.CG(op, mf.CG_CALLBACK)
    cg.set_vcycle(mf.VCycle.from_global_coarsening(mesh))
    delta = mf.DeviceVector(N)
    info = cg.solve(delta, b, 1e-12 * bnorm, 200)
    assert info.status == 1
    x.add(1.0, delta)
    u = mf.DeviceVector(N)
    u.equ(1.0, x)
    u.add(1.0, lift)
    l2 = it.l2_error(u)
    eta = it.recovery_indicator(u)
    mf.synchronize()
    return u, x, int(info.iterations), l2, eta.to_host(), it


@functools.lru_cache(maxsize=None)
def python_loop(dim=2, p=2, start_level=2, n_cycles=3, fraction=0.3):
    """[(mesh, l2, eta, iterations)] and the checks of every transfer"""
    mesh = mf.Mesh.from_leaves(dim, p, pr.refined_leaves([[0, 0, 0, 0]], dim, start_level))
    out, start = [], None
    for cycle in range(n_cycles):
        u, x, its, l2, eta, it = solve_on(mesh, start)
        out.append((mesh, l2, float(np.sqrt(eta.sum())), its))
        fine = mesh.refined(mf.mark_fixed_number(eta, fraction))
        assert gr.one_irregular(dim, fine.cell_levels())
        start = mf.DeviceVector(fine.n_dofs)
        start.fill(np.nan)
        mf.Transfer.h_hn_from_meshes(mesh, fine).prolongate(start, x)
        check_transfer(mesh, fine, x.to_host(), start.to_host(), it)
        mesh = fine
    return out


def check_transfer(coarse, fine, xc, xf, it_coarse):
    dim, p = int(coarse.desc.dim), int(coarse.desc.degree)
    parent, child = mf.coarsening_map(coarse, fine)
    ca, fa = coarse.arrays(), fine.arrays()
    cm = ca["constraint_mask"] if ca["constraint_mask"] is not None else np.zeros(coarse.n_cells, np.uint32)
    fm = fa["constraint_mask"] if fa["constraint_mask"] is not None else np.zeros(fine.n_cells, np.uint32)
    cd = np.zeros(coarse.n_dofs, bool)
    cd[ca["constrained_dofs"]] = True
    xc = np.where(cd, 0.0, xc)  # the transfer reads the coarse constrained dofs as 0 (x is 0 there anyway)
    # a cell that did not change carries its values bit for bit (at the positions neither mask constrains)
    n_same = 0
    for f in np.nonzero(child == 0)[0]:
        c = parent[f]
        free = ~(ar.constrained_positions(dim, p, int(cm[c])) | ar.constrained_positions(dim, p, int(fm[f])))
        got, want = xf[fa["loc2glob"][f][free]], xc[ca["loc2glob"][c][free]]
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
        n_same += 1
    assert 0 < n_same < fine.n_cells
    # the prolongated field at the fine quadrature points is the coarse field there
    cells_c = pr.Cells(coarse)
    nodes, xq = o.shape_info(p)[4], o.shape_info(p)[2]
    vals = nan_vector(fine.n_cells * fine.nd)
    integrator(fine).evaluate(dv(np.where(np.isnan(xf), 0.0, xf)), values=vals)
    mf.synchronize()
    got = vals.to_host().reshape(fine.n_cells, fine.nd)
    want = np.zeros_like(got)
    for f in range(fine.n_cells):
        c, k = parent[f], int(child[f]) - 1
        uc = cells_c._hn(c, xc[ca["loc2glob"][c]], False)
        tabs = [lagrange_at(nodes, xq if k < 0 else 0.5 * (((k >> d) & 1) + xq)) for d in range(dim)]
        want[f] = pr._kron_tables(tabs) @ uc
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"transfer {coarse.n_cells} -> {fine.n_cells} cells: {n_same} unchanged cells bit-equal, "
          f"field at the fine quadrature points rel {err:.2e}")
    assert err <= 1e-13


def test_loop_through_pymfgpu():
    cpu = ar.amr_loop(2, 2, 2, 3, 0.3)
    assert cpu[-1][1] < cpu[0][1]  # the CPU model shows the drop
    out = python_loop()
    for (mesh, l2, eta, its), (leaves, l2_cpu, eta_cpu) in zip(out, cpu):
        print(f"{mesh.n_cells} cells {mesh.n_dofs} dofs: {its} iterations, l2 {l2:.4e} (CPU model {l2_cpu:.4e}), "
              f"eta {eta:.4e} ({eta_cpu:.4e})")
        assert sorted(map(tuple, mesh.cell_levels().tolist())) == sorted(map(tuple, leaves.tolist()))
        assert abs(l2 - l2_cpu) <= 1e-8 * l2_cpu and abs(eta - eta_cpu) <= 1e-8 * eta_cpu
    assert out[-1][1] < out[0][1]


def test_poisson_amr_driver():
    """one line per cycle: cycle cells dofs cg_iterations cg_iterations_from_zero l2_error eta seconds"""
    out = subprocess.run([os.path.join(BIN, "poisson-amr-2d-p2"), "2", "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.strip().splitlines() if not ln.startswith("#")]
    print(out.stdout)
    want = python_loop()
    assert len(lines) == 3 and all(len(f) == 8 for f in lines)
    assert [int(f[1]) for f in lines] == [m.n_cells for m, _, _, _ in want]
    assert [int(f[2]) for f in lines] == [m.n_dofs for m, _, _, _ in want]
    for f, (_, l2, eta, _) in zip(lines, want):
        assert abs(float(f[5]) - l2) <= 1e-6 * l2 and abs(float(f[6]) - eta) <= 1e-6 * eta
    assert float(lines[-1][5]) < float(lines[0][5])
