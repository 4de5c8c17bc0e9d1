"""mfgpu_points_*: a field and its gradient at arbitrary points (points_evaluate_kernel) and the transpose of the value
part, point sources (points_integrate_kernel + points_gather_kernel), against the numpy restatement in
tests/points_reference.py and against known answers.

Meshes: the uniform 2 x 2 (x 2) cube and the 7- / 15-leaf mesh with one refined cell at every p = 1..6 in 2D and 3D (each
(dim, p) is its own instantiation of both kernels), the ball at n_ref 1 at p = 2, 4.  The field is a seeded random dof
vector, nonzero on the constrained dofs (they are read); the dofs no cell lists (hanging dofs) are NaN (they are not).
Tolerance: 1e-12 relative to the largest reference entry, the project's own (tests/test_gpu_evaluate.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import points_reference as ptr
import poisson_reference as pr
import pymfgpu as mf
from oracle import mf_oracle as o
from stream_harness import Case, check_graph, check_ordered, sets
from test_gpu_evaluate import integrator, nan_vector
from test_gpu_poisson import close, dv
from test_points_host import one_refined

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")  # (the stream tests; imported before the library first touches the GPU)

CUBES = [(kind, dim, p) for kind in ("cube", "hanging") for dim in (2, 3) for p in range(1, 7)]
BALLS = [("ball", dim, p) for dim in (2, 3) for p in (2, 4)]
CASES = CUBES + BALLS
POINTS_PER_ITEM = 512  # kPointsPerItem (csrc/mfgpu_points.h)

_cache = {}


class Setup:
    def __init__(self, kind, dim, p):
        if kind == "cube":
            self.mesh = mf.Mesh.uniform(dim, p, 2)
        elif kind == "hanging":
            self.mesh = mf.Mesh.from_leaves(dim, p, one_refined(dim))
        else:
            self.mesh = mf.Mesh.ball(dim, p, 1)
        mesh = self.mesh
        self.kind, self.dim, self.p = kind, dim, p
        self.cells = pr.Cells(mesh)
        self.it = integrator(mesh)
        self.unread = ptr.unread_dofs(mesh)
        assert (kind == "hanging") == bool(self.unread.any())
        rng = np.random.default_rng(1000 * dim + 10 * p + len(kind))
        self.u = rng.standard_normal(mesh.n_dofs)
        self.u0 = np.where(self.unread, 0.0, self.u)  # what the reference reads
        self.u[self.unread] = np.nan
        # five random points per cell, in an order that is not the cell order
        xi = rng.random((5 * mesh.n_cells, dim))
        cell = np.repeat(np.arange(mesh.n_cells), 5)
        x = np.concatenate([ptr.mapping(p, self.cells.qpts[c], xi[cell == c])[0] for c in range(mesh.n_cells)])
        self.x = x[rng.permutation(len(x))]
        self.x.setflags(write=False)
        self.u.setflags(write=False)
        self._ref = None

    @property
    def ref(self):
        """the reference's own location of self.x and its PointsRef"""
        if self._ref is None:
            cell, xi, missing = ptr.locate(self.cells, self.x)
            assert missing == 0
            self._ref = ptr.PointsRef(self.cells, cell, xi)
        return self._ref


def setup(kind, dim, p):
    key = (kind, dim, p)
    if key not in _cache:
        _cache[key] = Setup(kind, dim, p)
    return _cache[key]


def run_evaluate(pts, u, dim):
    v, g = nan_vector(max(pts.n, 1)), nan_vector(max(pts.n, 1) * dim)
    pts.evaluate(dv(u), v, g)
    mf.synchronize()
    return v.to_host()[:pts.n], g.to_host()[:pts.n * dim].reshape(-1, dim)


def run_integrate(pts, n_dofs, w=None):
    r = nan_vector(n_dofs)
    pts.integrate(r, None if w is None else dv(w))
    mf.synchronize()
    return r.to_host()


@pytest.mark.parametrize("kind,dim,p", CASES)
def test_nodal_property(kind, dim, p):
    """at the coordinates of every dof that is not hanging, evaluate returns u[dof]"""
    s = setup(kind, dim, p)
    dofs = np.flatnonzero(~s.unread)
    pts = mf.Points(s.it, s.mesh.desc, s.mesh.dof_coords()[dofs])
    assert pts.n_not_found == 0 and np.all(pts.cells < s.mesh.n_cells)
    v, _ = run_evaluate(pts, s.u, dim)
    close(v, s.u[dofs], 1e-12)


@pytest.mark.parametrize("kind,dim,p", CASES)
def test_polynomial_exactness(kind, dim, p):
    """cube meshes: the nodal interpolant of a tensor polynomial of degree p per direction is that polynomial; ball:
    a + b . x gives a + b . x_k and the gradient b"""
    from test_nonlinear_host import _poly
    s = setup(kind, dim, p)
    if kind == "ball":
        b = np.arange(1, dim + 1) * 0.5
        value, gradient = (lambda x: 0.25 + x @ b), (lambda x: np.broadcast_to(b, x.shape))
    else:
        value, gradient = _poly(dim, p, 7)
    u = value(s.mesh.dof_coords())
    u[s.unread] = np.nan
    pts = mf.Points(s.it, s.mesh.desc, s.x)
    assert pts.n_not_found == 0
    v, g = run_evaluate(pts, u, dim)
    close(v, value(s.x), 1e-12)
    close(g, gradient(s.x), 1e-12)


@pytest.mark.parametrize("kind,dim,p", CASES)
def test_parity_with_reference(kind, dim, p):
    s = setup(kind, dim, p)
    pts = mf.Points(s.it, s.mesh.desc, s.x)
    np.testing.assert_array_equal(pts.cells, s.ref.cell)
    vals, grads = s.ref.evaluate(s.u0)
    v, g = run_evaluate(pts, s.u, dim)
    close(v, vals, 1e-12)
    close(g, grads, 1e-12)
    # values only, gradients only: the same bits
    v2, g2 = nan_vector(pts.n), nan_vector(pts.n * dim)
    pts.evaluate(dv(s.u), values=v2)
    pts.evaluate(dv(s.u), gradients=g2)
    mf.synchronize()
    np.testing.assert_array_equal(v2.to_host(), v)
    np.testing.assert_array_equal(g2.to_host().reshape(-1, dim), g)


@pytest.mark.parametrize("kind,dim,p", CASES)
def test_tie_to_integrator_evaluate(kind, dim, p):
    """in_cells with xi = the Gauss points of every cell reproduces Integrator.evaluate, values and gradients"""
    s = setup(kind, dim, p)
    mesh, n = s.mesh, p + 1
    xq = o.gauss_01(n)[0]
    grid = np.stack(np.meshgrid(*([xq] * dim), indexing="ij"), axis=-1).reshape(-1, dim)[:, ::-1]  # x fastest
    cell = np.repeat(np.arange(mesh.n_cells, dtype=np.uint32), mesh.nd)
    pts = mf.Points.in_cells(s.it, cell, np.tile(grid, (mesh.n_cells, 1)))
    npts = mesh.n_cells * mesh.nd
    rv, rg = nan_vector(npts), nan_vector(npts * dim)
    s.it.evaluate(dv(s.u), rv, rg)
    v, g = run_evaluate(pts, s.u, dim)
    close(v, rv.to_host(), 1e-12)
    close(g.reshape(-1), rg.to_host(), 1e-12)


@pytest.mark.parametrize("dim,p", [(2, 1), (2, 3), (2, 6), (3, 2), (3, 4), (3, 5)])
def test_hanging_face_is_continuous(dim, p):
    """the same physical points on the face between the refined cell's children and a coarse neighbour, given once in the
    fine cells and once in the coarse cell: the values agree (the normal derivative may jump: gradients not compared)"""
    s = setup("hanging", dim, p)
    leaves = s.mesh.cell_levels().reshape(-1, 4)
    coarse = int(np.flatnonzero((leaves[:, 0] == 1) & (leaves[:, 1] == 1) & (leaves[:, 2] == 0) & (leaves[:, 3] == 0))[0])
    fine = np.flatnonzero((leaves[:, 0] == 2) & (leaves[:, 1] == 1))  # the children that touch the face x = 0
    assert len(fine) == 2 ** (dim - 1)
    rng = np.random.default_rng(dim * 10 + p)
    cf, xf, xc = [], [], []
    for c in fine:
        xi = rng.random((6, dim))
        xi[:, 0] = 1.0
        xi[0, 1:] = 0.0  # a vertex and an edge of the fine face too
        xi[1, 1] = 1.0
        x = ptr.mapping(p, s.cells.qpts[c], xi)[0]
        acc, t = ptr.newton(p, s.cells.qpts[coarse], x)
        assert np.all(acc) and np.all(np.abs(t[:, 0]) <= 1e-13)
        cf += [c] * len(xi)
        xf.append(xi)
        xc.append(t)
    vf, _ = run_evaluate(mf.Points.in_cells(s.it, cf, np.concatenate(xf)), s.u, dim)
    vc, _ = run_evaluate(mf.Points.in_cells(s.it, [coarse] * len(cf), np.concatenate(xc)), s.u, dim)
    close(vf, vc, 1e-12)


# the work-item bound is 512 points: 1000 takes two work items, 1025 three (the last holds one point)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 512, 513, 1000, 1025])
def test_chunking_one_cell_holds_all_points(n):
    s = setup("hanging", 3, 2)
    masked = int(np.flatnonzero(s.mesh.arrays()["constraint_mask"])[-1])
    rng = np.random.default_rng(n)
    cell, xi, w = np.full(n, masked, np.uint32), rng.random((n, 3)), rng.standard_normal(n)
    pts = mf.Points.in_cells(s.it, cell, xi)
    ref = ptr.PointsRef(s.cells, cell, xi)
    vals, grads = ref.evaluate(s.u0)
    v, g = run_evaluate(pts, s.u, 3)
    close(v, vals, 1e-12)
    close(g, grads, 1e-12)
    close(run_integrate(pts, s.mesh.n_dofs, w), ref.integrate(w), 1e-12)
    close(run_integrate(pts, s.mesh.n_dofs), ref.integrate(), 1e-12)


def test_no_points_and_only_points_without_a_cell():
    s = setup("cube", 3, 2)
    empty = mf.Points.in_cells(s.it, np.zeros(0, np.uint32), np.zeros((0, 3)))
    assert empty.n == 0 and empty.n_not_found == 0 and len(empty.cells) == 0
    v, g = nan_vector(1), nan_vector(3)
    empty.evaluate(dv(s.u), v, g)  # MFGPU_OK, nothing to write
    assert np.all(run_integrate(empty, s.mesh.n_dofs) == 0.0)
    lost = mf.Points(s.it, s.mesh.desc, np.array([[2.0, 0.0, 0.0], [0.0, -2.0, 0.0], [0.0, 0.0, 2.0]] * 30))
    assert lost.n_not_found == 90 and np.all(lost.cells == mf.POINT_NOT_FOUND)
    v, g = run_evaluate(lost, s.u, 3)
    assert np.all(v == 0.0) and np.all(g == 0.0)
    assert np.all(run_integrate(lost, s.mesh.n_dofs, np.ones(90)) == 0.0)
    # found and lost points mixed: zeros exactly where the lost ones are
    x = np.concatenate([s.x[:7], [[2.0, 0.0, 0.0]], s.x[7:9], [[0.0, 2.0, 0.0]]])
    mixed = mf.Points(s.it, s.mesh.desc, x)
    assert mixed.n_not_found == 2
    ref = ptr.PointsRef(s.cells, *ptr.locate(s.cells, x)[:2])
    v, g = run_evaluate(mixed, s.u, 3)
    close(v, ref.evaluate(s.u0)[0], 1e-12)
    assert v[7] == 0.0 and v[10] == 0.0 and np.all(g[[7, 10]] == 0.0)
    close(run_integrate(mixed, s.mesh.n_dofs), ref.integrate(), 1e-12)


def many_points(s, seed):
    """the setup's points plus 1100 more in one masked (or the last) cell: that cell has three work items"""
    rng = np.random.default_rng(seed)
    mask = s.mesh.arrays()["constraint_mask"]
    c = int(np.flatnonzero(mask)[0]) if mask is not None and mask.any() else s.mesh.n_cells - 1
    cell = np.concatenate([s.ref.cell, np.full(1100, c, np.uint32)])
    xi = np.concatenate([s.ref.xi, rng.random((1100, s.dim))])
    order = rng.permutation(len(cell))
    return cell[order], xi[order]


@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 3), ("hanging", 2, 2), ("hanging", 3, 1), ("hanging", 3, 4),
                                        ("hanging", 3, 6), ("ball", 3, 2)])
def test_integrate_is_the_transpose(kind, dim, p):
    s = setup(kind, dim, p)
    cell, xi = many_points(s, 5)
    assert np.max(np.bincount(cell)) > 2 * POINTS_PER_ITEM
    pts = mf.Points.in_cells(s.it, cell, xi)
    ref = ptr.PointsRef(s.cells, cell, xi)
    rng = np.random.default_rng(17)
    w = rng.standard_normal(len(cell))
    con = s.cells.od.constrained
    rhs = run_integrate(pts, s.mesh.n_dofs, w)
    close(rhs, ref.integrate(w), 1e-12)
    assert np.all(rhs[con] == 0.0) and np.all(rhs[s.unread] == 0.0)
    close(run_integrate(pts, s.mesh.n_dofs), ref.integrate(), 1e-12)
    # <w, evaluate(u)> = <integrate(w), u> for u that is 0 on the constrained dofs
    u = rng.standard_normal(s.mesh.n_dofs)
    u[con] = 0.0
    u[s.unread] = np.nan
    v, _ = run_evaluate(pts, u, dim)
    lhs, rhs_dot = float(w @ v), float(rhs @ np.where(s.unread, 0.0, u))
    scale = float(np.abs(w) @ np.abs(v))
    print(f"{kind} {dim}D p={p}: <w, E u> = {lhs:.15e}, <E^T w, u> = {rhs_dot:.15e}, scale {scale:.3e}")
    assert abs(lhs - rhs_dot) <= 1e-12 * scale


@pytest.mark.parametrize("kind,dim,p", [("hanging", 2, 3), ("hanging", 3, 4), ("ball", 3, 2)])
def test_bitwise_repeatable(kind, dim, p):
    s = setup(kind, dim, p)
    cell, xi = many_points(s, 6)
    pts = mf.Points.in_cells(s.it, cell, xi)
    w = np.random.default_rng(3).standard_normal(len(cell))
    v0, g0 = run_evaluate(pts, s.u, dim)
    r0 = run_integrate(pts, s.mesh.n_dofs, w)
    for _ in range(3):
        v, g = run_evaluate(pts, s.u, dim)
        np.testing.assert_array_equal(v, v0)
        np.testing.assert_array_equal(g, g0)
        np.testing.assert_array_equal(run_integrate(pts, s.mesh.n_dofs, w), r0)
    # a second object from the same points: the same bits
    again = mf.Points.in_cells(s.it, cell, xi)
    np.testing.assert_array_equal(run_integrate(again, s.mesh.n_dofs, w), r0)


def stream_cases():
    out = []
    for kind, dim, p in (("hanging", 3, 2), ("ball", 2, 2)):
        s = setup(kind, dim, p)
        cell, xi = many_points(s, 8)
        pts = mf.Points.in_cells(s.it, cell, xi)
        ref = ptr.PointsRef(s.cells, cell, xi)
        n, nd = len(cell), s.mesh.n_dofs
        u = sets(lambda rng: np.where(s.unread, np.nan, rng.standard_normal(nd)), 301)
        w = sets(lambda rng: rng.standard_normal(n), 302)

        def check_eval(k, got, ret, ref=ref, u=u, s=s, dim=dim):
            vals, grads = ref.evaluate(np.where(s.unread, 0.0, u[k]))
            close(got["values"], vals, 1e-12)
            close(got["gradients"], grads.reshape(-1), 1e-12)

        def check_int(k, got, ret, ref=ref, w=w):
            close(got["rhs"], ref.integrate(w[k]), 1e-12)
        out.append(Case(f"points_evaluate-{kind}{dim}d", {"u": u}, {"values": (np.float64, n), "gradients": (np.float64, n * dim)},
                        lambda b, st, pts=pts: pts.evaluate(b["u"], b["values"], b["gradients"], st), check_eval))
        out.append(Case(f"points_integrate-{kind}{dim}d", {"w": w}, {"rhs": (np.float64, nd)},
                        lambda b, st, pts=pts: pts.integrate(b["rhs"], b["w"], st), check_int))
    return out


@pytest.mark.parametrize("index", range(4))
def test_stream_order(index):
    check_ordered(stream_cases()[index])


@pytest.mark.parametrize("index", range(4))
def test_graph_capture(index):
    check_graph(stream_cases()[index])


def test_errors():
    s = setup("cube", 2, 2)
    it, nc = s.it, s.mesh.n_cells
    f32 = mf.Mesh.uniform(2, 2, 2, number_type=mf.F32)
    with pytest.raises(mf.MfgpuError) as e:  # an F32 description gives no integrator ...
        mf.Integrator(f32.desc, f32)
    assert e.value.code == mf.EUNSUPPORTED
    with pytest.raises(mf.MfgpuError) as e:  # ... and no points object
        mf.Points(it, f32.desc, np.zeros((1, 2)))
    assert e.value.code == mf.EUNSUPPORTED
    pts = mf.Points.in_cells(it, [0], [[0.5, 0.5]])
    with pytest.raises(mf.MfgpuError, match="error -1.*both NULL"):
        pts.evaluate(dv(s.u))
    for cell, xi in (([nc], [[0.5, 0.5]]), ([0, nc + 5], [[0.5, 0.5]] * 2), ([0], [[0.5, 1.0 + 1e-12]]),
                     ([0], [[-1e-12, 0.5]]), ([0], [[np.nan, 0.5]])):
        with pytest.raises(mf.MfgpuError) as e:
            mf.Points.in_cells(it, cell, xi)
        assert e.value.code == mf.EINVAL
    mf.Points.in_cells(it, [0, mf.POINT_NOT_FOUND], [[0.0, 1.0], [7.0, 7.0]])  # allowed: xi of a lost point is not read
    assert pts.memory_consumption() > 0


HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dealii-cuda_amd", "host", "bin")


@pytest.mark.parametrize("dim,p", [(2, 2), (3, 4)])
def test_probe_driver(dim, p):
    """host/probe.cc on the C-ABI alone: all points found, and its maximum point error is what Points.evaluate gives in
    Python for the same solve and the same points"""
    n_ref, n_points = 2, 200
    exe = os.path.join(HOST, f"poisson-probe-{dim}d-p{p}")
    run = subprocess.run([exe, str(n_ref), str(n_points)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout[-3000:]
    print(run.stdout)
    m = re.search(r"points found:\s*(\d+) of (\d+)", run.stdout)
    assert m and int(m.group(1)) == n_points == int(m.group(2)), run.stdout[-3000:]
    err = float(re.search(r"max point error:\s*(\S+)", run.stdout).group(1))
    # the same solve through the numpy reference's linear algebra, evaluated by Points.evaluate at the driver's points
    mesh = mf.Mesh.uniform(dim, p, 1 << n_ref)
    cells = pr.Cells(mesh)
    u, _ = cells.solve()
    x = probe_points(dim, n_points)
    pts = mf.Points(integrator(mesh), mesh.desc, x)
    assert pts.n_not_found == 0
    v, _ = run_evaluate(pts, u, dim)
    mine = float(np.max(np.abs(v - pr.solution(x))))
    print(f"probe {dim}D p={p}: driver {err:.12e}, python {mine:.12e}")
    assert abs(err - mine) <= 1e-10


def probe_points(dim, n):
    """the fixed seeded point set of host/probe.cc: xorshift32 from 2463534242, coordinates in (-0.999, 0.999)"""
    state, out = 2463534242, np.zeros((n, dim))
    for k in range(n):
        for d in range(dim):
            state ^= (state << 13) & 0xFFFFFFFF
            state ^= state >> 17
            state ^= (state << 5) & 0xFFFFFFFF
            out[k, d] = -0.999 + 1.998 * (state / 4294967296.0)
    return out
