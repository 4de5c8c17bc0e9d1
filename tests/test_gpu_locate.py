"""mfgpu_locator_*: point location on the device (locate_kernel) against the host function mfgpu_locate_points, which
tests/test_points_host.py holds equal to the brute-force numpy restatement ptr.locate on these point sets; where a mesh
is new here (the 6-cells-per-direction cube of the bin test) host == ptr.locate is asserted first.

The cell must equal the host's for every point (cap on points left out: 0) and xi must agree to 1e-12, the project's own
bound for a located xi (the round trip of tests/test_points_host.py); the measured maximum is printed.  Meshes: the
3 x 2 (x 2) cube and the 7- / 15-leaf mesh with one refined cell at every p = 1..6 in 2D and 3D (each (dim, p) is its own
instantiation of the kernel), the adaptive stand-in at n_ref 2 and the ball at n_ref 0 and 1 at p = 2, 4.  Points: three
random points per cell, the coordinates of ALL dofs (ties on vertices, edges, faces and the hanging face), the points
outside the mesh, one point with a NaN coordinate.

Cells travel in 4-byte device memory: DeviceVector(n, F32) read back as uint32 (pymfgpu.Locator)."""
import os
import re
import subprocess

import numpy as np
import pytest

import points_reference as ptr
import poisson_reference as pr
import pymfgpu as mf
from stream_harness import Case, check_graph, check_ordered, sets
from test_gpu_evaluate import integrator
from test_gpu_points import run_evaluate, run_integrate, setup
from test_points_host import MESHES, inside_points, outside_points

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")  # (the stream tests; imported before the library first touches the GPU)

PARITY = ([(kind, dim, p) for kind in ("uniform", "one_refined") for dim in (2, 3) for p in range(1, 7)] +
          [(kind, dim, p) for kind in ("adaptive2", "ball0", "ball1") for dim in (2, 3) for p in (2, 4)])
XI_TOL = 1e-12
SENTINEL = np.float32(1.0).view(np.uint32)  # what the cell and count buffers hold before a call

_cache = {}


class Located:
    """a mesh with its integrator and locator"""

    def __init__(self, mesh):
        self.mesh, self.dim = mesh, mesh.desc.dim
        self.it = integrator(mesh)
        self.loc = mf.Locator(self.it, mesh.desc)


def located(kind, dim, p):
    """a mesh of tests/test_points_host.py with the point set of the module docstring and the host's location of it"""
    key = (kind, dim, p)
    if key not in _cache:
        s = Located(MESHES[kind](dim, p))
        nan_row = np.full((1, dim), 0.25)
        nan_row[0, dim - 1] = np.nan
        s.inside = inside_points(s.mesh, pr.Cells(s.mesh), kind, 100 * dim + p)
        s.x = np.concatenate([s.inside, outside_points(dim), nan_row])
        s.x.setflags(write=False)
        s.host = mf.locate_points(s.mesh.desc, s.x)
        _cache[key] = s
    return _cache[key]


def u32_vector(values_or_n):
    """DeviceVector(n, F32) holding uint32 values, or n sentinels (at least one element is allocated)"""
    if np.ndim(values_or_n) == 0:
        v = mf.DeviceVector(max(int(values_or_n), 1), mf.F32)
        v.fill(1.0)
        return v
    a = np.ascontiguousarray(values_or_n, dtype=np.uint32)
    v = mf.DeviceVector(max(len(a), 1), mf.F32)
    if len(a):
        v.from_host(a.view(np.float32))
    return v


def f64_vector(a):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    v = mf.DeviceVector(max(len(a), 1))
    v.from_host(a if len(a) else np.zeros(1))
    return v


def device_locate(s, x, hint=None, count=True, hint_is_cell=False):
    """(cell [n] uint32, xi [n, dim], n_not_found or None) of one call on fresh buffers"""
    x = np.asarray(x, np.float64).reshape(-1, s.dim)
    n = len(x)
    dx = f64_vector(x)
    cell = u32_vector(hint) if hint_is_cell else u32_vector(n)
    xi = mf.DeviceVector(max(n * s.dim, 1))
    xi.fill(np.nan)
    cnt = u32_vector(1) if count else None
    dh = cell if hint_is_cell else (None if hint is None else u32_vector(hint))
    s.loc.locate(dx, cell, xi, hint=dh, n_not_found=cnt, n=n)
    mf.synchronize()
    missing = int(mf.Locator.cells_to_host(cnt)[0]) if count else None
    return mf.Locator.cells_to_host(cell)[:n].copy(), xi.to_host()[:n * s.dim].reshape(n, s.dim), missing


def assert_matches_host(tag, got, host):
    cell, xi, missing = got
    hcell, hxi, hmissing = host
    np.testing.assert_array_equal(cell, hcell)  # every point: the cap on points left out is zero
    worst = float(np.max(np.abs(xi - hxi))) if len(xi) else 0.0
    print(f"{tag}: {len(cell)} points, {hmissing} not found, max |xi_dev - xi_host| = {worst:.3e}, "
          f"bitwise equal: {np.array_equal(xi, hxi)}")
    assert worst <= XI_TOL
    assert np.all((xi >= 0.0) & (xi <= 1.0))
    assert np.all(xi[cell == mf.POINT_NOT_FOUND] == 0.0)
    if missing is not None:
        assert missing == hmissing


@pytest.mark.parametrize("kind,dim,p", PARITY)
def test_parity_with_host(kind, dim, p):
    s = located(kind, dim, p)
    n_in = len(s.inside)
    hcell, _, hmissing = s.host
    assert hmissing == 5 and np.all(hcell[:n_in] != mf.POINT_NOT_FOUND) and np.all(hcell[n_in:] == mf.POINT_NOT_FOUND)
    assert_matches_host(f"{kind} {dim}D p={p}", device_locate(s, s.x), s.host)
    assert s.loc.memory_consumption() > 0


@pytest.mark.parametrize("dim,p", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_bins(dim, p):
    """6 cells per direction: 6 bins per direction, every cell's box in its own bin and (by its inflation) its
    neighbours'"""
    mesh = mf.Mesh.uniform(dim, p, 6)
    cells = pr.Cells(mesh)
    rng = np.random.default_rng(60 + 10 * dim + p)
    x = np.concatenate([ptr.mapping(p, cells.qpts[c], rng.random((2, dim)))[0] for c in range(mesh.n_cells)])
    x = np.concatenate([x[rng.permutation(len(x))], mesh.dof_coords()])
    host = mf.locate_points(mesh.desc, x)
    ref_cell, ref_xi, ref_missing = ptr.locate(cells, x)
    np.testing.assert_array_equal(host[0], ref_cell)
    assert host[2] == 0 == ref_missing and np.max(np.abs(host[1] - ref_xi)) <= XI_TOL
    assert_matches_host(f"bins {dim}D p={p}", device_locate(Located(mesh), x), host)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_sizes(n):
    """tail lanes and the launch with no points; the buffers behind the n-th entry stay as they were"""
    s = located("one_refined", 3, 2)
    reps = -(-max(n, 1) // len(s.x))
    x = np.tile(s.x, (reps, 1))[:n]
    host = mf.locate_points(s.mesh.desc, x)
    assert_matches_host(f"n = {n}", device_locate(s, x), host)
    cell, xi = u32_vector(n + 70), mf.DeviceVector((n + 70) * 3)
    xi.fill(np.nan)
    s.loc.locate(f64_vector(x), cell, xi, n=n)
    mf.synchronize()
    c, t = mf.Locator.cells_to_host(cell), xi.to_host()
    np.testing.assert_array_equal(c[:n], host[0])
    assert np.all(c[n:] == SENTINEL) and np.all(np.isnan(t[n * 3:])) and not np.any(np.isnan(t[:n * 3]))


def test_known_answers():
    """the cases of test_points_host.test_not_found_and_errors"""
    mesh = mf.Mesh.uniform(2, 2, 2)
    s = Located(mesh)
    x = np.array([[np.nan, 0.0], [0.0, 0.0], [1.0 + 1e-6, 0.0], [1.0 + 5e-11, 0.25]])
    cell, xi, missing = device_locate(s, x)
    assert missing == 2 and cell[0] == mf.POINT_NOT_FOUND and cell[2] == mf.POINT_NOT_FOUND
    assert np.all(xi[[0, 2]] == 0.0)
    assert cell[1] == 0 and np.all(xi[1] == 1.0)  # the shared vertex: the lowest of the four cells
    assert cell[3] != mf.POINT_NOT_FOUND and xi[3, 0] == 1.0  # within the acceptance tolerance: found and clamped
    assert_matches_host("known answers", (cell, xi, missing), mf.locate_points(mesh.desc, x))


@pytest.mark.parametrize("kind,dim,p", [("one_refined", 2, 2), ("one_refined", 3, 2), ("one_refined", 3, 4),
                                        ("ball1", 2, 2), ("ball1", 3, 2), ("ball1", 3, 4)])
def test_hints_do_not_change_the_result(kind, dim, p):
    """every kind of hint gives the bits of the unhinted call; the dof coordinates sit on faces and vertices, where a
    hint is wrong by construction (the hinted cell converges on its boundary, outside the hint margin)"""
    s = located(kind, dim, p)
    nc, n = s.mesh.n_cells, len(s.x)
    plain = device_locate(s, s.x)
    assert_matches_host(f"hints {kind} {dim}D p={p}", plain, s.host)
    hcell = s.host[0]
    variants = {
        "correct": hcell,
        "off by one": ((hcell.astype(np.uint64) + 1) % nc).astype(np.uint32),
        "not found": np.full(n, mf.POINT_NOT_FOUND, np.uint32),
        "out of range": np.resize(np.array([nc, nc + 7, 0x7fffffff, 0xfffffffe], np.uint32), n),
    }
    for name, hint in variants.items():
        for same_buffer in (False, True):
            cell, xi, missing = device_locate(s, s.x, hint=hint, hint_is_cell=same_buffer)
            np.testing.assert_array_equal(cell, plain[0], err_msg=f"{name}, hint is cell: {same_buffer}")
            np.testing.assert_array_equal(xi, plain[1], err_msg=f"{name}, hint is cell: {same_buffer}")
            assert missing == plain[2]


@pytest.mark.parametrize("kind,dim,p", [("one_refined", 2, 3), ("one_refined", 3, 4), ("ball1", 3, 2)])
def test_bitwise_repeatable(kind, dim, p):
    s = located(kind, dim, p)
    first = device_locate(s, s.x)
    for _ in range(2):
        again = device_locate(s, s.x)
        np.testing.assert_array_equal(again[0], first[0])
        np.testing.assert_array_equal(again[1], first[1])
        assert again[2] == first[2]


def stream_cases():
    out = []
    for kind, dim, p in (("one_refined", 3, 2), ("ball1", 2, 2)):
        s = located(kind, dim, p)
        n = 700
        x = sets(lambda rng: -1.1 + 2.2 * rng.random(n * dim), 401 + dim)  # some of them outside the mesh
        for count in (True, False):
            def check(k, got, ret, s=s, x=x, dim=dim, count=count):
                host = mf.locate_points(s.mesh.desc, x[k].reshape(-1, dim))
                assert 0 < host[2] < n
                missing = int(got["count"].view(np.uint32)[0]) if count else None
                assert_matches_host("stream", (got["cell"].view(np.uint32), got["xi"].reshape(-1, dim), missing), host)

            outputs = {"cell": (np.float32, n), "xi": (np.float64, n * dim)}
            if count:
                outputs["count"] = (np.float32, 1)
            out.append(Case(f"locate-{kind}{dim}d-{'count' if count else 'nocount'}", {"x": x}, outputs,
                            lambda b, st, s=s: s.loc.locate(b["x"], b["cell"], b["xi"], n_not_found=b.get("count"),
                                                            stream=st), check))
    return out


@pytest.mark.parametrize("index", range(4))
def test_stream_order(index):
    check_ordered(stream_cases()[index])


@pytest.mark.parametrize("index", range(4))
def test_graph_capture(index):
    check_graph(stream_cases()[index])


@pytest.mark.parametrize("kind,dim,p", [(kind, dim, p) for kind in ("hanging", "ball") for dim in (2, 3) for p in (2, 4)])
def test_points_located(kind, dim, p):
    """Points.located on the device's location gives the bits of Points.in_cells on the host's location, in evaluate
    (values and gradients) and in integrate"""
    s = setup(kind, dim, p)
    n = len(s.x)
    hcell, hxi, hmissing = mf.locate_points(s.mesh.desc, s.x)
    assert hmissing == 0
    loc = mf.Locator(s.it, s.mesh.desc)
    cell, xi = u32_vector(n), mf.DeviceVector(n * dim)
    loc.locate(f64_vector(s.x), cell, xi)
    dev = mf.Points.located(s.it, cell, xi, n)  # synchronises
    ref = mf.Points.in_cells(s.it, hcell, hxi)
    assert dev.n == n and dev.n_not_found == 0
    np.testing.assert_array_equal(dev.cells, hcell)
    print(f"{kind} {dim}D p={p}: max |xi_dev - xi_host| = {np.max(np.abs(xi.to_host().reshape(-1, dim) - hxi)):.3e}")
    v, g = run_evaluate(dev, s.u, dim)
    rv, rg = run_evaluate(ref, s.u, dim)
    np.testing.assert_array_equal(v, rv)
    np.testing.assert_array_equal(g, rg)
    w = np.random.default_rng(31).standard_normal(n)
    np.testing.assert_array_equal(run_integrate(dev, s.mesh.n_dofs, w), run_integrate(ref, s.mesh.n_dofs, w))
    np.testing.assert_array_equal(run_integrate(dev, s.mesh.n_dofs), run_integrate(ref, s.mesh.n_dofs))


def test_errors():
    s = located("uniform", 2, 2)
    f32 = mf.Mesh.uniform(2, 2, (3, 2), number_type=mf.F32)
    with pytest.raises(mf.MfgpuError) as e:  # an F32 description gives no integrator ...
        mf.Integrator(f32.desc, f32)
    assert e.value.code == mf.EUNSUPPORTED
    with pytest.raises(mf.MfgpuError) as e:  # ... and no locator
        mf.Locator(s.it, f32.desc)
    assert e.value.code == mf.EUNSUPPORTED
    for other in (mf.Mesh.uniform(2, 2, 2), mf.Mesh.uniform(2, 3, (3, 2)), mf.Mesh.uniform(3, 2, (3, 2, 1))):
        with pytest.raises(mf.MfgpuError) as e:
            mf.Locator(s.it, other.desc)
        assert e.value.code == mf.EINVAL
    x, cell, xi = f64_vector(s.x[:1]), u32_vector(1), mf.DeviceVector(2)
    for args in ((None, cell, xi), (x, None, xi), (x, cell, None)):
        with pytest.raises(mf.MfgpuError) as e:
            s.loc.locate(*args, n=1)
        assert e.value.code == mf.EINVAL
    s.loc.locate(None, None, None, n=0)  # allowed
    with pytest.raises(mf.MfgpuError) as e:
        mf.Points.located(s.it, None, xi, 1)
    assert e.value.code == mf.EINVAL


HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dealii-cuda_amd", "host", "bin")


@pytest.mark.parametrize("name", ["2d-p2", "3d-p4", "3d-p4-adaptive", "3d-p4-ball"])
def test_probe_driver_device_location(name):
    """each -devloc binary prints the found count and the error lines of its counterpart, to the printed digits, and
    reports no cell that differs from the host's location.

    The ball's "max point error" is the exception, and not because of the location: the general-geometry operator of the
    solve sums with atomics, and the unchanged poisson-probe-3d-p4-ball printed 1.076738624517e-05, ...511e-05 and
    ...528e-05 in consecutive runs of itself while the located cells and xi of both binaries were bit for bit the same.
    That line is compared to 1e-10, the bound host/probe.cc states for its point values across implementations and
    test_gpu_points.test_probe_driver applies; every other line of the ball, and every line of the other three drivers
    (whose solves are reproducible), to the printed digits."""
    def run(exe):
        r = subprocess.run([os.path.join(HOST, exe), "2", "200"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        return r.stdout

    base, dev = run(f"poisson-probe-{name}"), run(f"poisson-probe-{name}-devloc")
    print(dev)
    for pattern in (r"points found:\s*(\d+ of \d+)", r"max point error:\s*(\S+)", r"L2 error:\s*(\S+)"):
        a, b = re.search(pattern, base), re.search(pattern, dev)
        assert a and b, (pattern, base[-600:], dev[-600:])
        if name.endswith("ball") and pattern.startswith("max point"):
            assert abs(float(a.group(1)) - float(b.group(1))) <= 1e-10, (base[-600:], dev[-600:])
        else:
            assert a.group(1) == b.group(1), (pattern, base[-600:], dev[-600:])
    assert re.search(r"points found:\s*200 of 200", dev)
    m = re.search(r"device location: (\d+) cells differ from the host's, max \|xi_dev - xi_host\| (\S+)", dev)
    assert m and int(m.group(1)) == 0 and float(m.group(2)) <= XI_TOL, dev[-600:]
