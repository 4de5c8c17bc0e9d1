"""mfgpu_locate_points (host, plain C++) against the brute-force numpy restatement in tests/points_reference.py: the cell
of every point, the round trip x(xi) = x, and the points outside the mesh.  Location depends on the degree only through
the Gauss points, so p = 1, 2, 4.

Points per mesh: three seeded random points per cell (mapped from random xi), the coordinates of ALL dofs (points on
vertices, edges and faces, where several cells accept and the lowest index must win) and four points at |x|_inf = 2.
On the ball additionally seeded points with |x| <= 0.5, which lie inside the mesh at every n_ref.  Every point inside
must be found: the cap on points left out is zero, and the reference stays within it too."""
import numpy as np
import pytest

import points_reference as ptr
import poisson_reference as pr
import pymfgpu as mf


def one_refined(dim):
    """2^dim cells of level 1, the first one refined once: 7 leaves in 2D, 15 in 3D"""
    rng = (0, 1)
    zs = rng if dim == 3 else (0,)
    coarse = [(1, x, y, z) for z in zs for y in rng for x in rng][1:]
    fine = [(2, x, y, z) for z in zs for y in rng for x in rng]
    return np.array(fine + coarse, dtype=np.uint32)


MESHES = {
    "uniform": lambda dim, p: mf.Mesh.uniform(dim, p, (3, 2) if dim == 2 else (3, 2, 2)),
    "one_refined": lambda dim, p: mf.Mesh.from_leaves(dim, p, one_refined(dim)),
    "adaptive2": lambda dim, p: mf.Mesh.adaptive(dim, p, 2),
    "ball0": lambda dim, p: mf.Mesh.ball(dim, p, 0),
    "ball1": lambda dim, p: mf.Mesh.ball(dim, p, 1),
}
CASES = [(kind, dim, p) for kind in MESHES for dim in (2, 3) for p in (1, 2, 4)]


def outside_points(dim):
    x = np.zeros((4, dim))
    x[0, 0], x[1, 0], x[2, 1], x[3, dim - 1] = 2.0, -2.0, 2.0, -2.0
    x[3, 0] = 0.3
    return x


def inside_points(mesh, cells, kind, seed):
    """the points of the docstring that lie inside the mesh"""
    rng = np.random.default_rng(seed)
    dim, p = cells.dim, cells.p
    parts = [ptr.mapping(p, cells.qpts[c], rng.random((3, dim)))[0] for c in range(mesh.n_cells)]
    parts.append(mesh.dof_coords().copy())
    if kind.startswith("ball"):
        y = rng.standard_normal((40, dim))
        parts.append(0.5 * rng.random((40, 1)) ** (1.0 / dim) * y / np.linalg.norm(y, axis=1, keepdims=True))
    return np.concatenate(parts)


@pytest.mark.parametrize("kind,dim,p", CASES)
def test_locate_matches_brute_force(kind, dim, p):
    mesh = MESHES[kind](dim, p)
    if kind == "one_refined":
        assert mesh.n_cells == (7 if dim == 2 else 15)
    cells = pr.Cells(mesh)
    inside = inside_points(mesh, cells, kind, 100 * dim + p)
    x = np.concatenate([inside, outside_points(dim)])
    cell, xi, missing = mf.locate_points(mesh.desc, x)
    ref_cell, ref_xi, ref_missing = ptr.locate(cells, x)
    n_in = len(inside)
    # every point inside is found (cap on points left out: 0), by the reference too
    assert ref_missing == 4 and np.all(ref_cell[:n_in] != ptr.NOT_FOUND)
    assert missing == 4 and np.all(cell[:n_in] != mf.POINT_NOT_FOUND)
    assert np.all(cell[n_in:] == mf.POINT_NOT_FOUND) and np.all(xi[n_in:] == 0.0)
    np.testing.assert_array_equal(cell, ref_cell)
    assert np.all((xi >= 0.0) & (xi <= 1.0))
    # round trip through the reference's mapping
    worst = 0.0
    for c in np.unique(cell[:n_in]):
        k = np.flatnonzero(cell[:n_in] == c)
        worst = max(worst, np.max(np.abs(ptr.mapping(p, cells.qpts[c], xi[k])[0] - x[k])))
    print(f"{kind} {dim}D p={p}: {n_in} points, round trip {worst:.2e}, "
          f"xi against the reference {np.max(np.abs(xi - ref_xi)):.2e}")
    assert worst <= 1e-12


def test_not_found_and_errors():
    mesh = mf.Mesh.uniform(2, 2, 2)
    cell, xi, missing = mf.locate_points(mesh.desc, np.array([[np.nan, 0.0], [0.0, 0.0], [1.0 + 1e-6, 0.0]]))
    assert missing == 2 and cell[0] == mf.POINT_NOT_FOUND and cell[2] == mf.POINT_NOT_FOUND
    assert cell[1] == 0 and np.all(xi[1] == 1.0)  # the shared vertex: the lowest of the four cells
    cell, xi, missing = mf.locate_points(mesh.desc, np.zeros((0, 2)))
    assert len(cell) == 0 and missing == 0
    # a point within the acceptance tolerance outside the boundary is found and clamped
    cell, xi, missing = mf.locate_points(mesh.desc, np.array([[1.0 + 5e-11, 0.25]]))
    assert missing == 0 and xi[0, 0] == 1.0
    f32 = mf.Mesh.uniform(2, 2, 2, number_type=mf.F32)
    with pytest.raises(mf.MfgpuError) as e:
        mf.locate_points(f32.desc, np.zeros((1, 2)))
    assert e.value.code == mf.EUNSUPPORTED
