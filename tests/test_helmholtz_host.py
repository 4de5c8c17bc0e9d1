"""Mass term (mfgpu_desc.mass_coefficient), host side: the numpy reference of tests/helmholtz_reference.py checked
against itself and against an analytic integral, the ctypes mirror of mfgpu_desc, the plan's independence of the
field, and the helmholtz drivers of the build.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import helmholtz_reference as hr
import poisson_reference as pr
import pymfgpu as mf
from util import desc_from_oracle, oracle_desc_from_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def random_c(od, seed=0):
    """c in [0.5, 1.5] per quadrature point: no structure a wrong layout could hide behind"""
    return np.random.default_rng(seed).uniform(0.5, 1.5, (od.n_cells, od.nd))


MESHES = [("cube", 2, 1), ("cube", 2, 3), ("cube", 3, 2), ("cube", 3, 4), ("hanging", 2, 2), ("hanging", 3, 2),
          ("hanging", 3, 3), ("ball", 2, 2), ("ball", 3, 2)]


def small_mesh(kind, dim, p):
    if kind == "cube":
        return mf.Mesh.uniform(dim, p, 3 if dim == 2 or p <= 2 else 2)
    if kind == "hanging":
        return mf.Mesh.adaptive(dim, p, 3 if dim == 2 else 4)
    return mf.Mesh.ball(dim, p, 1 if dim == 2 else 0)


@pytest.mark.parametrize("kind,dim,p", MESHES)
def test_reference_forms_agree(kind, dim, p):
    """sum-factorised apply == assembled apply, vmult and vmult_add; the diagonal of the assembled matrix on meshes
    without hanging nodes (there the distributed local diagonal is not the matrix diagonal, as for the Laplacian)"""
    mesh = small_mesh(kind, dim, p)
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    c = random_c(od, p)
    A = hr.assemble(od, c)
    rng = np.random.default_rng(dim * 10 + p)
    x, y0 = rng.standard_normal(od.n_dofs), rng.standard_normal(od.n_dofs)
    assert rel(hr.vmult(od, c, x), A @ x) <= 1e-12
    assert rel(hr.vmult_add(od, c, y0, x), y0 + A @ x) <= 1e-12  # (identity rows: dst_c += src_c)
    assert abs(A - A.T).max() <= 1e-12 * abs(A).max()
    if kind != "hanging":
        assert rel(1.0 / hr.inverse_diagonal(od, c), A.diagonal()) <= 1e-12


@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 2), ("cube", 2, 4), ("cube", 3, 2), ("cube", 3, 3), ("hanging", 2, 2),
                                        ("hanging", 3, 2), ("hanging", 3, 4)])
def test_known_answer_mass_energy(kind, dim, p):
    """coefficient = 0, c = 1, u = prod_d (1 - x_d^2): u^T A u = int u^2 = (16/15)^dim, an integral no table of the
    product enters.  u^2 has degree 4 per direction and QGauss(p+1) is exact to degree 2p + 1 >= 5."""
    mesh = small_mesh(kind, dim, p)
    od = oracle_desc_from_mesh(mesh, dtype=np.float64)
    od.coefficient[:] = 0.0
    c = np.ones((od.n_cells, od.nd))
    u = hr.known_answer_vector(mesh.dof_coords(), od.constrained)
    exact = (16.0 / 15.0) ** dim
    assert abs(u @ hr.vmult(od, c, u) - exact) <= 1e-12 * exact
    assert abs(u @ (hr.assemble(od, c) @ u) - exact) <= 1e-12 * exact


def test_lift_is_minus_operator():
    """rhs with f = 0 and a lift u_b: minus the unconstrained Helmholtz operator on u_b, on the free rows"""
    for kind, dim, p in [("cube", 2, 2), ("hanging", 2, 2), ("ball", 2, 2), ("hanging", 3, 2)]:
        mesh = small_mesh(kind, dim, p)
        cells = pr.Cells(mesh)
        od = cells.od
        c = random_c(od, 3)
        ub = np.random.default_rng(7).standard_normal(od.n_dofs)
        got = hr.rhs(cells, c, np.zeros((od.n_cells, od.nd)), ub)
        from oracle import mf_oracle as o
        un = o.Desc(od.dim, od.degree, od.n_dofs, od.loc2glob, od.JxW, od.inv_jac, od.coefficient, np.zeros(0, np.uint32),
                    od.constraint_mask, np.float64, od.shape_values, od.shape_gradients, od.weights)
        free = np.ones(od.n_dofs, bool)
        free[od.constrained] = False
        ref = -(hr.assemble(un, c) @ ub)
        assert np.abs(got[free] - ref[free]).max() <= 1e-12 * np.abs(ref).max()
        assert np.all(got[~free] == 0.0)


def test_desc_mirror_matches_header():
    assert ctypes.sizeof(mf.Desc) == mf.lib().mfgpu_desc_size()
    assert mf.Desc.mass_coefficient.offset + ctypes.sizeof(ctypes.c_void_p) == ctypes.sizeof(mf.Desc)  # the last field
    assert "mfgpu_desc_size" in mf.SYMBOLS


PLAN_ARRAYS = ["batch_cell_off", "batch_dof_off", "color_batch_off", "cell_order", "bdofs", "orphans", "batch_nint",
               "halo_off", "sdofs", "s_off", "s_idx", "chunks", "gstarts", "pr_dofs", "pr_idx", "pr_hn", "pr_hn_slot",
               "sh_dofs", "sh_idx", "sh_batch", "sh_p2rec", "sh_p2tab", "lmap", "bflags"]


@pytest.mark.parametrize("make", [lambda: mf.Mesh.uniform(3, 4, 6), lambda: mf.Mesh.uniform(3, 5, 3),
                                  lambda: mf.Mesh.uniform(2, 2, 9), lambda: mf.Mesh.adaptive(3, 4, 4),
                                  lambda: mf.Mesh.adaptive(2, 2, 4), lambda: mf.Mesh.ball(3, 2, 1),
                                  lambda: mf.Mesh.ball(2, 2, 2)],
                         ids=["cube_p4", "cube_p5", "cube_2d", "adaptive_3d", "adaptive_2d", "ball_3d", "ball_2d"])
def test_plan_ignores_the_mass_coefficient(make):
    mesh = make()
    plain = mf.Plan(mesh.desc, mesh)
    mesh.set_mass_coefficient(np.random.default_rng(0).uniform(0.5, 1.5, mesh.n_cells * mesh.nd))
    assert mesh.desc.mass_coefficient
    with_mass = mf.Plan(mesh.desc, mesh)
    for name in PLAN_ARRAYS:
        np.testing.assert_array_equal(getattr(plain, name), getattr(with_mass, name), err_msg=name)
    assert plain.shares_records == with_mass.shares_records
    assert plain.shares_pass2_records == with_mass.shares_pass2_records
    np.testing.assert_array_equal(mesh.suggest_renumbering(), _renumbering_without_mass(mesh))


def _renumbering_without_mass(mesh):
    keep = mesh.desc.mass_coefficient
    mesh.desc.mass_coefficient = None
    try:
        return mesh.suggest_renumbering()
    finally:
        mesh.desc.mass_coefficient = keep


def test_make_desc_forwards_the_mass_coefficient():
    from oracle import mf_oracle as o
    od = o.uniform_mesh_desc(2, 2, 3)
    c = random_c(od)
    desc, keep = desc_from_oracle(od, mass_coefficient=c)
    got = np.ctypeslib.as_array(ctypes.cast(desc.mass_coefficient, ctypes.POINTER(ctypes.c_double)), shape=(c.size,))
    np.testing.assert_array_equal(got, c.reshape(-1))
    desc, keep = desc_from_oracle(od)
    assert not desc.mass_coefficient


@pytest.mark.parametrize("exe", ["helmholtz-2d-p2", "helmholtz-3d-p4", "helmholtz-3d-p4-adaptive", "helmholtz-3d-p2-ball"])
def test_helmholtz_binaries_exist(exe):
    path = os.path.join(ROOT, "dealii-cuda_amd", "host", "bin", exe)
    assert os.path.isfile(path) and os.access(path, os.X_OK), path
