"""Host checks of tests/vqop_reference.py, the checker of the vector-valued operator mfgpu_vqop_*, and of the part of the
new ABI that needs no device.  Small 2D / 3D meshes at p = 1, 2 with one hanging-node mesh and one ball per dimension
that has one."""
import ctypes as C

import numpy as np
import pytest

import poisson_reference as pr
import pymfgpu as mf
import qop_reference as qr
import vqop_reference as vr

MESHES = [("cube", 2, 2), ("cube", 3, 1), ("hanging", 2, 2), ("ball", 2, 2), ("ball", 3, 1)]

_cells = {}


def cells_of(kind, dim, p, dirichlet=True):
    key = (kind, dim, p, dirichlet)
    if key not in _cells:
        mesh = pr.family(kind, dim, p, 0)
        if not dirichlet:
            mesh.desc.n_constrained = 0  # every dof free
        _cells[key] = pr.Cells(mesh)
    return _cells[key]


def vfields(cells, seed):
    """seeded coefficients: lam, mu, mass positive; tensor random without any symmetry; tensor_pos the isotropic tensor
    plus a perturbation of 0.05, without symmetry either: its blocks C[a][.][a][.] have a symmetric part >= mu - 0.05 dim
    >= 0.35, so the diagonal of the operator is a sum of positive terms"""
    od, dim = cells.od, cells.dim
    rng = np.random.default_rng(seed)
    shape = (od.n_cells, od.nd)
    f = {"lam": rng.uniform(0.5, 2.0, shape), "mu": rng.uniform(0.5, 2.0, shape),
         "tensor": rng.standard_normal(shape + (dim,) * 4) + 3.0 * vr.isotropic_tensor(0.0, 0.5, dim),
         "mass": rng.uniform(0.5, 2.0, shape)}
    f["tensor_pos"] = vr.isotropic_tensor(f["lam"], f["mu"], dim) + rng.uniform(-0.05, 0.05, shape + (dim,) * 4)
    return f


def pick(f, *names):
    return {k: f[k] for k in names}


TERM_SETS = [("lam", "mu"), ("tensor",), ("mass",), ("lam", "mu", "mass"), ("tensor", "mass")]


@pytest.mark.parametrize("kind,dim,p", MESHES)
def test_apply_is_the_assembled_matrix(kind, dim, p):
    c = cells_of(kind, dim, p)
    f = vfields(c, 1)
    x = np.random.default_rng(2).standard_normal(dim * c.od.n_dofs)
    for names in TERM_SETS:
        t = pick(f, *names)
        y, A = vr.apply(c, x, **t), vr.assemble(c, **t)
        assert np.linalg.norm(y - A @ x) <= 1e-12 * np.linalg.norm(y), names
        d = vr.diagonal(c, **t)
        assert np.abs(d - A.diagonal()).max() <= 1e-12 * np.abs(d).max(), names


@pytest.mark.parametrize("kind,dim,p", MESHES)
def test_isotropic_matrix_is_symmetric_and_equals_the_tensor_form(kind, dim, p):
    c = cells_of(kind, dim, p)
    f = vfields(c, 3)
    A = vr.assemble(c, lam=f["lam"], mu=f["mu"], mass=f["mass"])
    assert abs(A - A.T).max() <= 1e-12 * abs(A).max()
    x = np.random.default_rng(4).standard_normal(dim * c.od.n_dofs)
    y = vr.apply(c, x, lam=f["lam"], mu=f["mu"])
    z = vr.apply(c, x, tensor=vr.isotropic_tensor(f["lam"], f["mu"], dim))
    assert np.linalg.norm(y - z) <= 1e-12 * np.linalg.norm(y)


@pytest.mark.parametrize("kind,dim,p", MESHES)
def test_decoupled_tensor_gives_the_scalar_operator_in_every_block(kind, dim, p):
    """C = a d_ab d_kl: component a of sigma is a grad u_a"""
    c = cells_of(kind, dim, p)
    n = c.od.n_dofs
    a = vfields(c, 5)["lam"]
    d = np.eye(dim)
    A = vr.assemble(c, tensor=a[..., None, None, None, None] * np.einsum("ab,kl->akbl", d, d))
    ref = qr.assemble(c, diffusion=a)
    for i in range(dim):
        for j in range(dim):
            blk = A[i * n:(i + 1) * n, j * n:(j + 1) * n]
            want = ref if i == j else 0.0 * ref
            assert abs(blk - want).max() <= 1e-12 * abs(ref).max()


def rigid_body_modes(cells):
    """translations and the infinitesimal rotations u = W x, W skew: dim (dim + 1) / 2 block vectors"""
    dim, x = cells.dim, cells.dof_coords
    modes = []
    for a in range(dim):
        t = np.zeros((dim, len(x)))
        t[a] = 1.0
        modes.append(t.reshape(-1))
    for a in range(dim):
        for b in range(a + 1, dim):
            W = np.zeros((dim, dim))
            W[a, b], W[b, a] = 1.0, -1.0
            modes.append((W @ x.T).reshape(-1))
    return modes


@pytest.mark.parametrize("kind,dim,p", [("cube", 2, 2), ("cube", 3, 1), ("ball", 2, 2), ("ball", 3, 1)])
def test_rigid_body_modes_are_in_the_null_space(kind, dim, p):
    c = cells_of(kind, dim, p, dirichlet=False)
    assert len(c.od.constrained) == 0
    f = vfields(c, 6)
    A = vr.assemble(c, lam=f["lam"], mu=f["mu"], constrained=[])
    fro = np.sqrt(A.multiply(A).sum())
    modes = rigid_body_modes(c)
    assert len(modes) == dim * (dim + 1) // 2
    for r in modes:
        assert np.linalg.norm(vr.apply(c, r, lam=f["lam"], mu=f["mu"], constrained=[])) <= 1e-12 * fro * np.linalg.norm(r)
        assert np.linalg.norm(A @ r) <= 1e-12 * fro * np.linalg.norm(r)


def test_per_component_constraints_and_the_inverse_diagonal():
    c = cells_of("hanging", 2, 2)
    od = c.od
    f = vfields(c, 7)
    # component 1 free on the Dirichlet dofs of the right half: not what the GPU accepts (its gather lists are the
    # description's), but the reference takes any list
    keep = np.concatenate([od.constrained, od.n_dofs + od.constrained[c.dof_coords[od.constrained, 0] < 0.0]])
    keep = np.unique(keep)
    x = np.random.default_rng(8).standard_normal(2 * od.n_dofs)
    A = vr.assemble(c, lam=f["lam"], mu=f["mu"], constrained=keep)
    y = vr.apply(c, x, lam=f["lam"], mu=f["mu"], constrained=keep)
    assert np.linalg.norm(y - A @ x) <= 1e-12 * np.linalg.norm(y)
    np.testing.assert_array_equal(y[keep], x[keep])
    d = vr.inverse_diagonal(c, lam=f["lam"], mu=f["mu"], constrained=keep)
    unref = np.ones(od.n_dofs, bool)
    unref[od.loc2glob.reshape(-1)] = False
    assert unref.any() and np.all(d[np.tile(unref, 2)] == 1.0) and np.all(d[keep] == 1.0) and np.all(np.isfinite(d))


def test_argument_errors_without_a_device():
    L = mf.lib()
    for s in ("mfgpu_vqop_create", "mfgpu_vqop_set_coefficients", "mfgpu_vqop_vmult",
              "mfgpu_vqop_compute_inverse_diagonal", "mfgpu_vqop_set_constrained_values",
              "mfgpu_vqop_memory_consumption", "mfgpu_vqop_destroy", "mfgpu_bicgstab_set_operator_vqop"):
        assert s in mf.SYMBOLS and hasattr(L, s)
    h = C.c_void_p()
    assert L.mfgpu_vqop_create(None, mf.VQOP_MASS, None, 0, C.byref(h)) == mf.EINVAL and not h.value
    assert L.mfgpu_vqop_create(None, 0, None, 0, None) == mf.EINVAL
    co = mf.VqopCoefficients()
    assert L.mfgpu_vqop_set_coefficients(None, C.byref(co), None) == mf.EINVAL
    assert L.mfgpu_vqop_vmult(None, None, None, None) == mf.EINVAL
    assert L.mfgpu_vqop_compute_inverse_diagonal(None, None, None) == mf.EINVAL
    assert L.mfgpu_vqop_set_constrained_values(None, None, 0.0, None) == mf.EINVAL
    assert L.mfgpu_vqop_memory_consumption(None) == 0
    L.mfgpu_vqop_destroy(None)
    assert L.mfgpu_bicgstab_set_operator_vqop(None, None) == mf.EINVAL
    assert (mf.VQOP_ISOTROPIC, mf.VQOP_TENSOR4, mf.VQOP_MASS) == (1, 2, 4)
    assert C.sizeof(mf.VqopCoefficients) == 4 * C.sizeof(C.c_void_p)
