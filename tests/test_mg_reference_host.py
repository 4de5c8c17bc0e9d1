"""Keeps tests/mg_reference.py honest without a GPU (tests/test_gpu_mg_parity.py compares the GPU V-cycle with it value
for value).  On the hierarchies of Mesh.adaptive_mg(2, 2, 3) (711 dofs, 6 levels, a refinement edge that reaches the boundary)
and Mesh.adaptive_mg(2, 2, 4) (27245 dofs, 12 levels):
  - every sparse matrix of the reference against the oracle function it restates, on random vectors;
  - the V-cycle's matrix: symmetric (equal pre- and post-smoothing polynomials make it so) and positive definite on
    the free dofs.  On the small mesh the matrix is built column by column; on the large one, where it would be 20425^2
    dense entries (3.3 GB and eleven minutes of CPU), symmetry is <M x, y> = <x, M y> and definiteness <x, M x> > 0 on
    random vectors;
  - CG preconditioned with it reaches 1e-10 |b| in at most the 25 iterations test_gpu_mg_adaptive.py allows, and the
    sparse direct solution."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import mg_reference as mg
from oracle import mf_oracle as o
from util import oracle_desc_from_mesh


@pytest.fixture(scope="module", params=[3, 4], ids=["n_ref3", "n_ref4"])
def hier(request):
    return mg.Hierarchy(2, 2, request.param)


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def test_matrices_are_the_oracle_pieces(hier):
    h = hier
    rng = np.random.default_rng(0)
    assert h.n_levels >= 3 and any(len(E) for E in h.edge)
    for l in range(h.n_levels):
        od, odc, E = h.od[l], h.odc[l], h.edge[l]
        x = rng.standard_normal(od.n_dofs)
        assert _rel(h.A[l] @ x, o.vmult(odc, x)) <= 1e-13
        if len(E):
            assert _rel(h.down[l] @ x, o.vmult_interface_down(od, E, x)) <= 1e-13
            assert _rel(h.up[l] @ x, o.vmult_interface_up(od, E, x)) <= 1e-13
        else:
            assert h.down[l].nnz == 0 and h.up[l].nnz == 0
        np.testing.assert_array_equal(h.dinv[l][odc.constrained], 1.0)
        np.testing.assert_allclose(1.0 / h.dinv[l], h.A[l].diagonal(), rtol=1e-12)
        # lambda_max: 1.2 times the largest eigenvalue of D^-1 A, against the dense spectrum
        if od.n_dofs <= 2000:
            lam = np.linalg.eigvals(h.dinv[l][:, None] * h.A[l].toarray()).real.max()
            assert abs(h.lmax[l] - 1.2 * lam) <= 1e-9 * lam
        if l > 0:
            cd, fd = h.patches[l]
            C = h.od[l - 1]
            xc, yf, z = rng.standard_normal(C.n_dofs), rng.standard_normal(od.n_dofs), rng.standard_normal(C.n_dofs)
            assert _rel(h.P[l] @ xc, o.mg_prolongate(h.dim, h.p, cd, fd, od.n_dofs, C.constrained, xc)) <= 1e-13
            assert _rel(z + h.P[l].T @ yf,
                        o.mg_restrict_and_add(h.dim, h.p, cd, fd, C.n_dofs, C.constrained, z, yf)) <= 1e-13


def test_block_of_vectors_is_the_vectors_one_by_one(hier):
    r = np.random.default_rng(1).standard_normal((hier.mesh.n_dofs, 3))
    Z = hier.vcycle(r)
    for k in range(3):
        assert _rel(Z[:, k], hier.vcycle(r[:, k])) <= 1e-13


def test_vcycle_is_a_symmetric_positive_definite_preconditioner(hier):
    h = hier
    N = h.mesh.n_dofs
    od = oracle_desc_from_mesh(h.mesh)
    free = np.setdiff1d(np.arange(N), od.constrained)  # Dirichlet and hanging-node dofs are constrained
    if N <= 2000:
        M = h.vcycle(np.eye(N)[:, free])[free]         # column j = V-cycle of e_j
        assert np.abs(M - M.T).max() <= 1e-10 * np.abs(M).max()
        ev = np.linalg.eigvalsh(0.5 * (M + M.T))
        print(f"V-cycle matrix on {len(free)} free dofs: eigenvalues in [{ev[0]:.3e}, {ev[-1]:.3e}]")
        assert ev[0] > 0
    else:
        X = np.zeros((N, 8))
        X[free] = np.random.default_rng(3).standard_normal((len(free), 8))
        G = X.T @ h.vcycle(X)                          # G[i, j] = <x_i, M x_j>
        assert np.abs(G - G.T).max() <= 1e-10 * np.abs(G).max()
        assert np.linalg.eigvalsh(0.5 * (G + G.T))[0] > 0
    # preconditioned CG on the active-mesh operator (hanging nodes included), against spsolve
    A = o.assemble(od).tocsr()
    b = np.zeros(N)
    b[free] = np.random.default_rng(2).standard_normal(len(free))
    x, r = np.zeros(N), b.copy()
    z = h.vcycle(r)
    pv, rz, r0 = z.copy(), r @ z, np.linalg.norm(r)
    for it in range(1, 80):
        q = A @ pv
        alpha = rz / (pv @ q)
        x += alpha * pv
        r -= alpha * q
        if np.linalg.norm(r) <= 1e-10 * r0:
            break
        z = h.vcycle(r)
        rz, rz_old = r @ z, rz
        pv = z + (rz / rz_old) * pv
    print(f"CG iterations with the reference V-cycle: {it}")
    assert it <= 25
    xr = spla.spsolve(A.tocsc(), b)
    assert np.linalg.norm(x - xr) <= 1e-8 * np.linalg.norm(xr)
