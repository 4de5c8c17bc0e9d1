"""p-multigrid without a GPU: the library's default 1D matrix of the p-transfer for all 15 degree
pairs against tests/pmg_reference.py and against what it must be, and the algorithm itself -- CG preconditioned by one
V-cycle over h-, p- and hybrid hierarchies -- in the float64 numpy model of pmg_reference.py on the oracle's matrices:
Chebyshev(5, range 15) on Jacobi with lambda_max = 1.2 x the exact largest eigenvalue, exact coarse solve, the reference's
variable coefficient, CG to 1e-10 relative.

Counts of the model with the drivers' right-hand side (b = A x* for x* = sin(0.37 i) + 0.5 cos(0.011 i), zero on the
Dirichlet dofs; a random right-hand side moves a count by at most one); hierarchies are (cells per direction, degree),
coarse to fine:
  2D h-only (2,4)(4,4)(8,4)(16,4)                5      3D h-only (1,4)(2,4)(4,4)                5
  2D p-only (16,1)(16,2)(16,4)                   5      3D p-only (4,1)(4,2)(4,4)                5
  2D hybrid (2,1)(4,1)(8,1)(16,1)(16,2)(16,4)    6      3D hybrid (1,1)(2,1)(4,1)(4,2)(4,4)      5
  2D (16,1)(16,2)(16,3)(16,4)                    5
The assertion is the one that pins the algorithm: a hierarchy with p-levels takes at most one iteration more than the
h-only hierarchy of the same finest level."""
import functools

import numpy as np
import pytest

import pmg_reference as pr
import pymfgpu as mf
from oracle import mf_oracle as o

PAIRS = [(pc, pf) for pf in range(2, 7) for pc in range(1, pf)]
assert len(PAIRS) == 15


@pytest.mark.parametrize("pc,pf", PAIRS)
def test_default_prolongation_1d(pc, pf):
    got = mf.p_prolongation_1d(pc, pf)
    assert got.shape == (pf + 1, pc + 1)
    assert np.abs(got - pr.P1(pc, pf)).max() <= 1e-14
    assert np.abs(got.sum(axis=1) - 1.0).max() <= 1e-14  # the coarse basis is a partition of unity
    xc, xf = o.gll_01(pc), o.gll_01(pf)
    for k in range(pc + 1):  # polynomials of degree <= pc are reproduced at the fine nodes
        assert np.abs(got @ xc ** k - xf ** k).max() <= 1e-13, k
    # a fine node that is a coarse node: exact zeros and a one
    unit = {0: 0, pf: pc}
    if pc % 2 == 0 and pf % 2 == 0:
        unit[pf // 2] = pc // 2
    for X, x in unit.items():
        want = np.zeros(pc + 1)
        want[x] = 1.0
        np.testing.assert_array_equal(got[X], want)


@pytest.mark.parametrize("pc,pf", [(0, 2), (2, 2), (3, 2), (1, 7), (7, 8), (-1, 3)])
def test_default_prolongation_1d_rejects_bad_pairs(pc, pf):
    with pytest.raises(mf.MfgpuError, match="error -1"):
        mf.p_prolongation_1d(pc, pf)


def test_new_symbols_are_exported():
    for name in ("mfgpu_transfer_create_p", "mfgpu_transfer_create_p_from_meshes", "mfgpu_transfer_p_prolongation_1d"):
        assert name in mf.SYMBOLS and hasattr(mf.lib(), name)


def test_owner_rule_counts_every_fine_dof_once():
    """P of the model maps the constant 1 (no Dirichlet dofs) to the constant 1: every fine dof is written once"""
    c, f = mf.Mesh.uniform(2, 2, (3, 2)), mf.Mesh.uniform(2, 5, (3, 2))
    P = pr.p_transfer_matrix(2, 2, 5, c.arrays()["loc2glob"], f.arrays()["loc2glob"], c.n_dofs, f.n_dofs, [])
    assert np.abs(P @ np.ones(c.n_dofs) - 1.0).max() <= 1e-13


HIERARCHIES = {
    "2d_h": (2, [(2, 4), (4, 4), (8, 4), (16, 4)]),
    "2d_p": (2, [(16, 1), (16, 2), (16, 4)]),
    "2d_hybrid": (2, [(2, 1), (4, 1), (8, 1), (16, 1), (16, 2), (16, 4)]),
    "2d_p1234": (2, [(16, 1), (16, 2), (16, 3), (16, 4)]),
    "3d_h": (3, [(1, 4), (2, 4), (4, 4)]),
    "3d_p": (3, [(4, 1), (4, 2), (4, 4)]),
    "3d_hybrid": (3, [(1, 1), (2, 1), (4, 1), (4, 2), (4, 4)]),
}
TABLE = {"2d_h": 5, "2d_p": 5, "2d_hybrid": 6, "2d_p1234": 5, "3d_h": 5, "3d_p": 5, "3d_hybrid": 5}


@functools.lru_cache(maxsize=None)
def model_iterations(name):
    dim, spec = HIERARCHIES[name]
    H = pr.level_hierarchy(pr.meshes_of(dim, spec))
    it, x = pr.cg_iterations(H, pr.rhs(H))
    b = pr.rhs(H)
    assert np.linalg.norm(H.A[-1] @ x - b) <= 1.0001e-10 * np.linalg.norm(b)
    return it


@pytest.mark.parametrize("name", [n for n in HIERARCHIES if not n.endswith("_h")])
def test_p_levels_cost_at_most_one_iteration(name):
    h_only = model_iterations(name[:2] + "_h")
    it = model_iterations(name)
    print(f"{name}: {it} CG iterations, h-only hierarchy of the same finest level {h_only} (table: {TABLE[name]} / "
          f"{TABLE[name[:2] + '_h']})")
    assert it <= h_only + 1
    assert (it, h_only) == (TABLE[name], TABLE[name[:2] + "_h"])  # the table of the module docstring
