"""GPU parity on descriptions no mesh stand-in produces (tests/topology.py; the case table is
test_topology_host.CASES): periodic rings and tori (the planner's box seeding on a walk that wraps), a dof listed twice
by one cell outside the hanging-node case, holes in the numbering, random numberings and cell orders, a pinched vertex
of valence 27 (the run-time-k path of pass 2, beyond the unrolled k and the shared pass-2 records), general geometry on
top.  Every cell-loop kernel family, both number types and both scatter modes against the oracle, which defines
A = sum_c P_c^T K_c P_c for any loc2glob; then properties that need no oracle: permutation equivariance, symmetry, the
constants in the null space of a torus.  Tolerances are test_gpu.TOL (relative l2: 1e-12 in double, 1e-5 in float) and
the rtol of test_gpu_aux for the inverse diagonal."""
import functools

import numpy as np
import pytest

import helmholtz_reference as hr
import pymfgpu as mf
import topology as tp
from oracle import mf_oracle as o
from test_gpu import TOL, gpu_vmult, rel
from test_gpu_aux import TOL as DIAG_TOL
from test_gpu_multi import run_multi
from test_topology_host import CASE, CASES, KERNELS, expected_kernel
from util import desc_from_oracle

pytestmark = pytest.mark.gpu
NTS = [mf.F64, mf.F32]
KERNEL_IDS = ["auto", "pencils_x", "planes", "planes_2w"]
SUBSET = ["ring2-p4", "torus-p4", "pinch27-p2-onecell", "2d-torus-p4"]


def _rounded(v, nt):
    return np.asarray(v).astype(mf.np_dtype(nt)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(name, nt):
    """(x, y0, A x, y0 + A x, 1 / diag A) of a case by the oracle, on vectors rounded to the number type; computed once"""
    od = CASE[name].make()
    rng = np.random.default_rng(len(name) * 7 + od.n_dofs)
    x, y0 = (_rounded(rng.standard_normal(od.n_dofs), nt) for _ in range(2))
    out = x, y0, o.vmult(od, x), o.vmult_add(od, y0, x), o.compute_inverse_diagonal(od)
    for a in out:
        a.setflags(write=False)
    return out


def create(od, kernel, colored, nt, mass=None, **kw):
    """the operator, checked to run the documented kernel -- or None where the documented refusal came, by its message"""
    what, detail = expected_kernel(od, kernel, colored, nt, mass is not None)
    desc, keep = desc_from_oracle(od, number_type=nt, colored=colored, kernel=kernel, mass_coefficient=mass, **kw)
    if colored and not od.uniform_j0:
        # no family has a coloured-scatter instantiation on general geometry: mfgpu_create refuses the description
        # before it looks at mfgpu_desc.kernel (also asserted in test_gpu.py)
        what, detail = "refused", "implemented in two-pass scatter mode only"
    elif what == "refused":
        assert kernel != mf.KERNEL_AUTO  # (the library's own choice never refuses a case)
    if what == "refused":
        with pytest.raises(mf.MfgpuError, match=detail):
            mf.Operator(desc, keep)
        return None
    op = mf.Operator(desc, keep)
    assert op.kernel_name() == detail, (op.kernel_name(), detail)
    return op


def inverse_diagonal(op, n, nt):
    d = mf.DeviceVector(n, nt)
    d.fill(123.0)
    op.compute_inverse_diagonal(d)
    mf.synchronize()
    return d.to_host()


@pytest.mark.parametrize("nt", NTS, ids=["f64", "f32"])
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_vmult_vmult_add_and_diagonal_match_oracle(case, kernel, nt):
    od = case.make()
    x, y0, ref, ref_add, ref_diag = reference(case.name, nt)
    for colored in (False, True):
        op = create(od, kernel, colored, nt, **case.kw)
        if op is None:
            continue
        info = (case.name, kernel, nt, colored, op.kernel_name())
        e1 = rel(gpu_vmult(op, x, nt), ref)  # (dst filled with 7 first; checks that src is untouched)
        e2 = rel(gpu_vmult(op, x, nt, y0=y0), ref_add)
        print(f"{info}: vmult {e1:.3e} vmult_add {e2:.3e}")
        assert e1 <= TOL[nt] and e2 <= TOL[nt], (info, e1, e2)
        np.testing.assert_allclose(inverse_diagonal(op, od.n_dofs, nt), ref_diag, rtol=DIAG_TOL[nt], err_msg=str(info))


@pytest.mark.parametrize("nt", NTS, ids=["f64", "f32"])
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("name", SUBSET)
def test_mass_term(name, kernel, nt):
    case = CASE[name]
    od = case.make()
    c = _rounded(np.random.default_rng(3).uniform(0.5, 1.5, (od.n_cells, od.nd)), nt)
    x, y0 = reference(name, nt)[:2]
    ref, ref_add = hr.vmult(od, c, x), hr.vmult_add(od, c, y0, x)
    for colored in (False, True):
        op = create(od, kernel, colored, nt, mass=c, **case.kw)
        if op is None:
            continue
        info = (name, kernel, nt, colored, op.kernel_name())
        assert rel(gpu_vmult(op, x, nt), ref) <= TOL[nt], info
        assert rel(gpu_vmult(op, x, nt, y0=y0), ref_add) <= TOL[nt], info


@pytest.mark.parametrize("nt", NTS, ids=["f64", "f32"])
@pytest.mark.parametrize("count", [3, 5])
@pytest.mark.parametrize("name", ["general-ring2-p2", "general-ring2-p4"])
def test_vmult_multi_on_the_deformed_ring(name, count, nt):
    od = CASE[name].make()
    op = create(od, mf.KERNEL_AUTO, False, nt)
    assert op.multi_width() > 1  # (the fused sweep of apply_batches_g)
    rng = np.random.default_rng(count)
    X, Y0 = (_rounded(rng.standard_normal((count, od.n_dofs)), nt) for _ in range(2))
    got = run_multi(op, X, nt, stride=od.n_dofs + 37, mode=None)  # (checks src and the padding between the vectors)
    got_add = run_multi(op, X, nt, stride=od.n_dofs + 37, mode=None, Y0=Y0)
    for k in range(count):
        assert rel(got[k], o.vmult(od, X[k])) <= TOL[nt], (name, count, nt, k)
        assert rel(got_add[k], o.vmult_add(od, Y0[k], X[k])) <= TOL[nt], (name, count, nt, k)


@pytest.mark.parametrize("nt", NTS, ids=["f64", "f32"])
@pytest.mark.parametrize("knobs", [dict(cell_loop_segments=1), dict(cell_loop_segments=3), dict(max_workgroups=1)],
                         ids=["segments1", "segments3", "one_workgroup"])
@pytest.mark.parametrize("name", SUBSET)
def test_segments_and_one_workgroup(name, knobs, nt):
    case = CASE[name]
    od = case.make()
    x, y0, ref, ref_add, _ = reference(name, nt)
    for kernel in (mf.KERNEL_AUTO, mf.KERNEL_PENCILS_X):
        op = create(od, kernel, False, nt, **case.kw, **knobs)
        if op is None:
            continue
        info = (name, knobs, nt, op.kernel_name())
        assert rel(gpu_vmult(op, x, nt), ref) <= TOL[nt], info
        assert rel(gpu_vmult(op, x, nt, y0=y0), ref_add) <= TOL[nt], info


# ---- properties that need no oracle


@pytest.mark.parametrize("nt", NTS, ids=["f64", "f32"])
@pytest.mark.parametrize("kernel", [mf.KERNEL_AUTO, mf.KERNEL_PENCILS_X], ids=["auto", "pencils_x"])
@pytest.mark.parametrize("p,n", [(4, (3, 4, 4)), (2, (5, 5, 5))])
def test_permutation_equivariance(p, n, kernel, nt):
    """the operator of a shuffled description on the shuffled vector is the shuffled result of the original operator:
    each side is within TOL of an oracle that is equivariant to rounding, so they agree within 2 TOL"""
    od = o.uniform_mesh_desc(3, p, n)
    t1 = tp.permute_dofs(od, 21)
    t2 = tp.permute_cells(t1.desc, 22)
    x = _rounded(np.random.default_rng(p).standard_normal(od.n_dofs), nt)
    y = gpu_vmult(create(od, kernel, False, nt), x, nt)
    assert rel(tp.pull(t1, o.vmult(t2.desc, tp.push(t1, x))), o.vmult(od, x)) <= 1e-13  # (the oracle's own figure)
    # (shuffled description, the map that carries the vectors; the cells alone leave the numbering as it is)
    variants = {"dofs": (t1.desc, t1), "dofs and cells": (t2.desc, t1), "cells": (tp.permute_cells(od, 23).desc, None)}
    for what, (sd, t) in variants.items():
        ys = gpu_vmult(create(sd, kernel, False, nt), x if t is None else tp.push(t, x), nt)
        assert rel(ys if t is None else tp.pull(t, ys), y) <= 2 * TOL[nt], (p, n, kernel, nt, what)


@pytest.mark.parametrize("nt", NTS, ids=["f64", "f32"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_operator_is_symmetric(case, nt):
    """|x.(A y) - y.(A x)| <= 2 TOL |x| |A y|, the dot products on the host in double"""
    od = case.make()
    x, y = reference(case.name, nt)[:2]
    for colored in (False, True):
        op = create(od, mf.KERNEL_AUTO, colored, nt, **case.kw)
        if op is None:
            continue
        ax, ay = (gpu_vmult(op, v, nt).astype(np.float64) for v in (x, y))
        if "holes" in case.tags:  # (a dof no cell touches and that is not constrained: row and column are zero)
            holes = np.setdiff1d(np.arange(od.n_dofs), np.union1d(od.loc2glob.reshape(-1), od.constrained))
            assert len(holes) > 0 and (ax[holes] == 0).all()
        assert abs(x @ ay - y @ ax) <= 2 * TOL[nt] * np.linalg.norm(x) * np.linalg.norm(ay), (case.name, nt, colored)


@pytest.mark.parametrize("nt", NTS, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["torus-p4", "torus2-p1", "torus2-p2", "2d-torus-p4", "general-2d-torus-p4"])
def test_constants_are_in_the_null_space_on_a_torus(name, nt):
    """no constrained dofs: max |A 1| <= TOL * (largest absolute row sum); test_topology_host shows the oracle's own
    assembled matrix meets this at 1e-13"""
    od = CASE[name].make()
    assert len(od.constrained) == 0
    bound = TOL[nt] * abs(o.assemble(od)).sum(axis=1).max()
    for kernel in KERNELS:
        for colored in (False, True):
            op = create(od, kernel, colored, nt)
            if op is not None:
                got = np.abs(gpu_vmult(op, np.ones(od.n_dofs), nt)).max()
                assert got <= bound, (name, nt, kernel, colored, got, bound)
